"""numpy fp64 restatement of the 1-4 Coulomb pair lists (include/chem_mi355.h, CHEM_POT_COULOMB_BOND) for the tests.  Imports
nothing from the product.  For a list entry (i, j) with minimum-image distance r <= rc (inclusive):
    U = k q_i q_j / r,     F_i = k q_i q_j r_ij / r^3,     no energy shift;
nothing else is asked of the entry (exclusions and the Verlet list do not matter).  By types: (k, rc) of the entry's current
type pair, nothing for a type pair without parameters.  Hybrid lists: force and energy times the entry's lambda."""
import numpy as np


def entry_params(pairs, k, rc, types=None, typed=None):
    """(k, rc) per entry: the plain parameters, or those of the unordered type pair from `typed` ({(t1, t2): (k, rc)};
    k = 0 where the pair has none)"""
    b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if typed is None:
        return np.full(len(b), float(k)), np.full(len(b), float(rc))
    look = {}
    for (t1, t2), p in typed.items():
        look[(int(t1), int(t2))] = look[(int(t2), int(t1))] = p
    ty = np.asarray(types)
    kk, rr = np.zeros(len(b)), np.ones(len(b))
    for e, (i, j) in enumerate(b.tolist()):
        p = look.get((int(ty[i]), int(ty[j])))
        if p is not None:
            kk[e], rr[e] = p
    return kk, rr


def distances(pos, box, pairs):
    b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    box = np.asarray(box, dtype=np.float64)
    d = np.asarray(pos, dtype=np.float64)[b[:, 0]] - np.asarray(pos, dtype=np.float64)[b[:, 1]]
    d -= box * np.rint(d / box)
    return b, d, np.sqrt((d * d).sum(1))


def terms(pos, box, q, pairs, k=0.0, rc=1.0, types=None, typed=None, lam=None):
    """pairs: 0-based index pairs.  Returns (per-particle forces, list energy)."""
    F = np.zeros((len(pos), 3))
    b, d, r = distances(pos, box, pairs)
    if len(b) == 0:
        return F, 0.0
    kk, rr = entry_params(b, k, rc, types, typed)
    q = np.asarray(q, dtype=np.float64)
    lam = np.ones(len(b)) if lam is None else np.asarray(lam, dtype=np.float64)
    inside = r <= rr
    u = np.where(inside, lam * kk * q[b[:, 0]] * q[b[:, 1]] / r, 0.0)
    fvec = (u / (r * r))[:, None] * d
    np.add.at(F, b[:, 0], fvec)
    np.add.at(F, b[:, 1], -fvec)
    return F, float(u.sum())


def energy(pos, box, q, pairs, k=0.0, rc=1.0, types=None, typed=None, lam=None):
    return terms(pos, box, q, pairs, k, rc, types, typed, lam)[1]


def live(q, pairs):
    """mask of the entries with q_i q_j != 0"""
    b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    q = np.asarray(q, dtype=np.float64)
    return q[b[:, 0]] * q[b[:, 1]] != 0.0
