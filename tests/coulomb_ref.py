"""numpy fp64 restatement of the truncated Coulomb term (rule set: include/chem_mi355.h, chem_nb_coulomb) and brute-force
references built on it.  Shared by tests/test_host_coulomb.py and tests/test_gpu_coulomb.py.  Imports nothing from the
product; the LJ, table and bond parts come from tests/spline_ref.py.

Rule set: for every pair that is not excluded, whose type pair is in the mask and whose minimum-image distance has
r^2 <= rc_qq^2 (inclusive):  U = k q_i q_j / r,  F_i = k q_i q_j r_ij / r^3  (r_ij = x_i - x_j), no energy shift; the term
is added on top of whatever else the type pair carries."""
import numpy as np

import spline_ref as S


def _pairs(pos, box, excluded):
    pos, box = np.asarray(pos, np.float64), np.asarray(box, np.float64)
    n = len(pos)
    iu = np.triu_indices(n, 1)
    d = pos[iu[0]] - pos[iu[1]]
    d -= box * np.rint(d / box)
    r2 = (d * d).sum(1)
    live = np.ones(len(r2), dtype=bool)
    if len(excluded):
        ex = np.zeros((n, n), dtype=bool)
        for a, b in excluded:
            ex[a, b] = ex[b, a] = True
        live = ~ex[iu]
    return iu, d, r2, live


def coulomb_energy(pos, box, types, q, k, rc, mask, excluded=()):
    """the energy alone (for the finite-difference check of the forces)"""
    return coulomb_sums(pos, box, types, q, k, rc, mask, excluded)[1]


def coulomb_sums(pos, box, types, q, k, rc, mask, excluded=()):
    """mask: set of type pairs (t1, t2) with t1 <= t2 that carry the term; excluded: index pairs (0-based) left out.
    Returns forces, energy, virial (sum over pairs of r_ij . F_ij)."""
    types, q = np.asarray(types), np.asarray(q, np.float64)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    on = np.zeros(len(r2), dtype=bool)
    for t1, t2 in mask:
        on |= (ti == min(t1, t2)) & (tj == max(t1, t2))
    sel = np.nonzero(live & on & (r2 <= rc * rc))[0]
    r = np.sqrt(r2[sel])
    e = k * q[iu[0][sel]] * q[iu[1][sel]] / r
    ff = e / r2[sel]
    fvec = ff[:, None] * d[sel]
    F = np.zeros((len(q), 3))
    np.add.at(F, iu[0][sel], fvec)
    np.add.at(F, iu[1][sel], -fvec)
    return F, e.sum(), (ff * r2[sel]).sum()


def pair_virial(pos, box, types, matrix, excluded=()):
    """sum over pairs of r_ij . F_ij of the LJ / table matrix of spline_ref.pair_sums (which returns no virial)"""
    types = np.asarray(types)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    w = 0.0
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        x = r2[live & (ti == t1) & (tj == t2) & (r2 <= rc * rc)]
        if prm[0] == "lj":
            s6 = (prm[2] * prm[2] / x) ** 3
            w += (24.0 * prm[1] * (2.0 * s6 * s6 - s6)).sum()
        else:
            r = np.sqrt(x)
            w += (prm[1](r)[1] * r).sum()
    return w


def min_gap_to_cutoff(pos, box, rc, excluded=()):
    """smallest | r - rc | over all pairs: the unshifted force is discontinuous at rc"""
    _, _, r2, live = _pairs(pos, box, excluded)
    return np.abs(np.sqrt(r2[live]) - rc).min()


def total(pos, box, types, q, matrix, k, rc, mask, excluded=()):
    """LJ / table matrix (spline_ref.pair_sums) plus the Coulomb term: dict of forces, the Coulomb part of them, energies
    and virials"""
    Fp, e_lj, e_tab = S.pair_sums(pos, box, types, matrix, excluded=excluded)
    Fq, e_q, w_q = coulomb_sums(pos, box, types, q, k, rc, mask, excluded)
    return dict(F=Fp + Fq, Fq=Fq, e_lj=e_lj, e_tab=e_tab, e_q=e_q, w_q=w_q, w_nb=pair_virial(pos, box, types, matrix, excluded) + w_q)
