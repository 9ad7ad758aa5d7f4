"""numpy fp64 restatement of the capped pair potentials (rule set: include/chem_mi355.h, chem_nb_cap) and a brute-force
all-pairs reference built on it.  Shared by tests/test_capped_ref.py, tests/test_gpu_capped.py and tests/test_driver_capped.py.
Imports nothing from the product; the LJ and table arithmetic comes from tests/spline_ref.py.

Rule set.  For every pair that is not excluded, whose type pair carries a potential and whose minimum-image distance has
r^2 <= rc^2: with c the cap radius of the type pair (none: c = 0), r_e = c if r^2 < c^2, else r (decided on the squares).
F_i = f(r_e) / r * r_ij with f the potential's force magnitude, zero at r = 0; the energy is U(r_e) (plus the LJ shift); the
virial share is r . F of the applied force.  Optionally the resolution rule of tests/dynres_ref.py on OTHER type pairs: a
marked pair's term is scaled by w = lambda_i lambda_j and its force then capped at max_force; a type pair is never both."""
import numpy as np

import spline_ref as S  # noqa: F401  (matrix entries are spline_ref.lj tuples and spline_ref.Table objects)


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


def pot_at(prm, r):
    """(u, f) of a matrix entry at the distances r: the energy (with the LJ shift) and the force magnitude f = -dU/dr"""
    r = np.asarray(r, np.float64)
    if prm[0] == "lj":
        _, eps, sig, _, shift = prm
        s6 = (sig / r) ** 6
        return 4.0 * eps * (s6 * s6 - s6) + shift, 24.0 * eps * (2.0 * s6 * s6 - s6) / r
    return prm[1](r)


def pair_terms(pos, box, types, matrix, caps, lam=None, marked=None, excluded=()):
    """Every interacting pair: index arrays i, j, the displacement d = x_i - x_j, r2, the evaluation radius re, the scalar
    ff of the unscaled term (F = ff d; 0 at r = 0), its energy u, the weight w (1 unless the type pair is marked), flags
    `inside` (r < c), `capped` (the type pair has a cap), `marked`, `is_lj`, the force cap fmax of marked pairs, and the cutoff.
    matrix: {(t1, t2) with t1 <= t2: ("lj", eps, sig, rc, shift) | ("tab", Table, rc)}; caps: {(t1, t2): caprad};
    marked: {(t1, t2): max_force} with lam the lambda per particle (dynres_ref's rule)."""
    types = np.asarray(types)
    marked = marked or {}
    assert not set(marked) & {k for k, c in caps.items() if c > 0}, "a type pair is capped or resolution-marked, not both"
    lam = np.ones(len(types)) if lam is None else np.asarray(lam, np.float64)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    keys = ("i", "j", "d", "r2", "re", "ff", "u", "w", "inside", "capped", "marked", "is_lj", "fmax", "rc")
    out = {k: [] for k in keys}
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        c = float(caps.get((t1, t2), 0.0))
        c = c if c > 0 else 0.0
        sel = np.nonzero(live & (ti == t1) & (tj == t2) & (r2 <= rc * rc))[0]
        q = r2[sel]
        inside = q < c * c
        re = np.where(inside, c, np.sqrt(q))
        u, f = pot_at(prm, np.where(re > 0, re, 1.0))
        r = np.sqrt(q)
        ff = np.where(r > 0, f / np.where(r > 0, r, 1.0), 0.0)
        mk = (t1, t2) in marked
        w = lam[iu[0][sel]] * lam[iu[1][sel]] if mk else np.ones(len(sel))
        m = len(sel)
        for k, v in zip(keys, (iu[0][sel], iu[1][sel], d[sel], q, re, ff, u, w, inside, np.full(m, c > 0), np.full(m, mk),
                               np.full(m, prm[0] == "lj"), np.full(m, float(marked.get((t1, t2), 0.0)) if mk else 0.0), np.full(m, rc))):
            out[k].append(v)
    return {k: (np.concatenate(v) if len(v) else np.zeros((0, 3) if k == "d" else 0)) for k, v in out.items()}


def total(pos, box, types, matrix, caps, lam=None, marked=None, excluded=()):
    """dict of forces F, energies e_lj / e_tab, the virial w_nb and the pair records (`pairs`, with `fs` = the scalar that
    was applied: F_ij = fs d)"""
    p = pair_terms(pos, box, types, matrix, caps, lam, marked, excluded)
    fs = p["w"] * p["ff"]
    mag = np.abs(fs) * np.sqrt(p["r2"])
    limited = (p["fmax"] > 0.0) & (mag > p["fmax"])
    fs = np.where(limited, fs * (p["fmax"] / np.where(limited, mag, 1.0)), fs)
    on = p["w"] != 0.0
    fs = np.where(on, fs, 0.0)
    fvec = fs[:, None] * p["d"]
    F = np.zeros((len(pos), 3))
    np.add.at(F, p["i"].astype(int), fvec)
    np.add.at(F, p["j"].astype(int), -fvec)
    e = np.where(on, p["w"] * p["u"], 0.0)
    lj = p["is_lj"].astype(bool)
    p["fs"] = fs
    return dict(F=F, e_lj=e[lj].sum(), e_tab=e[~lj].sum(), w_nb=(fs * p["r2"]).sum(), pairs=p)


def gap_to_cutoff(pos, box, types, matrix, lam=None, marked=None, excluded=()):
    """smallest | r - rc | over the pairs, on either side of their cutoff, that carry a non-zero term there (the truncated
    force jumps at rc; at the cap radius force and energy are continuous, so no such gap is needed there)"""
    types = np.asarray(types)
    marked = marked or {}
    lam = np.ones(len(types)) if lam is None else np.asarray(lam, np.float64)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    gap = np.inf
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        ok = live & (ti == t1) & (tj == t2)
        if (t1, t2) in marked:
            ok &= lam[iu[0]] * lam[iu[1]] != 0.0
        if ok.any():
            gap = min(gap, np.abs(np.sqrt(r2[ok]) - rc).min())
    return gap
