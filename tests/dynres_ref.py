"""numpy / plain-Python fp64 restatement of the per-particle resolution lambda (rule set: include/chem_mi355.h,
chem_nb_resolution, chem_resolution_rate, chem_set_resolution) and brute-force references built on it.  Shared by
tests/test_host_resolution.py and tests/test_gpu_resolution.py.  Imports nothing from the product; the LJ and table
arithmetic comes from tests/spline_ref.py.

Rule set.  lambda(s) = min(1.0, lambda0 + alpha * float(s - s0)), two roundings, no fused multiply-add (Python floats).
s_full = the first step s >= s0 at which that expression is >= 1.0.  For every pair that is not excluded, whose type pair
carries a potential and whose minimum-image distance has r^2 <= rc^2: an unmarked type pair contributes F_pot and U; a marked
one w = lambda_i lambda_j times them, nothing at all if w == 0, the force rescaled to |F| = max_force where max_force > 0 and
|w F_pot| > max_force (the energy stays w U); the virial is the sum over pairs of r_ij . F_ij of the applied force."""
import numpy as np

import spline_ref as S


# ---- lambda as a function of the step ------------------------------------------------------------------------------------

def lam(l0, s0, alpha, s):
    ramp = float(alpha) * float(s - s0)
    return min(1.0, float(l0) + ramp)


def s_full(l0, s0, alpha):
    """by stepping: no division, so independent of the product's estimate-and-correct routine; None = never"""
    if l0 >= 1.0:
        return s0
    if not alpha > 0.0:
        return None
    k = max(0, int((1.0 - l0) / alpha) - 3)
    while float(l0) + float(alpha) * float(k) < 1.0:
        k += 1
    assert k == 0 or float(l0) + float(alpha) * float(k - 1) < 1.0
    return s0 + k


def pieces(step, nsteps, fulls):
    """lengths of the pieces of run(nsteps) from `step` that end at every s_full in `fulls` inside (step, step + nsteps)"""
    cuts = sorted({f for f in fulls if f is not None and step < f < step + nsteps})
    edges = [step] + cuts + [step + nsteps]
    return [b - a for a, b in zip(edges[:-1], edges[1:])] if nsteps > 0 else []


class Stamps:
    """the stamps of a set of particles as plain Python: per particle [lambda0, s0], the type it was taken under; per type
    the rate and the change (new_type or None)"""

    def __init__(self, types):
        self.types = list(types)
        self.st = [[1.0, 0] for _ in types]
        self.rate = {}

    def alpha(self, t):
        return self.rate.get(t, (0.0, None))[0]

    def lam(self, i, s):
        return lam(self.st[i][0], self.st[i][1], self.alpha(self.types[i]), s)

    def set_lambda(self, i, v, s):
        self.st[i] = [float(v), s]

    def set_type(self, i, t, s):
        self.st[i] = [self.lam(i, s), s]
        self.types[i] = t

    def set_rate(self, t, alpha, s, new_type=None):
        for i, ty in enumerate(self.types):
            if ty == t and self.st[i][0] < 1.0:
                self.st[i] = [self.lam(i, s), s]
        if alpha > 0.0:
            self.rate[t] = (alpha, new_type)
        else:
            self.rate.pop(t, None)

    def full(self, i):
        a, nt = self.rate.get(self.types[i], (0.0, None))
        if not self.st[i][0] < 1.0 or nt is None or not a > 0.0:
            return None
        return s_full(self.st[i][0], self.st[i][1], a)

    def complete(self, s):
        """apply every change whose s_full <= s; returns the particles that changed"""
        done = [i for i in range(len(self.types)) if self.full(i) is not None and self.full(i) <= s]
        for i in done:
            self.types[i] = self.rate[self.types[i]][1]
            self.st[i] = [1.0, s]
        return done


# ---- brute-force pair sums -----------------------------------------------------------------------------------------------

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


def pair_terms(pos, box, types, lam_, matrix, marked, excluded=()):
    """Every interacting pair: dict of index arrays i, j, the displacement d = x_i - x_j, r2, the unscaled scalar ff (F = ff d)
    and energy u, the weight w (1 for unmarked pairs), flags `marked`, `is_lj`, the cap (0: none) and the pair's cutoff.
    matrix as spline_ref.pair_sums takes it; marked: {(t1, t2) with t1 <= t2: max_force}.  Marked pairs with w == 0 are kept
    in the arrays (with w = 0) so that guards can look at them."""
    types, lam_ = np.asarray(types), np.asarray(lam_, np.float64)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    out = {k: [] for k in ("i", "j", "d", "r2", "ff", "u", "w", "marked", "is_lj", "cap", "rc")}
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        sel = np.nonzero(live & (ti == t1) & (tj == t2) & (r2 <= rc * rc))[0]
        q = r2[sel]
        if prm[0] == "lj":
            _, eps, sig, _, shift = prm
            s6 = (sig * sig / q) ** 3
            ff = 24.0 * eps * (2.0 * s6 * s6 - s6) / q
            u = 4.0 * eps * (s6 * s6 - s6) + shift
        else:
            r = np.sqrt(q)
            u, fv = prm[1](r)
            ff = fv / r
        mk = (t1, t2) in marked
        w = lam_[iu[0][sel]] * lam_[iu[1][sel]] if mk else np.ones(len(sel))
        out["i"].append(iu[0][sel]); out["j"].append(iu[1][sel]); out["d"].append(d[sel]); out["r2"].append(q)
        out["ff"].append(ff); out["u"].append(u); out["w"].append(w)
        out["marked"].append(np.full(len(sel), mk)); out["is_lj"].append(np.full(len(sel), prm[0] == "lj"))
        out["cap"].append(np.full(len(sel), float(marked.get((t1, t2), 0.0)) if mk else 0.0)); out["rc"].append(np.full(len(sel), rc))
    return {k: (np.concatenate(v) if len(v) else np.zeros((0, 3) if k == "d" else 0)) for k, v in out.items()}


def total(pos, box, types, lam_, matrix, marked, excluded=()):
    """dict of forces F, energies e_lj / e_tab, the virial w_nb, and the pair arrays (`pairs`, with `fs` = the scalar that was
    applied: F_ij = fs d)"""
    p = pair_terms(pos, box, types, lam_, matrix, marked, excluded)
    fs = p["w"] * p["ff"]
    mag = np.abs(fs) * np.sqrt(p["r2"])
    capped = (p["cap"] > 0.0) & (mag > p["cap"])
    fs = np.where(capped, fs * (p["cap"] / np.where(capped, mag, 1.0)), fs)
    on = p["w"] != 0.0
    fvec = np.where(on[:, None], fs[:, None] * p["d"], 0.0)
    F = np.zeros((len(pos), 3))
    np.add.at(F, p["i"], fvec)
    np.add.at(F, p["j"], -fvec)
    e = np.where(on, p["w"] * p["u"], 0.0)
    p["fs"], p["capped"] = np.where(on, fs, 0.0), capped & on
    return dict(F=F, e_lj=e[p["is_lj"]].sum(), e_tab=e[~p["is_lj"]].sum(), w_nb=(p["fs"] * p["r2"]).sum(), pairs=p)


def energy(pos, box, types, lam_, matrix, marked, excluded=()):
    t = total(pos, box, types, lam_, matrix, marked, excluded)
    return t["e_lj"] + t["e_tab"]


def gap_to_cutoff(pos, box, types, lam_, matrix, marked, excluded=()):
    """smallest | r - rc | over the pairs, on either side of their cutoff, that carry a non-zero term there: the truncated
    force is discontinuous at rc, so a pair this close can be decided differently in fp32"""
    types, lam_ = np.asarray(types), np.asarray(lam_, np.float64)
    iu, d, r2, live = _pairs(pos, box, excluded)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    gap = np.inf
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        ok = live & (ti == t1) & (tj == t2)
        if (t1, t2) in marked:
            ok &= lam_[iu[0]] * lam_[iu[1]] != 0.0
        if ok.any():
            gap = min(gap, np.abs(np.sqrt(r2[ok]) - rc).min())
    return gap
