"""numpy restatement of the hybrid pair lists (include/chem_mi355.h, chem_list_set_hybrid) for the tests: the ramp
lambda = min(1, lambda0 + rate (step - birth)), birth steps from the event log, and the per-bond terms lambda F, lambda U that
are ADDED to the CPU oracle's result for the same configuration without the hybrid list.  Imports nothing from the product.
Built the way tests/spline_ref.py bond_terms is: F_ij = f(r) / r * r_ij on the minimum image."""
import numpy as np


def ramp(lambda0, rate, step, birth):
    return np.minimum(1.0, lambda0 + rate * (step - np.asarray(birth, dtype=np.float64)))


def births(events, reactions, bonds):
    """events: rows (step, id_a, id_b, reaction) in log order; reactions: the indices that FORM bonds of this list.
    Returns the step of the last such event of every pair of `bonds` (id pairs, either orientation)."""
    last = {}
    for step, a, b, r in events:
        if r in reactions:
            last[(min(a, b), max(a, b))] = step
    return np.array([last[(min(a, b), max(a, b))] for a, b in np.asarray(bonds).tolist()], dtype=np.int64)


def harmonic(K, r0):
    return lambda r: (K * (r - r0) ** 2, -2.0 * K * (r - r0))


def fene(K, r0, rmax):
    def fun(r):
        q = (r - r0) / rmax
        return -0.5 * K * rmax * rmax * np.log(1.0 - q * q), -K * (r - r0) / (1.0 - q * q)
    return fun


def table(r0, dr, e, f):
    """linear interpolation of both columns, the end rows beyond the grid (chem_table_create)"""
    grid = r0 + dr * np.arange(len(e))
    return lambda r: (np.interp(r, grid, e), np.interp(r, grid, f))


def bond_terms(pos, box, bonds, lam, fun):
    """bonds: 0-based index pairs; lam: one value per bond; fun(r) -> (u, f(r)), or a list of such functions, one per bond.
    Returns the forces sum over bonds of lam F and the energy sum of lam U."""
    F = np.zeros_like(pos)
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    if len(b) == 0:
        return F, 0.0
    box = np.asarray(box, dtype=np.float64)
    d = pos[b[:, 0]] - pos[b[:, 1]]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(1))
    if callable(fun):
        u, fv = fun(r)
    else:
        uf = [fk(rk) for fk, rk in zip(fun, r)]
        u, fv = np.array([x[0] for x in uf]), np.array([x[1] for x in uf])
    lam = np.asarray(lam, dtype=np.float64)
    fvec = (lam * fv / r)[:, None] * d
    np.add.at(F, b[:, 0], fvec); np.add.at(F, b[:, 1], -fvec)
    return F, float(np.sum(lam * u))
