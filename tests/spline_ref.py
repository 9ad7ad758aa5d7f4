"""numpy restatement of the spline kinds of the tabulated potentials (rule set: include/chem_mi355.h, chem_nb_table_interp)
and brute-force references built on it: all-pairs non-bonded sums and bonded terms evaluated from the tables.  Shared by
tests/test_host_tables.py and tests/test_gpu_spline_tables.py.  Imports nothing from the product."""
import numpy as np


# ---- the rule set ----------------------------------------------------------------------------------------------------------

def akima_coeffs(y):
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    m = np.empty(n + 3)                       # m[k + 2] = d_k, k = -2 .. n
    m[2:n + 1] = np.diff(y)
    m[1] = 2.0 * m[2] - m[3]; m[0] = 2.0 * m[1] - m[2]
    m[n + 1] = 2.0 * m[n] - m[n - 1]; m[n + 2] = 2.0 * m[n + 1] - m[n]
    w1 = np.abs(m[3:] - m[2:-1])              # |d_{k+1} - d_k|
    w2 = np.abs(m[1:-2] - m[:-3])             # |d_{k-1} - d_{k-2}|
    s = w1 + w2
    tie = s <= 1e-9 * s.max()
    t = np.where(tie, 0.5 * (m[1:-2] + m[2:-1]), (w1 * m[1:-2] + w2 * m[2:-1]) / np.where(tie, 1.0, s))
    d = m[2:n + 1]
    return np.stack([y[:-1], t[:-1], 3.0 * d - 2.0 * t[:-1] - t[1:], t[:-1] + t[1:] - 2.0 * d], 1)


def cubic_coeffs(y):
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    A = np.zeros((n, n))
    rhs = np.zeros(n)
    A[0, 0] = A[n - 1, n - 1] = 1.0           # natural ends: M_0 = M_{n-1} = 0
    for k in range(1, n - 1):
        A[k, k - 1:k + 2] = (1.0, 4.0, 1.0)
        rhs[k] = 6.0 * (y[k + 1] - 2.0 * y[k] + y[k - 1])
    M = np.linalg.solve(A, rhs)
    d = np.diff(y)
    return np.stack([y[:-1], d - (2.0 * M[:-1] + M[1:]) / 6.0, 0.5 * M[:-1], (M[1:] - M[:-1]) / 6.0], 1)


def linear_coeffs(y):
    y = np.asarray(y, dtype=np.float64)
    z = np.zeros(len(y) - 1)
    return np.stack([y[:-1], np.diff(y), z, z], 1)


def coeffs(y, itype):
    return {1: linear_coeffs, 2: akima_coeffs, 3: cubic_coeffs}[itype](y)


def evaluate(c, r0, dr, x, deriv=0):
    """Piecewise cubic c (nrow - 1 rows of c0..c3) at x: t clamped to [0, nrow - 1], k = min(int(t), nrow - 2), Horner.
    deriv = 1, 2: derivatives with respect to w, inside the interval of k."""
    nrow = len(c) + 1
    t = np.clip((np.asarray(x, dtype=np.float64) - r0) / dr, 0.0, nrow - 1.0)
    k = np.minimum(t.astype(np.int64), nrow - 2)
    w = t - k
    c0, c1, c2, c3 = c[k, 0], c[k, 1], c[k, 2], c[k, 3]
    if deriv == 1:
        return c1 + w * (2.0 * c2 + w * 3.0 * c3)
    if deriv == 2:
        return 2.0 * c2 + 6.0 * w * c3
    return c0 + w * (c1 + w * (c2 + w * c3))


class Table:
    """One tabulated potential: e and f columns interpolated independently with kind `itype`."""

    def __init__(self, r0, dr, e, f, itype):
        self.r0, self.dr, self.e, self.f, self.itype = float(r0), float(dr), np.asarray(e, np.float64), np.asarray(f, np.float64), itype
        self.ce, self.cf = coeffs(self.e, itype), coeffs(self.f, itype)

    def __call__(self, x):
        return evaluate(self.ce, self.r0, self.dr, x), evaluate(self.cf, self.r0, self.dr, x)


# ---- brute-force non-bonded sums ---------------------------------------------------------------------------------------

def lj(eps, sig, rc, shift_auto=True):
    s6 = (sig * sig / (rc * rc)) ** 3
    return ("lj", eps, sig, rc, -4.0 * eps * (s6 * s6 - s6) if shift_auto else 0.0)


def pair_sums(pos, box, types, matrix, excluded=()):
    """matrix: {(t1, t2) with t1 <= t2: ("lj", eps, sig, rc, shift) | ("tab", Table, rc)}.  All pairs, minimum image;
    `excluded`: index pairs (0-based) left out.  Returns forces, epot_lj, epot_tab."""
    pos, box, types = np.asarray(pos, np.float64), np.asarray(box, np.float64), np.asarray(types)
    n = len(pos)
    F = np.zeros((n, 3))
    e_lj = e_tab = 0.0
    ex = np.zeros((n, n), dtype=bool) if len(excluded) else None
    for a, b in excluded:
        ex[a, b] = ex[b, a] = True
    iu = np.triu_indices(n, 1)
    d = pos[iu[0]] - pos[iu[1]]
    d -= box * np.rint(d / box)
    r2 = (d * d).sum(1)
    ti, tj = np.minimum(types[iu[0]], types[iu[1]]), np.maximum(types[iu[0]], types[iu[1]])
    live = np.ones(len(r2), dtype=bool) if ex is None else ~ex[iu]
    for (t1, t2), prm in matrix.items():
        rc = prm[3] if prm[0] == "lj" else prm[2]
        sel = np.nonzero(live & (ti == t1) & (tj == t2) & (r2 <= rc * rc))[0]
        q = r2[sel]
        if prm[0] == "lj":
            _, eps, sig, _, shift = prm
            s6 = (sig * sig / q) ** 3
            ff = 24.0 * eps * (2.0 * s6 * s6 - s6) / q
            e_lj += (4.0 * eps * (s6 * s6 - s6) + shift).sum()
        else:
            r = np.sqrt(q)
            ev, fv = prm[1](r)
            ff = fv / r
            e_tab += ev.sum()
        fvec = ff[:, None] * d[sel]
        np.add.at(F, iu[0][sel], fvec)
        np.add.at(F, iu[1][sel], -fvec)
    return F, e_lj, e_tab


# ---- bonded terms ------------------------------------------------------------------------------------------------------

def _mi(d, box):
    return d - box * np.rint(d / box)


def bond_terms(pos, box, bonds, fun):
    """bonds: 0-based index pairs; fun(r) -> (u, f(r)) with F_ij = f(r)/r * r_ij.  Returns forces, energy."""
    F = np.zeros_like(pos)
    if len(bonds) == 0:
        return F, 0.0
    b = np.asarray(bonds)
    d = _mi(pos[b[:, 0]] - pos[b[:, 1]], box)
    r = np.sqrt((d * d).sum(1))
    u, fv = fun(r)
    fvec = (fv / r)[:, None] * d
    np.add.at(F, b[:, 0], fvec); np.add.at(F, b[:, 1], -fvec)
    return F, float(np.sum(u))


def angle_terms(pos, box, triples, fun):
    """fun(theta) -> (U, -dU/dtheta), theta at the middle particle."""
    F = np.zeros_like(pos)
    t = np.asarray(triples)
    r1, r2 = _mi(pos[t[:, 0]] - pos[t[:, 1]], box), _mi(pos[t[:, 2]] - pos[t[:, 1]], box)
    n1, n2 = np.sqrt((r1 * r1).sum(1)), np.sqrt((r2 * r2).sum(1))
    c = np.clip((r1 * r2).sum(1) / (n1 * n2), -1.0, 1.0)
    th = np.arccos(c)
    s = np.maximum(np.sqrt(1.0 - c * c), 1e-9)
    u, fv = fun(th)
    a = (-fv / s)[:, None]                    # dU/dtheta / sin(theta)
    fi = a * (r2 / (n1 * n2)[:, None] - r1 * (c / (n1 * n1))[:, None])
    fk = a * (r1 / (n1 * n2)[:, None] - r2 * (c / (n2 * n2))[:, None])
    np.add.at(F, t[:, 0], fi); np.add.at(F, t[:, 2], fk); np.add.at(F, t[:, 1], -(fi + fk))
    return F, float(np.sum(u))


def dihedral_angle(pos, box, quads):
    q = np.asarray(quads)
    b1, b2, b3 = _mi(pos[q[:, 1]] - pos[q[:, 0]], box), _mi(pos[q[:, 2]] - pos[q[:, 1]], box), _mi(pos[q[:, 3]] - pos[q[:, 2]], box)
    m, nn = np.cross(b1, b2), np.cross(b2, b3)
    lb = np.sqrt((b2 * b2).sum(1))
    return np.arctan2(lb * (b1 * nn).sum(1), (m * nn).sum(1)), (b1, b2, b3, m, nn, lb)


def dihedral_terms(pos, box, quads, fun):
    """fun(phi) -> (U, -dU/dphi), phi in [-pi, pi] by the IUPAC sign."""
    F = np.zeros_like(pos)
    q = np.asarray(quads)
    phi, (b1, b2, b3, m, nn, lb) = dihedral_angle(pos, box, quads)
    u, fv = fun(phi)
    dU = -fv
    m2, n2, lb2 = (m * m).sum(1), (nn * nn).sum(1), lb * lb
    g1, g4 = (-lb / m2)[:, None] * m, (lb / n2)[:, None] * nn
    s12, s32 = ((b1 * b2).sum(1) / lb2)[:, None], ((b3 * b2).sum(1) / lb2)[:, None]
    g = [g1, (-1.0 - s12) * g1 + s32 * g4, (-1.0 - s32) * g4 + s12 * g1, g4]
    for k in range(4):
        np.add.at(F, q[:, k], -dU[:, None] * g[k])
    return F, float(np.sum(u))
