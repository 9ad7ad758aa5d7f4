"""The static structure factor of include/chem_mi355.h ("static structure factor") restated in numpy, evaluated in np.longdouble from
positions, types and box: the reference tests/test_gpu_sq.py compares the device sums with, and the closed forms of
tests/test_sq_ref.py.  The enumeration of the wave vectors is written out here a second time (a triple loop), not imported."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
TWO_PI = 2 * np.arctan2(LD(0), LD(-1))      # 2 pi in long double


def vectors(nmax):
    """The kept integer triples in index order: lexicographic in (nx, ny, nz) over the canonical half."""
    out = []
    for nx in range(0, nmax + 1):
        for ny in range(-nmax, nmax + 1):
            for nz in range(-nmax, nmax + 1):
                if nx > 0 or (nx == 0 and ny > 0) or (nx == 0 and ny == 0 and nz > 0):
                    out.append((nx, ny, nz))
    return np.array(out, dtype=np.int64)


def in_set(t, types):
    types = np.asarray(types)
    return np.ones(len(types), bool) if t < 0 else types == t


def bound(nmax, na, nb, frames=1):
    """|sums_dev - sums_ref| <= 128 (nmax + 2) eps N_A N_B per frame (the issue's derivation: 2 eps relative per axis in x * invL,
    i.e. 2 pi 3 nmax 2 eps in theta; 6 (nmax + 2) eps for sincos, recurrence and products; |rho_A| <= N_A)."""
    return frames * 128.0 * (nmax + 2) * EPS * float(na) * float(nb)


def rho(box, pos, n, dtype=LD, chunk=512):
    """rho(n_k) = sum_j exp(-i theta_j(n_k)) as (re, im) arrays of dtype, theta = 2 pi n . (x / L)."""
    pos = np.asarray(pos, dtype=np.float64).astype(dtype).reshape(-1, 3)
    f = pos / np.asarray(box, dtype=np.float64).astype(dtype)
    two_pi = TWO_PI if dtype is LD else dtype(2.0 * np.pi)
    re, im = np.zeros(len(n), dtype=dtype), np.zeros(len(n), dtype=dtype)
    for k0 in range(0, len(n), chunk):
        # n . f is reduced by its integer part first: the phase is periodic, and the argument of cos / sin stays small
        u = n[k0:k0 + chunk].astype(dtype) @ f.T                       # (chunk, N)
        th = two_pi * (u - np.floor(u)) if dtype is LD else two_pi * u
        re[k0:k0 + chunk] = np.cos(th).sum(axis=1)
        im[k0:k0 + chunk] = -np.sin(th).sum(axis=1)
    return re, im


def sums(box, pos, types, nmax, sel, dtype=LD, n=None):
    """One frame: sums[s][k] = Re(rho_A conj rho_B) as float64 (computed in dtype), na[s], nb[s]."""
    n = vectors(nmax) if n is None else n
    types = np.asarray(types)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    cache = {}

    def r(t):
        if t not in cache:
            cache[t] = rho(box, pos[in_set(t, types)], n, dtype)
        return cache[t]
    out = np.zeros((len(sel), len(n)), dtype=dtype)
    na, nb = np.zeros(len(sel)), np.zeros(len(sel))
    for s, (t1, t2) in enumerate(sel):
        (ar, ai), (br, bi) = r(t1), r(t2)
        out[s] = ar * br + ai * bi
        na[s], nb[s] = in_set(t1, types).sum(), in_set(t2, types).sum()
    return out, na, nb


class Accumulator:
    """Frames summed as chem_sq_* sums them; `sums` stays in long double."""

    def __init__(self, nmax, sel=((-1, -1),)):
        self.nmax, self.sel, self.n = nmax, [tuple(s) for s in sel], vectors(nmax)
        self.sums = np.zeros((len(self.sel), len(self.n)), dtype=LD)
        self.na, self.nb, self.box_sum, self.frames = np.zeros(len(self.sel)), np.zeros(len(self.sel)), np.zeros(3), 0
        self.tol = np.zeros(len(self.sel))

    def add(self, box, pos, types):
        s, na, nb = sums(box, pos, types, self.nmax, self.sel, n=self.n)
        self.sums += s
        self.na += na
        self.nb += nb
        self.box_sum = self.box_sum + np.asarray(box, dtype=np.float64)
        self.frames += 1
        self.tol += np.array([bound(self.nmax, a, b) for a, b in zip(na, nb)])
        return self
