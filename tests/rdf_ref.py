"""Radial distribution functions: a plain numpy O(N^2) restatement of the rule set of include/chem_mi355.h ("radial
distribution functions") -- edges, bins, selectors, molecule split, normalisers.  No cells, no list, no oracle, no engine.

  pairs       every unordered pair of distinct particles, once
  distance    d2 = react_ref.dist2: fp64 minimum image, three products, two sums, nothing fused
  bins        dr = r_max / nbins, e[k] = k * dr, e2[k] = e[k] * e[k]; bin k holds e2[k] <= d2 < e2[k + 1]; d2 >= e2[nbins] is dropped
  selectors   unordered (t1, t2), -1 = any type; a pair is counted in every selector it matches
  split       part 0: mol[i] == mol[j], part 1: the rest
  normaliser  M = unordered pairs of distinct particles whose types match, from the type counts
  frame       counts[sel][part][k] += ..., frames += 1, pairs[sel] += M, density[sel] += M / (Lx Ly Lz) in frame order"""
import numpy as np

from react_ref import dist2


def edges(r_max, nbins):
    dr = np.float64(r_max) / np.float64(nbins)
    return np.arange(nbins + 1, dtype=np.float64) * dr


def edges2(r_max, nbins):
    e = edges(r_max, nbins)
    return e * e


def bin_of(d2, e2):
    """Bin of every d2 (array): k with e2[k] <= d2 < e2[k + 1], -1 where d2 >= e2[-1]."""
    d2 = np.asarray(d2, dtype=np.float64)
    k = np.searchsorted(e2, d2, side="right") - 1
    return np.where(d2 < e2[-1], k, -1)


def matches(sel, a, b):
    """Whether the unordered selector (t1, t2) counts pairs of types a, b (arrays)."""
    t1, t2 = sel
    fwd = ((t1 < 0) | (a == t1)) & ((t2 < 0) | (b == t2))
    rev = ((t1 < 0) | (b == t1)) & ((t2 < 0) | (a == t2))
    return fwd | rev


def norm_pairs(sel, types, ntypes=16):
    """M of a selector from the vector of type counts."""
    c = np.bincount(np.asarray(types, dtype=np.int64), minlength=ntypes)
    m = 0
    for u in range(len(c)):
        for v in range(u, len(c)):
            if matches(sel, np.int64(u), np.int64(v)):
                m += int(c[u]) * (int(c[u]) - 1) // 2 if u == v else int(c[u]) * int(c[v])
    return m


class Accumulator:
    """What chem_rdf_get returns after the frames given to add()."""

    def __init__(self, r_max, nbins, selectors=((-1, -1),), split=False):
        self.r_max, self.nbins, self.sel, self.split = float(r_max), int(nbins), [tuple(int(t) for t in s) for s in selectors], bool(split)
        self.e2 = edges2(r_max, nbins)
        self.reset()

    def reset(self):
        self.counts = np.zeros((len(self.sel), 2 if self.split else 1, self.nbins), dtype=np.uint64)
        self.frames = 0
        self.pairs = [0] * len(self.sel)
        self.density = [np.float64(0.0)] * len(self.sel)

    def add(self, box, pos, types, mol=None):
        L = np.asarray(box, dtype=np.float64)
        x = np.asarray(pos, dtype=np.float64)
        types = np.asarray(types, dtype=np.int64)
        mol = np.zeros(len(x), np.int64) if mol is None else np.asarray(mol, dtype=np.int64)
        n = len(x)
        for i in range(n - 1):
            d2 = dist2(L, x[i], x[i + 1:])
            near = np.nonzero(d2 < self.e2[-1])[0]
            if not len(near):
                continue
            k = bin_of(d2[near], self.e2)
            j = near + i + 1
            part = (mol[j] != mol[i]).astype(np.int64) if self.split else np.zeros(len(j), np.int64)
            for s, sel in enumerate(self.sel):
                m = matches(sel, types[i], types[j])
                for p in range(self.counts.shape[1]):
                    self.counts[s, p] += np.bincount(k[m & (part == p)], minlength=self.nbins).astype(np.uint64)
        V = L[0] * L[1] * L[2]
        self.frames += 1
        for s, sel in enumerate(self.sel):
            M = norm_pairs(sel, types)
            self.pairs[s] += M
            self.density[s] = self.density[s] + np.float64(M) / V
        return self


def ulps(a, b):
    """Distance of two finite doubles of equal sign in units in the last place."""
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(ia) - int(ib))
