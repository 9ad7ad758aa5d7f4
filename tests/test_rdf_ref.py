"""tests/rdf_ref.py, the numpy restatement of the g(r) rule set, checked on the CPU against cases with known answers."""
import numpy as np

import rdf_ref as RR


def _lattice(k, a):
    g = np.arange(k)
    cx, cy, cz = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 1).astype(np.float64) * a


def lattice_case(k=6, a=1.0, nbins=64, r_max=2.5):
    """A simple-cubic lattice of k^3 sites, spacing a (a power of two times an integer: every d2 is exact)."""
    return dict(box=[k * a] * 3, pos=_lattice(k, a) + 0.25 * a, types=np.zeros(k ** 3, np.int64), nbins=nbins, r_max=r_max * a)


def test_simple_cubic_shells_land_in_their_bins():
    c = lattice_case()
    acc = RR.Accumulator(c["r_max"], c["nbins"]).add(c["box"], c["pos"], c["types"])
    n = len(c["pos"])
    want = np.zeros(c["nbins"], np.uint64)
    e2 = RR.edges2(c["r_max"], c["nbins"])
    for d2, per_site in ((1.0, 6), (2.0, 12), (3.0, 8), (4.0, 6), (5.0, 24), (6.0, 24)):
        k = int(RR.bin_of(np.array([d2]), e2)[0])
        assert k >= 0 and e2[k] <= d2 < e2[k + 1]
        want[k] += n * per_site // 2
    assert np.array_equal(acc.counts[0, 0], want)
    assert acc.frames == 1 and acc.pairs == [n * (n - 1) // 2]
    assert acc.density[0] == (n * (n - 1) // 2) / 216.0


def test_two_particles_across_face_edge_and_corner():
    L = np.array([8.0, 8.0, 8.0])
    for other, d2 in (([7.5, 0.25, 0.25], 0.5625), ([7.5, 7.75, 0.25], 0.5625 + 0.25), ([7.5, 7.75, 7.5], 0.5625 + 0.25 + 0.5625)):
        acc = RR.Accumulator(2.0, 32).add(L, np.array([[0.25, 0.25, 0.25], other]), [0, 0])
        k = int(RR.bin_of(np.array([d2]), acc.e2)[0])
        assert acc.counts.sum() == 1 and acc.counts[0, 0, k] == 1, (other, k)


def test_a_pair_on_an_edge_goes_up_and_one_at_r_max_is_dropped():
    # nbins / r_max = 16: the edges are multiples of 2^-4, the coordinates multiples of 2^-10, every product exact
    r_max, nbins, L = 2.0, 32, np.array([16.0, 16.0, 16.0])
    e = RR.edges(r_max, nbins)
    for k in (1, 7, 31):
        x = np.array([[1.0, 1.0, 1.0], [1.0 + e[k], 1.0, 1.0]])
        acc = RR.Accumulator(r_max, nbins).add(L, x, [0, 0])
        assert acc.counts[0, 0, k] == 1 and acc.counts.sum() == 1, k
        x[1, 0] -= 2.0 ** -10
        acc = RR.Accumulator(r_max, nbins).add(L, x, [0, 0])
        assert acc.counts[0, 0, k - 1] == 1, k
    x = np.array([[1.0, 1.0, 1.0], [1.0 + e[nbins], 1.0, 1.0]])
    acc = RR.Accumulator(r_max, nbins).add(L, x, [0, 0])
    assert acc.counts.sum() == 0 and acc.frames == 1 and acc.pairs == [1]
    x[1, 0] -= 2.0 ** -10
    assert RR.Accumulator(r_max, nbins).add(L, x, [0, 0]).counts[0, 0, nbins - 1] == 1


def test_wildcards_sum_to_the_total_and_split_parts_add_up():
    rng = np.random.default_rng(5)
    n, L = 300, np.array([6.0, 7.0, 8.0])
    x = rng.uniform(0, 1, (n, 3)) * L
    types = rng.integers(0, 3, n)
    mol = rng.integers(0, 40, n)
    sel = [(-1, -1), (0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (-1, 1)]
    acc = RR.Accumulator(2.5, 50, sel, split=True).add(L, x, types, mol)
    whole = RR.Accumulator(2.5, 50, sel).add(L, x, types)
    assert np.array_equal(acc.counts.sum(1), whole.counts[:, 0])
    assert np.array_equal(whole.counts[0, 0], whole.counts[1:7, 0].sum(0))            # the six type pairs partition the total
    assert np.array_equal(whole.counts[7, 0], whole.counts[2, 0] + whole.counts[3, 0] + whole.counts[5, 0])      # (-1, 1) = (0,1) + (1,1) + (1,2)
    assert np.array_equal(RR.Accumulator(2.5, 50, [(1, 0)]).add(L, x, types).counts[0], whole.counts[2])           # unordered
    # brute force, pair by pair
    want = np.zeros((50,), np.uint64)
    for i in range(n):
        for j in range(i + 1, n):
            if mol[i] == mol[j]:
                d = x[i] - x[j]
                d = d - L * np.rint(d * (1.0 / L))
                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                k = int(RR.bin_of(np.array([d2]), acc.e2)[0])
                if k >= 0:
                    want[k] += 1
    assert np.array_equal(acc.counts[0, 0], want)


def test_normalisers_for_equal_and_unequal_types():
    types = [0] * 5 + [1] * 3 + [4] * 2
    assert RR.norm_pairs((0, 0), types) == 10 and RR.norm_pairs((0, 1), types) == 15 and RR.norm_pairs((1, 0), types) == 15
    assert RR.norm_pairs((-1, -1), types) == 45 and RR.norm_pairs((-1, 4), types) == 5 * 2 + 3 * 2 + 1
    assert RR.norm_pairs((2, 2), types) == 0 and RR.norm_pairs((4, 4), types) == 1
    acc = RR.Accumulator(1.0, 4, [(0, 1)])
    acc.add([4.0, 4.0, 4.0], np.zeros((10, 3)), types).add([4.0, 4.0, 5.0], np.zeros((10, 3)), types)
    assert acc.frames == 2 and acc.pairs == [30] and acc.density[0] == 15 / 64.0 + 15 / 80.0
