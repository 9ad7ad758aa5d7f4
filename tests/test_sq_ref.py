"""tests/sq_ref.py against closed forms, and the derived device bound against what plain fp64 does: the bound
128 (nmax + 2) eps N_A N_B holds for a straightforward fp64 numpy evaluation on every fixture here, and a wrong evaluation -- one
particle dropped, the sign of n_z swapped -- leaves it.  Nothing here needs a GPU."""
import numpy as np
import pytest

import sq_ref as SR
from chemlab_amd import engine as E

ANY = [(-1, -1)]
SEL4 = [(-1, -1), (0, 0), (0, 1), (1, 1)]


def lattice(m=4, L=8.0):
    """m^3 sites of a simple-cubic lattice in a cubic box, shifted by 1/8 of the box: every coordinate an exact binary fraction."""
    g = np.arange(m) * (L / m) + L / 8.0
    return np.array([L, L, L]), np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def melt(n=500, seed=3):
    rng = np.random.default_rng(seed)
    box = np.array([9.0, 11.5, 7.25])
    return box, rng.uniform(0, 1, (n, 3)) * box, (np.arange(n) % 3 == 0).astype(np.int32)


FIXTURES = {
    "one": lambda: (np.array([5.0, 6.0, 7.0]), np.array([[1.3, 2.9, 6.6]]), np.zeros(1, np.int32), 5),
    "two": lambda: (np.array([5.0, 6.0, 7.0]), np.array([[1.3, 2.9, 6.1], [4.4, 0.2, 3.1]]), np.array([0, 1], np.int32), 5),
    "lattice": lambda: lattice() + (np.zeros(64, np.int32), 5),
    "melt": lambda: melt() + (4,),
    "melt16": lambda: melt(120, 5) + (16,),
}


def test_enumeration_is_the_engines():
    for nmax in (1, 2, 3, 8, 16):
        n = SR.vectors(nmax)
        assert len(n) == ((2 * nmax + 1) ** 3 - 1) // 2 == E.sq_nvec(nmax) and np.array_equal(n, E.sq_vectors(nmax))
    assert [E.sq_nvec(k) for k in (1, 3, 8, 16)] == [13, 171, 2456, 17968]
    assert SR.vectors(1).tolist()[:5] == [[0, 0, 1], [0, 1, -1], [0, 1, 0], [0, 1, 1], [1, -1, -1]]


def test_one_particle_gives_one_everywhere():
    box, pos, types, nmax = FIXTURES["one"]()
    s, na, nb = SR.sums(box, pos, types, nmax, ANY)
    assert np.abs(s[0] - 1).max() < 1e-18 and na[0] == nb[0] == 1


def test_two_particles_give_one_plus_cos_q_d():
    box, pos, types, nmax = FIXTURES["two"]()
    s, _, _ = SR.sums(box, pos, types, nmax, ANY)
    d = (pos[0].astype(SR.LD) - pos[1].astype(SR.LD)) / box.astype(SR.LD)
    want = 2 + 2 * np.cos(SR.TWO_PI * (SR.vectors(nmax).astype(SR.LD) @ d))      # |rho|^2 = N + 2 cos(q . d); per particle 1 + cos
    assert np.abs(s[0] - want).max() < 1e-16                                        # (long double: eps = 1e-19, phases up to 2 pi 15)
    assert np.abs(s[0] / 2 - (1 + np.cos(SR.TWO_PI * (SR.vectors(nmax).astype(SR.LD) @ d)))).max() < 1e-16


def test_lattice_bragg_peaks_and_nothing_else():
    box, pos, types, nmax = FIXTURES["lattice"]()
    s, na, nb = SR.sums(box, pos, types, nmax, ANY)
    n = SR.vectors(nmax)
    bragg = (n % 4 == 0).all(axis=1)
    N = len(pos)
    tol = SR.bound(nmax, N, N)
    assert bragg.sum() == 13 and tol < 1e-8                                         # n in {-4, 0, 4}^3, canonical half
    assert np.abs(s[0][bragg] - N * N).max() <= tol and np.abs(s[0][~bragg]).max() <= tol


@pytest.mark.parametrize("name", list(FIXTURES))
def test_minus_n_gives_the_same_sum(name):
    box, pos, types, nmax = FIXTURES[name]()
    n = SR.vectors(nmax)
    a, na, nb = SR.sums(box, pos, types, nmax, SEL4, n=n)
    b, _, _ = SR.sums(box, pos, types, nmax, SEL4, n=-n)
    for s in range(4):
        assert np.abs(a[s] - b[s]).max() <= max(SR.bound(nmax, na[s], nb[s]), 1e-300)


def test_partials_add_up_to_the_total():
    box, pos, types, nmax = FIXTURES["melt"]()
    s, na, nb = SR.sums(box, pos, types, nmax, SEL4)
    assert na[0] == len(pos) and na[1] + na[3] == len(pos) and (na[2], nb[2]) == (na[1], na[3])
    # ordered class pairs: (0,0) + (0,1) + (1,0) + (1,1), and Re(rho_0 conj rho_1) = Re(rho_1 conj rho_0)
    assert np.abs(s[1] + 2 * s[2] + s[3] - s[0]).max() <= SR.bound(nmax, na[0], nb[0])


def test_translation_leaves_every_sum():
    box, pos, types, nmax = FIXTURES["melt"]()
    a, na, nb = SR.sums(box, pos, types, nmax, SEL4)
    b, _, _ = SR.sums(box, (pos + np.array([0.731, -2.2, 5.05])) % box, types, nmax, SEL4)
    for s in range(4):
        # the shifted coordinates are other doubles: each carries half an ulp of its own, which the bound's 2 eps per axis covers
        assert np.abs(a[s] - b[s]).max() <= SR.bound(nmax, na[s], nb[s])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_plain_fp64_stays_inside_the_bound_and_wrong_answers_leave_it(name):
    box, pos, types, nmax = FIXTURES[name]()
    sel = SEL4 if len(pos) > 2 and types.any() else ANY
    ref, na, nb = SR.sums(box, pos, types, nmax, sel)
    f64, _, _ = SR.sums(box, pos, types, nmax, sel, dtype=np.float64)
    n = SR.vectors(nmax)
    for s in range(len(sel)):
        tol = SR.bound(nmax, na[s], nb[s])
        err = np.abs(f64[s].astype(SR.LD) - ref[s]).max()
        assert err <= tol, (name, s, float(err), tol)
    print("%s: fp64 error %.3g of a bound of %.3g" % (name, float(np.abs(f64[0].astype(SR.LD) - ref[0]).max()), SR.bound(nmax, na[0], nb[0])))
    if len(pos) < 2:
        return
    tol = SR.bound(nmax, na[0], nb[0])
    dropped, _, _ = SR.sums(box, pos[1:], types[1:], nmax, sel[:1])
    assert np.abs(dropped[0] - ref[0]).max() > 1000 * tol
    flipped, _, _ = SR.sums(box, pos, types, nmax, sel[:1], n=n * np.array([1, 1, -1]))
    if name != "lattice":                                                           # (the lattice is its own mirror image)
        assert np.abs(flipped[0] - ref[0]).max() > 1000 * tol


def test_sq_result_divides_and_averages_over_shells():
    n = E.sq_vectors(1)
    sums = np.stack([np.arange(13, dtype=np.float64) + 1, np.zeros(13)])
    r = E.sq_result(1, sums, 2, [8.0, 0.0], [2.0, 6.0], [8.0, 8.0, 16.0])
    assert np.array_equal(r["box"], [4.0, 4.0, 8.0]) and r["frames"] == 2 and r["nvec"] == 13 and np.array_equal(r["n"], n)
    assert np.allclose(r["S"][0], sums[0] / 4.0, rtol=1e-15) and not r["S"][1].any()
    q = 2 * np.pi * np.sqrt(((n / np.array([4.0, 4.0, 8.0])) ** 2).sum(axis=1))
    assert np.allclose(r["q"], q, rtol=1e-15)
    assert r["shell_count"].sum() == 13 and len(r["shell_q"]) == len(r["shell_count"]) == r["shell_S"].shape[1]
    k0 = int(np.argmin(r["shell_q"]))                                               # the first shell: n = (0, 0, 1) alone, |q| = 2 pi / 8
    assert r["shell_count"][k0] == 1 and np.isclose(r["shell_q"][k0], 2 * np.pi / 8) and np.isclose(r["shell_S"][0, k0], 0.25)
    z = E.sq_result(1, np.zeros((1, 13)), 0, [0.0], [0.0], [0.0, 0.0, 0.0])
    assert z["frames"] == 0 and not z["S"].any() and z["shell_S"].shape == (1, 0)
