"""tests/capped_ref.py (the numpy restatement of chem_nb_cap's rule set that the GPU tests compare with) against answers worked
out by hand: two bodies at r = c/2, c, 1.01 c and 0, a constant force magnitude inside the cap, continuity at the cap radius,
and uncapped pairs left alone."""
import numpy as np
import pytest

import capped_ref as C
import spline_ref as S

BOX = [20.0, 20.0, 20.0]
EPS, SIG, RCUT, CAP = 1.3, 0.9, 2.0, 0.8
LJ = S.lj(EPS, SIG, RCUT)


def lj_u(r):
    s6 = (SIG / r) ** 6
    return 4.0 * EPS * (s6 * s6 - s6) + LJ[4]


def lj_f(r):
    s6 = (SIG / r) ** 6
    return 24.0 * EPS * (2.0 * s6 * s6 - s6) / r


def table(itype=1):
    """U = 3 exp(-2 r), f = 6 exp(-2 r), rows every 0.01 from 0.01"""
    r = 0.01 * np.arange(1, 260)
    return S.Table(0.01, 0.01, 3.0 * np.exp(-2.0 * r), 6.0 * np.exp(-2.0 * r), itype)


def two(r, direction=(1.0, 2.0, -2.0)):
    u = np.asarray(direction) / np.linalg.norm(direction)
    return np.array([[5.0, 5.0, 5.0], np.array([5.0, 5.0, 5.0]) - r * u]), u


def one_pair(matrix, caps, r):
    pos, u = two(r)
    t = C.total(pos, BOX, [0, 0], matrix, caps)
    return t, u


@pytest.mark.parametrize("frac", [0.5, 0.25, 0.9])
def test_lj_inside_the_cap(frac):
    r = frac * CAP
    t, u = one_pair({(0, 0): LJ}, {(0, 0): CAP}, r)
    assert np.allclose(t["F"][0], lj_f(CAP) * u, rtol=1e-13) and np.allclose(t["F"][1], -lj_f(CAP) * u, rtol=1e-13)
    assert np.linalg.norm(t["F"][0]) == pytest.approx(lj_f(CAP), rel=1e-13)      # the magnitude does not depend on r
    assert t["e_lj"] == pytest.approx(lj_u(CAP), rel=1e-13) and t["e_tab"] == 0.0
    assert t["w_nb"] == pytest.approx(lj_f(CAP) * r, rel=1e-13)
    assert bool(t["pairs"]["inside"][0]) and t["pairs"]["re"][0] == CAP


def test_lj_at_and_above_the_cap():
    for r in (CAP, 1.01 * CAP):
        t, u = one_pair({(0, 0): LJ}, {(0, 0): CAP}, r)
        rr = np.sqrt(t["pairs"]["r2"][0])
        assert not t["pairs"]["inside"][0] or rr < CAP          # (r = c as a sum of squares may land a rounding below c)
        assert np.allclose(t["F"][0], lj_f(r) * u, rtol=1e-12)
        assert t["e_lj"] == pytest.approx(lj_u(r), rel=1e-12)
        assert t["w_nb"] == pytest.approx(lj_f(r) * r, rel=1e-12)


def test_zero_distance():
    for matrix, key in (({(0, 0): LJ}, "e_lj"), ({(0, 0): ("tab", table(), RCUT)}, "e_tab")):
        pos = np.array([[5.0, 5.0, 5.0], [5.0, 5.0, 5.0]])
        t = C.total(pos, BOX, [0, 0], matrix, {(0, 0): CAP})
        assert np.array_equal(t["F"], np.zeros((2, 3))) and np.isfinite(t["F"]).all()
        want = lj_u(CAP) if key == "e_lj" else table()(CAP)[0]
        assert t[key] == pytest.approx(float(want), rel=1e-13) and t["w_nb"] == 0.0


@pytest.mark.parametrize("itype", [1, 3])
def test_table_inside_the_cap_has_a_constant_magnitude(itype):
    tb = table(itype)
    uc, fc = (float(v) for v in tb(CAP))
    mags = []
    for r in (0.1, 0.4, 0.79):
        t, u = one_pair({(0, 0): ("tab", tb, RCUT)}, {(0, 0): CAP}, r)
        assert np.allclose(t["F"][0], fc * u, rtol=1e-13)
        assert t["e_tab"] == pytest.approx(uc, rel=1e-13) and t["e_lj"] == 0.0
        assert t["w_nb"] == pytest.approx(fc * r, rel=1e-13)
        mags.append(np.linalg.norm(t["F"][0]))
    assert np.allclose(mags, fc, rtol=1e-13)
    t, u = one_pair({(0, 0): ("tab", tb, RCUT)}, {(0, 0): CAP}, 1.01 * CAP)
    assert np.allclose(t["F"][0], float(tb(1.01 * CAP)[1]) * u, rtol=1e-12)


def test_force_and_energy_are_continuous_at_the_cap():
    for matrix, key in (({(0, 0): LJ}, "e_lj"), ({(0, 0): ("tab", table(), RCUT)}, "e_tab")):
        h = 1e-9
        lo, _ = one_pair(matrix, {(0, 0): CAP}, CAP - h)
        hi, _ = one_pair(matrix, {(0, 0): CAP}, CAP + h)
        assert bool(lo["pairs"]["inside"][0]) and not hi["pairs"]["inside"][0]
        slope = 30.0 * np.abs(hi["F"]).max() / CAP                    # |d(f)/dr| of either potential is far below this
        assert np.abs(lo["F"] - hi["F"]).max() < slope * 2 * h
        assert abs(lo[key] - hi[key]) < np.abs(hi["F"]).max() * 4 * h


def test_uncapped_pairs_are_unchanged():
    rng = np.random.default_rng(5)
    pos = rng.uniform(0.0, 4.0, (60, 3))
    box = [4.0, 4.0, 4.0]
    types = rng.integers(0, 2, 60)
    matrix = {(0, 0): S.lj(1.0, 0.5, 1.3), (0, 1): S.lj(0.8, 0.6, 1.4), (1, 1): ("tab", table(), 1.5)}
    plain_f, plain_lj, plain_tab = S.pair_sums(pos, box, types, matrix)
    none = C.total(pos, box, types, matrix, {})
    assert np.allclose(none["F"], plain_f, rtol=1e-12, atol=1e-12 * np.abs(plain_f).max())
    assert none["e_lj"] == pytest.approx(plain_lj, rel=1e-12) and none["e_tab"] == pytest.approx(plain_tab, rel=1e-12)
    capped = C.total(pos, box, types, matrix, {(0, 0): 0.7})
    p, q = capped["pairs"], none["pairs"]
    assert np.array_equal(p["i"], q["i"]) and np.array_equal(p["j"], q["j"])
    hit = p["inside"].astype(bool)
    assert hit.any() and (types[p["i"][hit]] == 0).all() and (types[p["j"][hit]] == 0).all()
    assert np.array_equal(p["fs"][~hit], q["fs"][~hit]) and np.array_equal(p["u"][~hit], q["u"][~hit])
    fc = C.pot_at(matrix[(0, 0)], 0.7)[1]                             # every pair inside the cap applies the magnitude f(c)
    assert np.allclose(p["fs"][hit] * np.sqrt(p["r2"][hit]), fc, rtol=1e-13) and not np.allclose(q["fs"][hit], p["fs"][hit], rtol=1e-3)
    assert capped["e_tab"] == none["e_tab"]


def test_caps_next_to_resolution_marks():
    """one function gives the reference of a context that has both, on different type pairs"""
    pos = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [1.0, 1.9, 1.0]])
    matrix = {(0, 0): LJ, (0, 2): S.lj(1.0, 0.5, 1.4)}
    t = C.total(pos, BOX, [0, 0, 2], matrix, {(0, 0): CAP}, lam=[1.0, 0.5, 0.5], marked={(0, 2): 0.0})
    p = t["pairs"]
    k00 = np.nonzero(~p["marked"].astype(bool))[0][0]
    assert p["fs"][k00] == pytest.approx(lj_f(CAP) / 0.5, rel=1e-13)
    k02 = np.nonzero(p["marked"].astype(bool) & (p["i"] == 0))[0][0]
    assert p["w"][k02] == 0.5
    with pytest.raises(AssertionError):
        C.total(pos, BOX, [0, 0, 2], matrix, {(0, 0): CAP}, lam=[1.0, 1.0, 1.0], marked={(0, 0): 0.0})
