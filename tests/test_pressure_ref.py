"""tests/pressure_ref.py against itself: W as sum r.F against W as -dU/dlambda, the limiting cases, the NPT stepper (CPU)."""
import numpy as np
import pytest

import aged_ref
import bonded_ref
import helpers as H
import pressure_ref as PR


def _lj_melt(n=216, rho=0.7, seed=5):
    from chemlab_amd import workloads as W
    rng = np.random.default_rng(seed)
    pos, L, _ = W._lattice(n, rho)
    pos = pos + rng.uniform(-0.08, 0.08, pos.shape)
    types = rng.integers(0, 2, n).astype(np.int32)
    lj = [(0, 0, 1.0, 1.0, 2.5), (0, 1, 0.8, 1.1, 2.5), (1, 1, 1.2, 0.9, 2.2)]
    return dict(n=n, box=np.array([L] * 3), rc=2.5, skin=0.3, ids=np.arange(1, n + 1), types=types, pos=pos, mass=rng.uniform(0.8, 1.5, n),
                vel=rng.normal(0, 1, (n, 3)), lj=lj, tables=[])


def test_nonbonded_rf_is_the_sum_exact_pairs_forms():
    spec = _lj_melt()
    w, a = PR.nonbonded_rf(spec, spec["pos"])
    ref = aged_ref.exact_pairs(spec, spec["pos"])
    assert abs(w - ref["virial_nb"]) <= 1e-12 * a
    assert abs(w - H.pair_reference(spec)[3]) <= 1e-12 * a


def test_nonbonded_rf_against_scaling_derivative():
    spec = _lj_melt()
    w, a = PR.nonbonded_rf(spec, spec["pos"])
    assert abs(w - PR.lj_scaling(spec, spec["pos"])) <= 1e-11 * a


@pytest.mark.parametrize("box_name", ["tiles", "cells"])
def test_lists_rf_against_scaling_derivative(box_name):
    if box_name not in bonded_ref.BOXES:
        box_name = sorted(bonded_ref.BOXES)[0]
    spec = bonded_ref.zoo(box_name)
    rf = PR.lists_rf(spec["pos"], spec["box"], spec["types"], spec["lists"])
    sc = PR.lists_scaling(spec["pos"], spec["box"], spec["types"], spec["lists"])
    seen = set()
    for lst, (w, a), s in zip(spec["lists"], rf, sc):
        seen.add(lst["arity"])
        if lst["arity"] == 2:
            assert a > 0, lst["name"]
            assert abs(w - s) <= 1e-11 * a, (lst["name"], w, s)
        else:      # angles and dihedrals: W = 0 to rounding, on the scale of the energy's own gradient terms
            e = abs(bonded_ref.reference(spec["pos"], spec["box"], spec["types"], [lst])["force"]).sum() * float(np.max(spec["box"]))
            assert w == 0.0 and abs(s) <= 1e-11 * max(e, 1.0), (lst["name"], s)
    assert seen == {2, 3, 4}


def test_hybrid_weight_and_coulomb_pairs():
    spec = bonded_ref.zoo(sorted(bonded_ref.BOXES)[0])
    li = bonded_ref.pick_lists(spec, kinds=("HARMONIC",))[0]
    base = spec["lists"][li]
    lam = dict(base, lam=0.37)
    (w1, a1), = PR.lists_rf(spec["pos"], spec["box"], spec["types"], [base])
    (w2, a2), = PR.lists_rf(spec["pos"], spec["box"], spec["types"], [lam])
    assert abs(w2 - 0.37 * w1) <= 1e-13 * a1 and abs(w2 - PR.lists_scaling(spec["pos"], spec["box"], spec["types"], [lam])[0]) <= 1e-11 * a2
    q = np.random.default_rng(3).uniform(-1, 1, spec["n"])
    coul = dict(name="c14", kind="COULOMB_BOND", arity=2, params=[138.9, 1.2], ids=base["ids"])
    (w, a), = PR.lists_rf(spec["pos"], spec["box"], spec["types"], [coul], q)
    assert a > 0 and abs(w - PR.lists_scaling(spec["pos"], spec["box"], spec["types"], [coul], q)[0]) <= 1e-11 * a
    # U = k qq / r: r.F = U for every pair inside the cutoff
    idx = np.asarray(base["ids"]).reshape(-1, 2) - 1
    d = spec["pos"][idx[:, 0]] - spec["pos"][idx[:, 1]]
    d -= spec["box"] * np.rint(d / spec["box"])
    r = np.sqrt((d * d).sum(1))
    u = np.where(r <= 1.2, 138.9 * q[idx[:, 0]] * q[idx[:, 1]] / r, 0.0)
    assert abs(w - u.sum()) <= 1e-12 * a


def test_ideal_gas_pressure_is_exact():
    spec = _lj_melt()
    spec = dict(spec, lj=[], tables=[])
    p = PR.pressure(spec, spec["pos"], spec["vel"])
    assert p["virial"] == 0.0
    assert p["pressure"] == PR.mv2(spec["mass"], spec["vel"]) / (3.0 * float(np.prod(spec["box"])))


def test_npt_stepper_follows_the_rule_and_relaxes_towards_p0():
    spec = _lj_melt(n=125, rho=0.6)
    fn = PR.exact_force_fn(spec)
    x, v, L = spec["pos"].copy(), 0.3 * spec["vel"], spec["box"].copy()
    f, w = fn(x, L)
    p_start = PR.pressure(spec, x, v)["pressure"]
    p0, dt, tau = p_start + 1.0, 0.002, 0.2
    ratios = L / L[0]
    for s in range(20):
        L_old, x_old = L, x
        x, v, f_new, L, p = PR.npt_step(spec, x, v, f, L, fn, dt, tau, p0)
        mu = L[0] / L_old[0]
        assert abs(mu ** 3 - PR.mu3(dt, tau, p0, p)) <= 4e-16 * 3
        assert np.array_equal(L / L[0], ratios)
        # the forces handed on are those from before the scaling
        # (x / mu is x before the scaling to one rounding: the forces agree to the rounding of the positions, and differ from
        #  the forces at the scaled positions by |mu - 1| times a force gradient, eight orders more)
        f_chk, _ = fn(x / mu, L_old)
        assert np.abs(f_chk - f_new).max() <= 1e-10 * np.abs(f_new).max()
        f = f_new
    assert L[0] < spec["box"][0]            # P < P0: the box shrinks
    assert PR.pressure(spec, x, v, box=L)["pressure"] > p_start - 0.5


def test_mu3_refusal():
    spec = _lj_melt(n=64, rho=0.5)
    fn = PR.exact_force_fn(spec)
    f, _ = fn(spec["pos"], spec["box"])
    with pytest.raises(ArithmeticError, match="Berendsen barostat"):
        PR.npt_step(spec, spec["pos"], spec["vel"], f, spec["box"], fn, 0.002, 1e-9, 1e3)


def test_guard_of_the_lists_under_scaling_test():
    """The cold lattice of tests/test_gpu_barostat.py under the reference stepper: pairs that were outside rc + skin at the first
    build come inside rc during the compression, and the first of them does so long BEFORE the displacement relative to the
    scaled lattice (all that the displacement criterion sees without the charge) reaches skin / 2: an engine that forgets to
    charge the scalings to its lists computes forces without them.  (Under expansion pairs only leave: no such pair.)"""
    from scipy.spatial import cKDTree
    spec = PR.cold_lattice("shrink")
    p0, tau = PR.cold_coupling(spec, "shrink")
    fn = PR.exact_force_fn(spec)
    x, v, L = spec["pos"].copy(), spec["vel"].copy(), spec["box"].copy()
    f, _ = fn(x, L)
    rl = PR.COLD_RC + PR.COLD_SKIN
    target, s, s_pair, s_thermal, s_cells, far = 0.93 * L[0], 0, None, None, None, 0
    while L[0] > target and s < 200:
        x, v, f, L, p = PR.npt_step(spec, x, v, f, L, fn, spec["dt"], tau, p0)
        s += 1
        moved = float(np.sqrt(((x / (L[0] / spec["box"][0]) - spec["pos"]) ** 2).sum(1)).max())
        if s_thermal is None and moved > 0.5 * PR.COLD_SKIN:
            s_thermal = s
        ij = cKDTree(x - np.floor(x / L) * L, boxsize=L).query_pairs(PR.COLD_RC, output_type="ndarray")
        d = spec["pos"][ij[:, 0]] - spec["pos"][ij[:, 1]]
        d -= spec["box"] * np.rint(d / spec["box"])
        far = int((np.sqrt((d * d).sum(1)) > rl).sum())
        if s_pair is None and far:
            s_pair = s
        if s_cells is None and np.floor(L[0] / rl) < 5:
            s_cells = s
    print("first pair from outside the list radius inside rc at step %s; displacement alone reaches skin / 2 at step %s; %d steps, %d such pairs at the end" % (s_pair, s_thermal, s, far))
    print("the cell count changes at step %s" % s_cells)
    assert 40 < s < 200 and L[0] <= target
    assert s_pair is not None and (s_thermal is None or s_pair + 10 < s_thermal) and s_pair + 10 < s_cells      # ... and before the re-plan builds lists anyway
    assert far > 1000, far
    assert int(np.floor(spec["box"][0] / rl)) == 5 and int(np.floor(L[0] / rl)) == 4
