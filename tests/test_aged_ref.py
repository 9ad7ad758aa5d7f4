"""tests/aged_ref.py on the CPU: the exact pair sum against helpers.pair_reference and against the oracle along a melt, the
restated rebuild rule against the oracle's counter step by step, the guards of every melt that tests/test_gpu_aged_lists.py
runs (enough rebuilds, few pairs on the cutoff, the fp32 tolerance far below what one missed pair changes), and the closing
pairs at the edge of the list radius on the oracle."""
import numpy as np
import pytest

import aged_ref as AR
import helpers as H
import mass_ref
from chemlab_amd import workloads as W
from conftest import rel_err


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.compile_geometry_harness(tmp_path_factory.mktemp("host"))


_TRAJ = {}


def oracle_traj(oracle_mod, spec, key, nsteps):
    """The oracle's run of `spec` step by step, once per key: unfolded and folded positions, forces and the rebuild counter
    after every step (index 0: after run(0))."""
    if key not in _TRAJ:
        o = oracle_mod.OracleEngine()
        try:
            W.apply(spec, o, thermostat=False)
            o.run(0)
            t = dict(x=[o.get_state("POS_UNFOLDED")], xf=[o.get_state("POS")], f=[o.get_state("FORCE")], reb=[o.timers()["rebuilds"]])
            for _ in range(nsteps):
                o.run(1)
                t["x"].append(o.get_state("POS_UNFOLDED")); t["xf"].append(o.get_state("POS")); t["f"].append(o.get_state("FORCE"))
                t["reb"].append(o.timers()["rebuilds"])
        finally:
            o.close()
        _TRAJ[key] = t
    return _TRAJ[key]


def test_exact_pairs_is_the_all_pairs_sum_with_exclusions():
    spec = mass_ref.small_box_config()
    f, elj, etab, vir = H.pair_reference(spec)
    free = AR.exact_pairs(spec, spec["pos"], exclusions=[])
    assert rel_err(free["f"], f) < 1e-12
    assert free["epot_lj"] == pytest.approx(elj, rel=1e-12) and free["virial_nb"] == pytest.approx(vir, rel=1e-12) and free["epot_tab"] == etab == 0.0
    # the two excluded pairs, taken out of the all-pairs sum by hand
    L, prm = np.asarray(spec["box"]), H.pair_params(spec)[(0, 0)]
    tag = {int(i): k for k, i in enumerate(spec["ids"])}
    inside = 0
    for a, b in spec["exclusions"]:
        d = spec["pos"][tag[int(a)]] - spec["pos"][tag[int(b)]]
        d -= L * np.rint(d / L)
        ff, e = H.pair_eval(prm, d @ d)
        inside += int(d @ d < spec["rc"] ** 2)
        f[tag[int(a)]] -= ff * d; f[tag[int(b)]] += ff * d
        elj -= float(e); vir -= float(ff * (d @ d))
    assert inside == 2                                        # both exclusions remove a pair that would interact
    got = AR.exact_pairs(spec, spec["pos"])
    assert rel_err(got["f"], f) < 1e-12 and got["npairs"] == free["npairs"] - 2
    assert got["epot_lj"] == pytest.approx(elj, rel=1e-12) and got["virial_nb"] == pytest.approx(vir, rel=1e-12)
    assert got["jump"] == pytest.approx(0.039, rel=0.01)      # |F(rc)| of eps = sigma = 1, rc = 2.5


def test_exact_pairs_equals_the_oracle_along_a_melt(oracle_mod):
    spec = AR.melt_spec("melt2197", 0)
    t = oracle_traj(oracle_mod, spec, ("melt2197", 0), AR.MELT_STEPS)
    for s in (1, 10, 40, 80):
        ref = AR.exact_pairs(spec, t["xf"][s])
        err = rel_err(ref["f"], t["f"][s])
        print("step %d: exact_pairs against the oracle %.1e (%d pairs)" % (s, err, ref["npairs"]))
        assert err < 1e-12


@pytest.mark.parametrize("crit", [0, 1])
def test_rule_predicts_the_oracles_rebuilds_step_by_step(oracle_mod, crit):
    spec = dict(W.lj_melt(n=2197, seed=31, jitter=0.05, kT=1.5, dt=0.004), rebuild_criterion=crit)
    t = oracle_traj(oracle_mod, spec, ("rule", crit), 120)
    want = AR.increments(t["reb"])
    steps, unsure = AR.rule_rebuilds(t["x"], 0.5 * spec["skin"], crit)
    print("criterion %d: %d rebuilds in 120 steps, %d undecidable steps" % (crit, len(want), len(unsure)))
    assert steps == want and unsure == [] and len(want) >= 12


def test_rule_follows_an_engine_through_an_undecidable_step():
    """Two particles on a line; the second step brings the accumulated distance within 1e-6 of half the skin."""
    x = np.zeros((5, 2, 3))
    x[:, 0, 0] = [0.0, 0.1, 0.15 + 1e-6, 0.2, 0.31]
    for crit in (0, 1):
        assert AR.rule_rebuilds(x, 0.15, crit) == ([2, 4], [2])
        assert AR.rule_rebuilds(x, 0.15, crit, follow={3}) == ([3], [2])      # the engine let step 2 pass: 0.2 > 0.15 at step 3, then 0.11
        assert AR.rule_rebuilds(x, 0.15, crit, follow={2, 4}) == ([2, 4], [2])


@pytest.mark.parametrize("crit", [0, 1])
@pytest.mark.parametrize("name", list(AR.MELTS))
def test_guards_of_the_melts(oracle_mod, name, crit):
    spec = AR.melt_spec(name, crit)
    t = oracle_traj(oracle_mod, spec, (name, crit), AR.MELT_STEPS)
    steps, oldest = AR.check_steps(t["reb"])
    nreb = t["reb"][-1] - t["reb"][0]
    worst = dict(shell=0, ratio=0.0, err=0.0)
    for s in steps:
        ref = AR.exact_pairs(spec, t["xf"][s])
        worst["shell"] = max(worst["shell"], ref["shell_pairs"])
        worst["ratio"] = max(worst["ratio"], 2e-5 * ref["fmax"] / (ref["jump"] / 4))
        worst["err"] = max(worst["err"], rel_err(t["f"][s], ref["f"]))
        assert AR.guards(ref), (name, crit, s, ref["shell_pairs"], ref["fmax"], ref["jump"])
    print("%s criterion %d: %d particles, %d rebuilds, %d steps compared (%d at the oldest list), shell pairs <= %d, "
          "2e-5 fmax / (jump / 4) <= %.2f, oracle against exact_pairs %.1e" % (name, crit, spec["n"], nreb, len(steps), len(oldest),
                                                                            worst["shell"], worst["ratio"], worst["err"]))
    assert nreb >= 8 and len(oldest) >= 7
    assert worst["err"] < 1e-12
    unsure = AR.rule_rebuilds(t["x"], 0.5 * spec["skin"], crit)[1]
    assert len(unsure) <= 1


def test_list_skin_of_the_header(harness):
    """The effective list skin of the closing pairs and of the melt that runs with option list_skin, from pick_list_skin itself:
    the whole cell edge.  Criterion 1, a slab count that leaves one layer per rank, or a small box leave the workload's skin."""
    probe = dict(box=[32.0] * 3, rc=1.5, skin=0.3, ids=np.arange(140), rebuild_criterion=0)
    for dd, P in ((0, 1), (1, 1), (1, 2), (1, 3)):
        assert AR.effective_skin(harness, probe, 0.5, dd, P) == 2.0 * (1.0 - 1e-9) - 1.5
    assert AR.effective_skin(harness, dict(probe, rebuild_criterion=1), 0.5) == 0.3
    assert AR.effective_skin(harness, probe, 0.0) == 0.3
    m = AR.melt_spec("melt8788", 0)
    assert 0.6 < AR.effective_skin(harness, m, 0.5) == pytest.approx(m["box"][0] / 7 - 2.5, rel=1e-8)
    assert AR.effective_skin(harness, AR.melt_spec("melt2197", 0), 0.5) == 0.3            # four cells of 3.0: no list skin there


TIGHT_CASES = [(v, False) for v in AR.TIGHT_VARIANTS] + [("crit0", True), ("crit1", True)]


@pytest.mark.parametrize("variant,flat", TIGHT_CASES, ids=["%s%s" % (v, "-flat" if f else "") for v, f in TIGHT_CASES])
def test_tight_closing_pairs_on_the_oracle(make_oracle, harness, variant, flat):
    """No rebuild in the M steps, every closing pair ends inside rc and pulls with a force component above 0.5.  The oracle has
    no list skin of its own: the list_skin geometry runs with the effective skin as its skin.  flat: the 32 x 32 x 5 box of the
    brute-force list."""
    spec, opts = AR.tight_variant(variant, harness, flat=flat)
    se = spec["skin_eff"]
    ncl = int(spec["closing"].sum())
    assert (len(spec["ids"]), ncl) == ((72, 23) if flat else (140, 51 + 6))
    assert np.floor(np.asarray(spec["box"]) / (spec["rc"] + se)).min() == (2 if flat else 16 if opts else 17)
    o = make_oracle()
    W.apply(dict(spec, skin=se), o)
    o.run(0)
    r0, reb0 = AR.pair_separations(spec, o.get_state("POS")), o.timers()["rebuilds"]
    o.run(spec["M"])
    x = o.get_state("POS")
    r1 = AR.pair_separations(spec, x)
    cl = spec["closing"]
    assert o.timers()["rebuilds"] == reb0
    assert r0[cl].min() > spec["rc"] + 0.98 * se and r1[cl].max() < spec["rc"] - 1e-4
    assert np.allclose(r1[~cl], spec["rc"] - AR.RECEDE_START + 2 * AR.RECEDE_TRAVEL * se, atol=1e-3)
    ref, f = AR.exact_pairs(spec, x), o.get_state("FORCE")
    part = np.repeat(cl, 2)
    print("%s: skin_eff %.9f, closing pairs end at %.4f .. %.4f, smallest largest force component %.3f, straddling %s" %
          (variant, se, r1[cl].min(), r1[cl].max(), np.abs(f[part]).max(1).min(), spec["straddle"]))
    assert rel_err(f, ref["f"]) < 1e-12 and ref["npairs"] == ncl + 13 * int(r1[~cl].max() < spec["rc"])
    assert np.abs(f[part]).max(1).min() > 0.5 and np.abs(ref["f"][part]).max(1).min() > 0.5
    # the travel falls short of half the skin by 0.002 skin_eff, and the next step passes it
    d = o.get_state("POS_UNFOLDED") - spec["pos"]
    d -= np.asarray(spec["box"]) * np.rint(d / np.asarray(spec["box"]))
    assert 0.497 * se < np.sqrt((d * d).sum(1)).max() < 0.4995 * se
    o.run(1)
    assert o.timers()["rebuilds"] == reb0 + 1
