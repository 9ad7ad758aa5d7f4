"""The Berendsen barostat on the device (include/chem_mi355.h chem_barostat_berendsen) against tests/pressure_ref.py.

mu step by step     a 5 x 5 x 5-cell melt without a thermostat, 30 steps as run(1) calls: before each call the numpy stepper,
                    restarted from the engine's state, says what P will be after the step; the engine's box change implies
                    P0 + (mu^3 - 1) tau / dt.  Tolerance of the static pressure test (tests/test_gpu_pressure.py).  The edges
                    keep their ratios exactly, and run(30) ends bit for bit where 30 x run(1) ends.
lists under scaling a cold lattice (pressure_ref.cold_lattice: coordinates exactly representable, zero velocities, a thin skin)
                    compressed from five cells per axis to four -- the tile path hands over to the per-cell list in the middle
                    of the run -- and expanded from four to five, |mu - 1| about 1e-3 per step: forces, epot_lj and virial_nb
                    against aged_ref.exact_pairs at the engine's positions and box before the threshold (behind the step at
                    which pairs from outside the first build's list radius have come inside rc: the lists must have been built
                    again by the charge of the scalings alone), at the first step behind it and at the end (tolerances of
                    tests/test_gpu_aged_lists.py), the cell counts against what a fresh context plans at that box; the lists
                    are reused (a few builds in 75 steps).  The guard is confirmed on the CPU with the reference stepper
                    (tests/test_pressure_ref.py).  The same switches inside ONE run(n), bit for bit the run(1) sequence.
coexistence         a reactive melt with fixed distances and a Langevin thermostat, 200 steps: events and bonds against
                    tests/react_ref.py at the engine's positions, fixed distances at their length, P against the reference.
off and refusals    tau = 0 before the first step reproduces a context that never called it bit for bit; dd_self refuses the
                    call; mu^3 <= 0 stops the run with the named error."""
import ctypes

import numpy as np
import pytest

import aged_ref as AR
import helpers as H
import pressure_ref as PR
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from test_gpu_pair_matrix import _energy_ok
from test_gpu_parity import TOL as PTOL, TOL_MELT32

pytestmark = pytest.mark.gpu

TOL = {64: 1e-10, 32: 2e-5}


def tiles(g):
    out = (ctypes.c_int32 * 6)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    return int(out[0]), int(out[1])            # (tile count, cells along x)


def snapshot(g):
    return dict(x=g.get_state("POS_UNFOLDED"), xf=g.get_state("POS"), v=g.get_state("VEL"), f=g.get_state("FORCE"), L=g.box())


# ---- mu, step by step --------------------------------------------------------------------------------------------------------

def _melt():
    spec = AR.melt_spec("melt2197", 0)
    p = PR.pressure(spec, spec["pos"], spec["vel"])
    return spec, p


@pytest.mark.parametrize("prec", [64, 32])
def test_mu_step_by_step_and_in_one_call(make_gpu, prec):
    spec, p_start = _melt()
    dt, tau = spec["dt"], 5.0
    # |P - P0| of the order of P, on the side on which the box grows: the 5 x 5 x 5 cells stay (the thresholds have a test of their own)
    p0 = 0.5 * p_start["pressure"] if p_start["pressure"] > 0 else p_start["pressure"] - 1.0
    fn = PR.exact_force_fn(spec)
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_berendsen(p0, tau)
    g.run(0)
    assert tiles(g) == (8, 5) or tiles(g)[1] == 5
    ratios = None
    worst = 0.0
    for s in range(30):
        st = snapshot(g)
        xr, vr, fr, Lr, p_ref = PR.npt_step(spec, st["x"], st["v"], st["f"], st["L"], fn, dt, tau, p0)
        g.run(1)
        L = g.box()
        mu = L / st["L"]
        assert mu[0] == mu[1] == mu[2] or np.ptp(mu) <= 2.3e-16            # one factor for the three edges
        if ratios is None:
            ratios = st["L"] / st["L"][0]
        assert np.array_equal(L / L[0], ratios)                              # the edges keep their ratios exactly
        p_implied = p0 + (mu[0] ** 3 - 1.0) * tau / dt
        ref = PR.pressure(spec, xr / (Lr[0] / st["L"][0]), vr, box=st["L"])   # the state the step's pressure was taken from
        scale = ref["scale"] / (3.0 * ref["volume"])
        assert abs(ref["pressure"] - p_ref) <= 1e-12 * scale
        err = abs(p_implied - p_ref) / scale
        worst = max(worst, err)
        print("step %d fp%d: P ref %.8g implied %.8g  err/scale %.2e  mu-1 %.3e" % (s, prec, p_ref, p_implied, err, mu[0] - 1.0))
        assert err <= TOL[prec], (s, p_implied, p_ref)
        assert np.abs(g.get_state("POS_UNFOLDED") - xr).max() <= (1e-9 if prec == 64 else 1e-4)
    assert abs(g.box()[0] / spec["box"][0] - 1.0) > 1e-4                     # the box moved
    a = snapshot(g)
    b_eng = make_gpu(prec)
    W.apply(spec, b_eng, thermostat=False, reactions=False)
    b_eng.barostat_berendsen(p0, tau)
    b_eng.run(0)
    b_eng.run(30)
    b = snapshot(b_eng)
    for k in ("x", "v", "L"):
        assert np.array_equal(a[k], b[k]), k
    print("fp%d: worst err/scale %.2e over 30 steps" % (prec, worst))


# ---- lists under compression and expansion ---------------------------------------------------------------------------------

RC, SKIN, cold_lattice = PR.COLD_RC, PR.COLD_SKIN, PR.cold_lattice


CASES = {"shrink-crit0": ("shrink", {"rebuild_criterion": 0, "list_skin": 0}), "shrink-crit1": ("shrink", {"rebuild_criterion": 1, "list_skin": 0}),
         "shrink-list_skin": ("shrink", {"rebuild_criterion": 0, "list_skin": 0.15}), "grow-crit0": ("grow", {"rebuild_criterion": 0, "list_skin": 0}),
         "grow-crit1": ("grow", {"rebuild_criterion": 1, "list_skin": 0})}


def check_forces(spec, L, x, f, prec, what):
    at = dict(spec, box=np.asarray(L, np.float64), pos=x)
    ref = AR.exact_pairs(at, x)
    assert AR.guards(ref), ("ill-posed", what, ref["shell_pairs"], ref["fmax"], ref["jump"])
    if prec == 64:
        err, flips = rel_err(f, ref["f"]), 0
        assert err < PTOL[64], (what, err)
    else:
        err, flips = H.force_error_without_cutoff_flips(at, f, ref["f"], TOL_MELT32, max_flips=ref["shell_pairs"])
        assert err < TOL_MELT32 and 0 <= flips <= ref["shell_pairs"], (what, err, flips, ref["shell_pairs"])
    return err, flips, ref["shell_pairs"]


def check_obs(spec, L, x, obs, prec, what):
    at = dict(spec, box=np.asarray(L, np.float64), pos=x)
    ref = AR.exact_pairs(at, x)
    sc = H.energy_scales(at)
    for k in ("epot_lj", "virial_nb"):
        assert _energy_ok(obs[k], ref[k], prec, sc[k]), (what, k, obs[k], ref[k], sc[k])


def fresh_plan(make_gpu, prec, spec, opts, snap):
    f = make_gpu(prec)
    for k, v in opts.items():
        f.set_option(k, v)
    W.apply(dict(spec, box=snap["L"], pos=snap["xf"]), f, thermostat=False, reactions=False)
    f.run(0)
    return tiles(f)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", sorted(CASES))
def test_lists_follow_the_box(make_gpu, case, prec):
    direction, opts = CASES[case]
    spec = cold_lattice(direction)
    p0, tau = PR.cold_coupling(spec, direction)                             # mu^3 - 1 = -+3e-3 at the start: |mu - 1| = 1e-3
    g = make_gpu(prec)
    for k, v in opts.items():
        g.set_option(k, v)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_berendsen(p0, tau)
    g.run(0)
    t0 = tiles(g)
    print("%s fp%d: starts with %d tiles, %d cells along x" % (case, prec, t0[0], t0[1]))
    if case == "shrink-list_skin":
        assert t0[1] in (4, 5)                   # (the wider list skin decides how many cells the start has: read, not assumed)
    else:
        assert t0 == ((8, 5) if direction == "shrink" else (0, 4)) or (direction == "shrink" and t0[1] == 5 and t0[0] > 0)
    target = spec["box"][0] * (0.93 if direction == "shrink" else 1.04)
    marks, switched_at = {}, None

    def checkpoint(label, L_before):
        """Forces: the step's own evaluation, at the positions and the box before the scaling (also on the step behind which the
        geometry is planned again).  Then epot_lj and virial_nb at the current positions and box."""
        L = g.box()
        mu = L[0] / L_before[0]
        f, x = g.get_state("FORCE"), g.get_state("POS")
        fe = check_forces(spec, L_before, x / mu, f, prec, (case, label))
        check_obs(spec, L, x, g.observe(), prec, (case, label))
        plan = tiles(g)
        assert plan == fresh_plan(make_gpu, prec, spec, opts, dict(L=L, xf=x)), (case, label, plan)
        print("%s fp%d %s: L %.4f, %s, force err %.2e (%d flips of %d)" % ((case, prec, label, L[0], plan) + fe))
        marks[label] = dict(L=L, xf=x, plan=plan)

    # "before": under compression behind the step at which the first pair from outside the list radius of the first build has
    # come inside rc (step 35 of the reference stepper, tests/test_pressure_ref.py) and in front of the change of the cell count
    before_at = spec["box"][0] * (0.955 if direction == "shrink" else 1.003)
    for s in range(1, 201):
        L_before = g.box()
        g.run(1)
        now = tiles(g)
        if switched_at is None and "before" not in marks and ((g.box()[0] <= before_at) if direction == "shrink" else (g.box()[0] >= before_at)):
            checkpoint("before", L_before)
            assert now[1] == t0[1]
        if switched_at is None and now[1] != t0[1]:
            switched_at = s
            checkpoint("first_after", L_before)
        L = g.box()[0]
        if switched_at is not None and ((direction == "shrink" and L <= target) or (direction == "grow" and L >= target)):
            checkpoint("end", L_before)
            break
    assert switched_at is not None and "end" in marks, (case, g.box(), t0, switched_at)
    # the lists are reused across scalings: far fewer list builds than steps (each checkpoint's observe() and fresh plan may add
    # one), yet some -- the charge of the scalings uses the skin up although nothing moves thermally
    builds = g.timers()["list_rebuilds"]
    print("%s fp%d: %d list builds in %d steps" % (case, prec, builds, s))
    # (with option list_skin the list skin is the whole cell edge: a shrinking box asks for a new plan, and a build, on every step)
    assert 2 <= builds and (case == "shrink-list_skin" or builds <= s // 4 + 6), (builds, s)
    first_after, end = marks["first_after"], marks["end"]
    print("%s fp%d: cell count %d -> %d at step %d, ended at step %d" % (case, prec, t0[1], first_after["plan"][1], switched_at, s))
    if direction == "shrink" and case != "shrink-list_skin":
        assert first_after["plan"] == (0, 4) and end["plan"] == (0, 4)      # tiles need five cells per axis: the per-cell list took over
    if direction == "grow":
        assert first_after["plan"][1] == 5 and first_after["plan"][0] > 0   # ... and the tiles came back
    if direction == "shrink":
        from scipy.spatial import cKDTree
        Le = end["L"]
        ij = cKDTree(AR.fold(end["xf"], Le), boxsize=Le).query_pairs(RC, output_type="ndarray")
        d = spec["pos"][ij[:, 0]] - spec["pos"][ij[:, 1]]
        d -= spec["box"] * np.rint(d / spec["box"])
        far = np.sqrt((d * d).sum(1)) > RC + SKIN
        print("%s: %d pairs inside rc at the end were outside rc + skin at the first build" % (case, far.sum()))
        assert far.sum() > 0 and "before" in marks


@pytest.mark.parametrize("prec", [64, 32])
def test_forces_during_the_run_are_those_of_the_unscaled_positions(make_gpu, prec):
    """After a step the force array holds the step's own evaluation: exact pairs at the positions and the box BEFORE the scaling."""
    spec, p_start = _melt()
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_berendsen(p_start["pressure"] + 5.0, 4.0)
    g.run(7)
    L_before = g.box()
    g.run(1)
    mu = g.box()[0] / L_before[0]
    assert abs(mu - 1.0) > 1e-4
    snap = dict(xf=g.get_state("POS") / mu, f=g.get_state("FORCE"), obs=g.observe())
    ref = AR.exact_pairs(dict(spec, box=L_before), snap["xf"])
    err = np.abs(snap["f"] - ref["f"]).max() / ref["fmax"]
    moved = np.abs(AR.exact_pairs(dict(spec, box=g.box()), g.get_state("POS"))["f"] - ref["f"]).max() / ref["fmax"]
    print("fp%d: forces against the unscaled positions %.2e; the scaling itself moves them by %.2e" % (prec, err, moved))
    assert err <= (1e-9 if prec == 64 else 1e-4) and moved > 10 * err


# ---- off means off, refusals --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_off_means_off(make_gpu, prec):
    spec, _ = _melt()
    runs = []
    for touch in (False, True):
        g = make_gpu(prec)
        W.apply(spec, g, thermostat=True, reactions=False)
        if touch:
            g.barostat_berendsen(1.0, 0.5)
            g.barostat_berendsen(1.0, 0.0)
        g.run(25)
        runs.append((g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("FORCE"), g.box(), g.timers()["rebuilds"]))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.array_equal(runs[0][3], np.asarray(spec["box"], np.float64))


def test_refused_on_a_decomposed_context(make_gpu):
    spec, _ = _melt()
    g = make_gpu(64)
    g.set_option("dd_self", 1)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.run(0)
    with pytest.raises(ChemError, match="Berendsen barostat on a decomposed context: a gap of the decomposed path") as e:
        g.barostat_berendsen(1.0, 1.0)
    assert e.value.code == _capi.ENOTIMPL
    g.run(2)                                   # nothing of the refused call stays


@pytest.mark.parametrize("prec", [64, 32])
def test_mu3_not_positive_stops_the_run_by_name(make_gpu, prec):
    spec, p_start = _melt()
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    tau = spec["dt"] / 2.0                      # dt / tau = 2: mu^3 = 1 - 2 (P0 - P) <= 0 for P0 >= P + 1/2, from finite forces
    g.barostat_berendsen(p_start["pressure"] + 10.0, tau)
    with pytest.raises(ChemError, match=r"Berendsen barostat: mu\^3 = .* <= 0") as e:
        g.run(3)
    assert e.value.code == _capi.ESTATE
    assert np.isfinite(g.get_state("POS")).all() and np.array_equal(g.box(), np.asarray(spec["box"], np.float64))


# ---- the path switch inside one chem_run ---------------------------------------------------------------------------------------

SWITCH = {"shrink": 75, "grow": 40}      # steps: enough to cross the threshold (the step is printed by test_lists_follow_the_box)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("direction", ["shrink", "grow"])
def test_path_switch_inside_one_run(make_gpu, direction, prec):
    """The cell count crosses its threshold in the middle of ONE run(n), nothing probed in between: the run loop drifts with the
    old plan, plans again, rebuilds and evaluates the forces within the call.  The end state equals, bit for bit, that of n
    run(1) calls (where the plan is made between two calls), the forces are exact pairs at the positions before the last
    scaling, epot_lj and virial_nb at the current ones, the cell counts those of a fresh context."""
    spec = cold_lattice(direction)
    opts = {"rebuild_criterion": 0, "list_skin": 0}
    p0, tau = PR.cold_coupling(spec, direction)
    n = SWITCH[direction]

    def start():
        g = make_gpu(prec)
        for k, v in opts.items():
            g.set_option(k, v)
        W.apply(spec, g, thermostat=False, reactions=False)
        g.barostat_berendsen(p0, tau)
        return g
    a = start()
    a.run(0)
    t0 = tiles(a)
    for s in range(n - 1):
        a.run(1)                      # (box() below reads the host's copy of L: no probe of the geometry, no rebuild)
    L_before = a.box()
    a.run(1)
    b = start()
    b.run(n)
    sa, sb = snapshot(a), snapshot(b)
    for k in ("x", "v", "f", "L"):
        assert np.array_equal(sa[k], sb[k]), k
    mu = sb["L"][0] / L_before[0]
    fe = check_forces(spec, L_before, sb["xf"] / mu, sb["f"], prec, (direction, "one run"))
    plan = tiles(b)
    print("%s fp%d: %s -> %s within run(%d), force err %.2e (%d flips of %d)" % ((direction, prec, t0, plan, n) + fe))
    assert plan[1] == (4 if direction == "shrink" else 5) and t0[1] == (5 if direction == "shrink" else 4)
    assert (plan[0] > 0) == (direction == "grow") and (t0[0] > 0) == (direction == "shrink")
    assert plan == fresh_plan(make_gpu, prec, spec, opts, dict(L=sb["L"], xf=sb["xf"]))
    check_obs(spec, sb["L"], sb["xf"], b.observe(), prec, (direction, "one run"))


# ---- coexistence: reactions, fixed distances and a Langevin thermostat under the barostat ---------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_coexistence_reactions_fixed_distances_langevin(make_gpu, prec):
    """reactive_melt (4000 monomers, 6 cells per axis: the reaction scan reads the tiles of the step's force evaluation after
    the box has moved), 40 fixed distances, Langevin, 200 steps with the barostat on.  At every reaction step the events are
    those tests/react_ref.py finds at the engine's positions and box (reaction cutoffs do not scale); behind every drift the
    fixed distances are at their length (read back after the scaling of that step: mu times the length); the bond list at
    the end is the reference's; P at the end agrees with tests/pressure_ref.py."""
    import react_ref as RR
    from scipy.spatial import cKDTree
    interval, steps, dfix = 10, 200, 1.19
    spec = W.reactive_melt(n=4000, seed=23, interval=interval)
    L0 = np.asarray(spec["box"], np.float64)
    near = cKDTree(AR.fold(spec["pos"], L0), boxsize=L0).query_pairs(dfix + 0.03, output_type="ndarray")
    d = spec["pos"][near[:, 0]] - spec["pos"][near[:, 1]]
    d -= L0 * np.rint(d / L0)
    near = near[np.abs(np.sqrt((d * d).sum(1)) - dfix) < 0.03]
    used, fixp = set(), []
    for i, j in near[np.lexsort((near[:, 1], near[:, 0]))]:
        if i not in used and j not in used and len(fixp) < 40:
            used.update((int(i), int(j)))
            fixp.append((int(i) + 1, int(j) + 1))
    fixp = np.asarray(fixp, np.int64)
    assert len(fixp) == 40
    spec = dict(spec, exclusions=fixp)             # an anchor and its target do not see each other (nor react with each other)
    ref = RR.Reference(spec)
    g = make_gpu(prec)
    h = W.apply(spec, g)
    hf = g.fix_create(-1, -1)
    g.fix_add(hf, fixp, dfix)
    g.run(0)
    assert tiles(g)[0] > 0
    p0 = g.pressure()["pressure"] + 2.0
    g.barostat_berendsen(p0, 1.0)
    seen = 0
    for k in range(steps // interval):
        g.run(interval - 1)
        L_before = g.box()
        g.run(1)
        L, x = g.box(), g.get_state("POS")
        mu = L[0] / L_before[0]
        dd = x[fixp[:, 1] - 1] - x[fixp[:, 0] - 1]
        dd -= L * np.rint(dd / L)
        off = np.abs(np.sqrt((dd * dd).sum(1)) / mu - dfix).max()
        assert off <= (1e-12 if prec == 64 else 2e-6), (k, off)
        assert g.fix_count(hf) == 40
        ref.L = np.asarray(L, np.float64)
        ev, _ = ref.step(g.step, x)
        got = [e for e in RR.engine_events(g.get_events()) if e[0] == g.step]
        want = RR.ref_events(ev)
        assert [e[:4] for e in got] == [e[:4] for e in want], (k, g.step)
        assert all(abs(float.fromhex(a[4]) - float.fromhex(b[4])) <= 1e-12 * float.fromhex(b[4]) for a, b in zip(got, want))
        seen += len(want)
    assert g.step == steps and seen > 100 and abs(g.box()[0] / L0[0] - 1.0) > 1e-4
    snap = ref.snapshot()
    assert np.array_equal(g.get_list(h["reaction_bonds"]), snap["bonds"]) and len(snap["bonds"]) > 20
    assert np.array_equal(g.get_state("TYPE"), snap["type"]) and np.array_equal(g.get_state("STATE"), snap["state"])
    p = g.pressure()
    x, v = g.get_state("POS"), g.get_state("VEL")
    at = dict(spec, types=g.get_state("TYPE"), mass=g.get_state("MASS"), exclusions=g.get_exclusions())
    lists = [dict(name="reaction_bonds", kind=spec["reaction"]["bond"][0], arity=2, params=spec["reaction"]["bond"][1], ids=snap["bonds"])]
    pr = PR.pressure(at, x, v, box=g.box(), lists=lists)
    sc = pr["scale"] / (3.0 * pr["volume"])
    slack = 0.0
    if prec == 32:
        e = AR.exact_pairs(dict(at, box=g.box()), x)
        slack = e["shell_pairs"] * max(abs(float(H.pair_eval(q, H.pair_cutoff(q) ** 2, cut=False)[0])) * H.pair_cutoff(q) ** 2 for q in H.pair_params(at).values()) / (3.0 * pr["volume"])
    print("coexistence fp%d: %d events, %d bonds, box %.5f -> %.5f, P %.6f (ref %.6f, err/scale %.2e)" % (
        prec, seen, len(snap["bonds"]), L0[0], g.box()[0], p["pressure"], pr["pressure"], abs(p["pressure"] - pr["pressure"]) / sc))
    assert abs(p["pressure"] - pr["pressure"]) <= TOL[prec] * sc + slack
    assert abs(p["virial_list"][h["reaction_bonds"]] - pr["virial_list"][0]) <= TOL[prec] * pr["virial_list_scale"][0]
