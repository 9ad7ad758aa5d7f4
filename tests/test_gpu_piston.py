"""The Langevin piston barostat on the device (include/chem_mi355.h chem_barostat_langevin) against tests/piston_ref.py.
Tolerances are those of tests/test_gpu_barostat.py (the quantities compared are the same sums).

step by step        a 5 x 5 x 5-cell melt without a thermostat, 30 steps as run(1) calls: before each call the numpy stepper,
                    restarted from the engine's x, v, f, L and piston momentum, says what follows; afterwards the momentum
                    agrees to TOL dt S (S = the sum of the absolute terms of G), the box is L exp(dt pe / W) to rounding with its
                    edge ratios kept exactly, the positions agree.  run(30) ends bit for bit where 30 x run(1) ends.
noise and friction  the same with gammaP = 1, kT = 1.5 and a Langevin thermostat on the particles: the momentum comparison uses the
                    restated draw, so a wrong counter, key or amplitude fails.
conserved quantity  H from chem_observe, chem_get_box and the state: 30 steps at dt against 60 at dt / 2, ratio of the maximum
                    deviations between 3 and 5 (tests/test_piston_ref.py: 3.95).
lists follow        the cold lattice of tests/test_piston_ref.py's guard, compressed from five cells per axis to four and
                    expanded from four to five: forces, epot_lj and virial_nb against aged_ref.exact_pairs at the engine's own
                    positions and box on the step before the crossing, on the first step behind it and at the end; the cell
                    counts those of a fresh context; fewer list builds than steps; ONE run(n) is bit for bit the run(1) sequence.
off means off       mass = 0 before the first step, or on and off again before any step: bit for bit a context that never called it.
coexistence         reactions, fixed distances and a Langevin thermostat with the piston on.
refusals            dd_self, the two barostats together, and the arithmetic stop by name."""
import numpy as np
import pytest

import aged_ref as AR
import helpers as H
import mass_ref as MR
import piston_ref as PS
import pressure_ref as PR
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from test_gpu_barostat import TOL, check_forces, check_obs, fresh_plan, snapshot, tiles
from test_piston_ref import CELL, COLD_W

pytestmark = pytest.mark.gpu

XTOL = {64: 1e-9, 32: 1e-4}


def _melt():
    spec = AR.melt_spec("melt2197", 0)
    return spec, PR.pressure(spec, spec["pos"], spec["vel"])["pressure"]


def _follow(make_gpu, prec, spec, p0, mass, gamma_p, kT, seed, nsteps, thermostat):
    """nsteps x run(1), each compared with the reference stepper restarted from the engine's state.  Returns the engine."""
    dt = spec["dt"]
    fn = PR.exact_force_fn(spec)
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=thermostat, reactions=False)
    g.barostat_langevin(p0, mass, gamma_p, kT, seed)
    g.run(0)
    assert tiles(g)[1] == 5
    st0 = g.barostat_state()
    assert st0["kind"] == 2 and st0["momentum"] == 0.0 and st0["mu_next"] == 1.0 and st0["sv_next"] == 1.0
    m, types = np.asarray(spec["mass"], np.float64), np.asarray(spec["types"])
    ratios, worst = None, 0.0
    for s in range(nsteps):
        st, pe = snapshot(g), g.barostat_state()["momentum"]
        step_index = g.step
        thermo = (lambda v: MR.langevin_force(v, m, types, spec["kT"], spec["gamma"], dt, spec["seed"], step_index, 1)) if thermostat else None
        ref = PS.piston_step(spec, st["x"], st["v"], st["f"], st["L"], pe, fn, dt, p0, mass, gamma_p, kT, seed, step_index + 1, thermo_fn=thermo)
        g.run(1)
        now = g.barostat_state()
        assert now["kind"] == 2
        L = g.box()
        if ratios is None:
            ratios = st["L"] / st["L"][0]
        assert np.array_equal(L / L[0], ratios)                                  # the edges keep their ratios exactly
        assert np.abs(L / (st["L"] * np.exp(dt * pe / mass)) - 1.0).max() <= 1e-14    # the box is host double in both builds
        pr = PR.pressure(spec, ref["x"], ref["v"], box=ref["L"])
        assert abs(pr["pressure"] - ref["P"]) <= 1e-12 * pr["scale"] / (3.0 * pr["volume"])
        S = pr["scale"] + 3.0 * pr["volume"] * abs(p0)
        err = abs(now["momentum"] - ref["pe"]) / (dt * S)
        worst = max(worst, err)
        print("step %d fp%d: pe ref %.8g engine %.8g  err/(dt S) %.2e  mu-1 %.3e  P %.6g (ref %.6g)" % (s, prec, ref["pe"], now["momentum"], err, ref["mu"] - 1.0, now["pressure_last"], ref["P"]))
        assert err <= TOL[prec], (s, now["momentum"], ref["pe"])
        assert abs(now["eps_dot"] - now["momentum"] / mass) <= 1e-15 * abs(now["eps_dot"])
        assert np.abs(g.get_state("POS_UNFOLDED") - ref["x"]).max() <= XTOL[prec]
    print("fp%d: worst err/(dt S) %.2e over %d steps" % (prec, worst, nsteps))
    return g


@pytest.mark.parametrize("prec", [64, 32])
def test_step_by_step_and_in_one_call(make_gpu, prec):
    spec, p_start = _melt()
    p0, mass = 0.5 * p_start, 5000.0
    g = _follow(make_gpu, prec, spec, p0, mass, 0.0, 0.0, 0, 30, False)
    assert abs(g.box()[0] / spec["box"][0] - 1.0) > 1e-4                     # the box moved
    a, pa = snapshot(g), g.barostat_state()["momentum"]
    b_eng = make_gpu(prec)
    W.apply(spec, b_eng, thermostat=False, reactions=False)
    b_eng.barostat_langevin(p0, mass, 0.0, 0.0, 0)
    b_eng.run(0)
    b_eng.run(30)
    b = snapshot(b_eng)
    for k in ("x", "v", "L"):
        assert np.array_equal(a[k], b[k]), k
    assert pa == b_eng.barostat_state()["momentum"]


@pytest.mark.parametrize("prec", [64, 32])
def test_momentum_survives_a_change_of_parameters(make_gpu, prec):
    """A call that only changes parameters while the barostat is on keeps pe; the factors of the next step follow the new mass
    (box, positions and momentum of that step against the reference stepper with the new parameters)."""
    spec, p_start = _melt()
    dt, p0 = spec["dt"], 0.5 * p_start
    fn = PR.exact_force_fn(spec)
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_langevin(p0, 5000.0, 0.0, 0.0, 0)
    g.run(5)
    pe = g.barostat_state()["momentum"]
    assert pe != 0.0
    g.barostat_langevin(0.75 * p0, 500.0, 0.0, 0.0, 0)
    now = g.barostat_state()
    assert now["kind"] == 2 and now["momentum"] == pe
    assert abs(now["mu_next"] - np.exp(dt * pe / 500.0)) <= 1e-15 * now["mu_next"] and abs(now["eps_dot"] - pe / 500.0) <= 1e-15 * abs(pe / 500.0)
    st = snapshot(g)
    ref = PS.piston_step(spec, st["x"], st["v"], st["f"], st["L"], pe, fn, dt, 0.75 * p0, 500.0, 0.0, 0.0, 0, g.step + 1)
    g.run(1)
    assert np.abs(g.box() / (st["L"] * np.exp(dt * pe / 500.0)) - 1.0).max() <= 1e-14
    assert np.abs(g.get_state("POS_UNFOLDED") - ref["x"]).max() <= XTOL[prec]
    pr = PR.pressure(spec, ref["x"], ref["v"], box=ref["L"])
    S = pr["scale"] + 3.0 * pr["volume"] * abs(0.75 * p0)
    assert abs(g.barostat_state()["momentum"] - ref["pe"]) <= TOL[prec] * dt * S


@pytest.mark.parametrize("prec", [64, 32])
def test_noise_and_piston_friction(make_gpu, prec):
    spec, p_start = _melt()
    spec = dict(spec, gamma=1.0, kT=1.5, seed=77)
    g = _follow(make_gpu, prec, spec, 0.5 * p_start, 5000.0, 1.0, 1.5, 99, 10, True)
    # the noise is there: the same run with another seed of the piston has another momentum
    h = make_gpu(prec)
    W.apply(spec, h, thermostat=True, reactions=False)
    h.barostat_langevin(0.5 * p_start, 5000.0, 1.0, 1.5, 100)
    h.run(10)
    assert h.barostat_state()["momentum"] != g.barostat_state()["momentum"]


def _h_deviation(make_gpu, spec, p0, mass, dt, nsteps):
    g = make_gpu(64)
    W.apply(dict(spec, dt=dt), g, thermostat=False, reactions=False)
    g.barostat_langevin(p0, mass, 0.0, 0.0, 0)
    g.run(0)
    hs = []
    for s in range(nsteps):
        pe = g.barostat_state()["momentum"]
        g.run(1)
        ob, pe_new = g.observe(), g.barostat_state()["momentum"]
        pe_full = pe + 0.5 * (pe_new - pe)                                       # pe + dt G / 2 with the step's own G
        hs.append(ob["ekin"] + ob["epot_lj"] + p0 * float(np.prod(g.box())) + pe_full * pe_full / (2.0 * mass))
    hs = np.asarray(hs)
    return float(np.abs(hs - hs[0]).max()), float(abs(hs[0]))


def test_conserved_quantity_on_the_device(make_gpu):
    spec, p_start = _melt()
    p0, mass, dt = 0.5 * p_start, 500.0, spec["dt"]
    d1, h = _h_deviation(make_gpu, spec, p0, mass, dt, 30)
    d2, _ = _h_deviation(make_gpu, spec, p0, mass, 0.5 * dt, 60)
    print("H = %.6g: max deviation %.4g at dt, %.4g at dt / 2, ratio %.2f" % (h, d1, d2, d1 / d2))
    assert 3.0 <= d1 / d2 <= 5.0


# ---- lists follow the box ------------------------------------------------------------------------------------------------------

def _cold(direction):
    spec = PR.cold_lattice(direction)
    p_start = PR.pressure(spec, spec["pos"], spec["vel"])["pressure"]
    return spec, p_start + (PR.COLD_DP if direction == "shrink" else -PR.COLD_DP)


def _cells(L):
    return int(np.floor(L / CELL))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("direction", ["shrink", "grow"])
def test_lists_follow_the_box(make_gpu, direction, criterion, prec):
    spec, p0 = _cold(direction)
    opts = {"rebuild_criterion": criterion, "list_skin": 0}
    what = "%s crit%d fp%d" % (direction, criterion, prec)

    def start():
        e = make_gpu(prec)
        for k, v in opts.items():
            e.set_option(k, v)
        W.apply(spec, e, thermostat=False, reactions=False)
        e.barostat_langevin(p0, COLD_W, 0.0, 0.0, 0)
        return e
    g = start()
    g.run(0)
    t0 = tiles(g)
    assert t0[1] == (5 if direction == "shrink" else 4) and (t0[0] > 0) == (direction == "shrink")
    marks = {}

    def checkpoint(label):
        """The state between steps is consistent: forces, epot_lj and virial_nb are exact pairs at the positions and the box
        read back; the plan is the one a fresh context makes at that box."""
        L, x, f = g.box(), g.get_state("POS"), g.get_state("FORCE")
        fe = check_forces(spec, L, x, f, prec, (what, label))
        check_obs(spec, L, x, g.observe(), prec, (what, label))
        plan = tiles(g)
        assert plan == fresh_plan(make_gpu, prec, spec, opts, dict(L=L, xf=x)), (what, label, plan)
        assert plan[1] == _cells(L[0])
        print("%s %s at step %d: L %.4f, %s, force err %.2e (%d flips of %d)" % ((what, label, g.step, L[0], plan) + fe))
        marks[label] = g.step

    crossed, worst = None, 0.0
    for s in range(1, 201):
        st = g.barostat_state()
        worst = max(worst, abs(st["mu_next"] - 1.0))
        if crossed is None and _cells(g.box()[0] * st["mu_next"]) != t0[1]:
            checkpoint("before")                          # the next step's scaling crosses the threshold
        g.run(1)
        if crossed is None and _cells(g.box()[0]) != t0[1]:
            crossed = s
            checkpoint("first_after")
        if crossed is not None and s == crossed + 10:
            checkpoint("end")
            break
    assert crossed is not None and 60 <= crossed <= 150 and worst < 2e-3, (what, crossed, worst)      # (the guard of tests/test_piston_ref.py)
    assert marks["before"] == crossed - 1 and marks["first_after"] == crossed and marks["end"] == crossed + 10
    n = g.step
    builds = g.timers()["list_rebuilds"]
    print("%s: cell count %d -> %d at step %d, %d list builds in %d steps, max |mu - 1| %.3g" % (what, t0[1], tiles(g)[1], crossed, builds, n, worst))
    assert 2 <= builds < n
    assert tiles(g)[1] == (4 if direction == "shrink" else 5) and (tiles(g)[0] > 0) == (direction == "grow")
    # the same run as ONE run(n): nothing probed in between, bit for bit the run(1) sequence
    a = start()
    for s in range(n):
        a.run(1)
    b = start()
    b.run(n)
    sa, sb = snapshot(a), snapshot(b)
    for k in ("x", "v", "f", "L"):
        assert np.array_equal(sa[k], sb[k]), (what, k)
    assert a.barostat_state()["momentum"] == b.barostat_state()["momentum"]
    assert tiles(a) == tiles(b)
    check_forces(spec, sb["L"], sb["xf"], sb["f"], prec, (what, "one run"))


# ---- off means off ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_off_means_off(make_gpu, prec):
    import react_ref as RR
    spec = W.reactive_melt(n=2744, seed=23, interval=10)      # (the reactive melt needs an even lattice: 14^3, five cells per axis)
    runs = []
    for touch in (0, 1, 2):
        g = make_gpu(prec)
        W.apply(spec, g)
        if touch == 1:
            g.barostat_langevin(1.0, 0.0, 1.0, 1.0, 5)
        if touch == 2:
            g.barostat_langevin(1.0, 50.0, 1.0, 1.0, 5)
            assert g.barostat_state()["kind"] == 2
            g.barostat_langevin(1.0, 0.0, 1.0, 1.0, 5)
        assert g.barostat_state()["kind"] == 0
        g.run(50)
        ev = RR.engine_events(g.get_events())
        runs.append((g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("FORCE"), g.box(), ev, g.timers()["rebuilds"]))
    assert len(runs[0][4]) > 0
    for other in runs[1:]:
        for a, b in zip(runs[0][:4], other[:4]):
            assert np.array_equal(a, b)
        assert runs[0][4] == other[4] and runs[0][5] == other[5]
    assert np.array_equal(runs[0][3], np.asarray(spec["box"], np.float64))


# ---- coexistence: reactions, fixed distances and a Langevin thermostat under the piston --------------------------------------------

def test_coexistence_reactions_fixed_distances_langevin(make_gpu):
    """The set-up of tests/test_gpu_barostat.py's coexistence test (fp32) with the piston on, 200 steps.  At every reaction step
    the events are those tests/react_ref.py finds at the engine's positions and box; the fixed distances, restored behind the
    scaling of every step, are at their length; the bond list at the end is the reference's; P agrees with the reference."""
    import react_ref as RR
    from scipy.spatial import cKDTree
    prec, interval, steps, dfix = 32, 10, 200, 1.19
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
    spec = dict(spec, exclusions=fixp)
    ref = RR.Reference(spec)
    g = make_gpu(prec)
    h = W.apply(spec, g)
    hf = g.fix_create(-1, -1)
    g.fix_add(hf, fixp, dfix)
    g.run(0)
    assert tiles(g)[0] > 0
    p0 = g.pressure()["pressure"] + 2.0
    g.barostat_langevin(p0, 2000.0, 1.0, spec["kT"], 41)
    seen = 0
    for k in range(steps // interval):
        g.run(interval)
        L, x = g.box(), g.get_state("POS")
        dd = x[fixp[:, 1] - 1] - x[fixp[:, 0] - 1]
        dd -= L * np.rint(dd / L)
        off = np.abs(np.sqrt((dd * dd).sum(1)) - dfix).max()
        assert off <= 2e-6, (k, off)                      # absolute lengths: set behind the scaling, not scaled
        assert g.fix_count(hf) == 40
        ref.L = np.asarray(L, np.float64)
        ev, _ = ref.step(g.step, x)
        got = [e for e in RR.engine_events(g.get_events()) if e[0] == g.step]
        want = RR.ref_events(ev)
        assert [e[:4] for e in got] == [e[:4] for e in want], (k, g.step)
        assert all(abs(float.fromhex(a[4]) - float.fromhex(b[4])) <= 1e-12 * float.fromhex(b[4]) for a, b in zip(got, want))
        seen += len(want)
    st = g.barostat_state()
    assert g.step == steps and seen > 100 and abs(g.box()[0] / L0[0] - 1.0) > 1e-4 and st["kind"] == 2
    snap = ref.snapshot()
    assert np.array_equal(g.get_list(h["reaction_bonds"]), snap["bonds"]) and len(snap["bonds"]) > 20
    assert np.array_equal(g.get_state("TYPE"), snap["type"]) and np.array_equal(g.get_state("STATE"), snap["state"])
    p = g.pressure()
    x, v = g.get_state("POS"), g.get_state("VEL")
    at = dict(spec, types=g.get_state("TYPE"), mass=g.get_state("MASS"), exclusions=g.get_exclusions())
    lists = [dict(name="reaction_bonds", kind=spec["reaction"]["bond"][0], arity=2, params=spec["reaction"]["bond"][1], ids=snap["bonds"])]
    pr = PR.pressure(at, x, v, box=g.box(), lists=lists)
    sc = pr["scale"] / (3.0 * pr["volume"])
    e = AR.exact_pairs(dict(at, box=g.box()), x)
    slack = e["shell_pairs"] * max(abs(float(H.pair_eval(q, H.pair_cutoff(q) ** 2, cut=False)[0])) * H.pair_cutoff(q) ** 2 for q in H.pair_params(at).values()) / (3.0 * pr["volume"])
    print("coexistence fp%d: %d events, %d bonds, box %.5f -> %.5f, P %.6f (ref %.6f, err/scale %.2e), pe %.4g" % (
        prec, seen, len(snap["bonds"]), L0[0], g.box()[0], p["pressure"], pr["pressure"], abs(p["pressure"] - pr["pressure"]) / sc, st["momentum"]))
    assert abs(p["pressure"] - pr["pressure"]) <= TOL[prec] * sc + slack
    assert abs(p["virial_list"][h["reaction_bonds"]] - pr["virial_list"][0]) <= TOL[prec] * pr["virial_list_scale"][0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_on_a_decomposed_context(make_gpu):
    spec, _ = _melt()
    g = make_gpu(64)
    g.set_option("dd_self", 1)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.run(0)
    with pytest.raises(ChemError, match="Langevin barostat on a decomposed context: a gap of the decomposed path") as e:
        g.barostat_langevin(1.0, 50.0, 1.0, 1.0, 0)
    assert e.value.code == _capi.ENOTIMPL
    assert g.barostat_state()["kind"] == 0
    g.run(2)                                   # nothing of the refused call stays


def test_one_barostat_at_a_time(make_gpu):
    spec, _ = _melt()
    g = make_gpu(64)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_berendsen(1.0, 5.0)
    with pytest.raises(ChemError, match="Langevin barostat: the Berendsen barostat is on") as e:
        g.barostat_langevin(1.0, 50.0, 1.0, 1.0, 0)
    assert e.value.code == _capi.EINVAL and g.barostat_state()["kind"] == 1
    g.barostat_langevin(1.0, 0.0, 0.0, 0.0, 0)             # switching the other one off touches nothing
    assert g.barostat_state()["kind"] == 1
    g.barostat_berendsen(1.0, 0.0)
    g.barostat_langevin(1.0, 50.0, 1.0, 1.0, 0)
    with pytest.raises(ChemError, match="Berendsen barostat: the Langevin barostat is on") as e:
        g.barostat_berendsen(1.0, 5.0)
    assert e.value.code == _capi.EINVAL and g.barostat_state()["kind"] == 2
    g.run(2)
    assert g.barostat_state()["momentum"] != 0.0


@pytest.mark.parametrize("prec", [64, 32])
def test_momentum_not_finite_stops_the_run_by_name(make_gpu, prec):
    """An arithmetic stop on the host: exp overflows for a piston of next to no mass.  Nothing faults on the device."""
    spec, p_start = _melt()
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.barostat_langevin(p_start + 10.0, 1e-12, 0.0, 0.0, 0)
    with pytest.raises(ChemError, match=r"Langevin barostat: .*step 1 .*P = .*P0 = ") as e:
        g.run(3)
    assert e.value.code == _capi.ESTATE
    assert np.isfinite(g.get_state("POS")).all() and np.array_equal(g.box(), np.asarray(spec["box"], np.float64))
    g.barostat_langevin(0.0, 0.0, 0.0, 0.0, 0)             # off: the context goes on
    assert g.barostat_state()["kind"] == 0 and g.barostat_state()["momentum"] == 0.0
    g.run(3)
    assert np.isfinite(g.get_state("POS")).all() and np.isfinite(g.get_state("VEL")).all()
