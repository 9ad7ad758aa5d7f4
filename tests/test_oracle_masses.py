"""Per-particle masses on the CPU: the oracle against the numpy restatement of tests/mass_ref.py, equipartition under
Langevin, and the guards of the configurations tests/test_gpu_masses.py runs.

Measured deviations oracle / mass_ref.verlet (rel_err, this suite's own runs on the CPU; the bounds are 100 x these, never
looser than 1e-9 and never tighter than 100 eps of fp64 = 2.2e-14, which a different but equally valid order of the
same fp64 operations may reach):
    NVE melt, 500 particles, 60 steps, 8 rebuilds       POS_UNFOLDED 1.1e-16   VEL 4.6e-15
    Berendsen, 40 steps                                 POS_UNFOLDED 2.1e-16   VEL 5.8e-15
    isokinetic (coupling 3), 40 steps                   POS_UNFOLDED 3.2e-16   VEL 6.0e-15
    free particles, Langevin, 12 steps in two runs      POS_UNFOLDED 1.0e-16   VEL 0 (bit-identical)
"""
import functools

import numpy as np
import pytest

import mass_ref as MR
from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import pair_reference

STATIC = 1e-12          # forces at step 0 and observables, as test_oracle_pair_matrix


def bound(measured):
    return min(max(100.0 * measured, 100.0 * np.finfo(np.float64).eps), 1e-9)


def thermostat_on(eng, th):
    if th is None:
        return
    if th[0] == "langevin":
        eng.thermostat_langevin(th[1], th[2], th[3])
        if th[4]:
            eng.thermostat_langevin_types(th[4])
    else:
        eng.thermostat_rescale(th[0], th[1], th[2])


def oracle_run(make_oracle, spec, chunks, th=None):
    o = make_oracle()
    spec = dict(spec)
    spec.setdefault("rebuild_criterion", 1)
    W.apply(spec, o, thermostat=False)
    thermostat_on(o, th)
    for k in chunks:
        o.run(k)
    return o


@functools.lru_cache(maxsize=None)
def small_melt():
    return MR.with_masses(W.lj_melt(n=500, seed=61, jitter=0.05), 62)


def test_with_masses_properties():
    spec = small_melt()
    m = spec["mass"]
    assert len(np.unique(m)) == len(m) and m.min() > 0.39 and m.max() < 25.1
    assert not (m.astype(np.float32).astype(np.float64) == m).any()
    assert np.log(m).std() == pytest.approx(np.log(25 / 0.4) / np.sqrt(12), rel=0.1)      # log-uniform
    ekin, temp, p = MR.observables(spec["vel"], m)
    assert np.abs(p).max() < 1e-12 * np.abs(m[:, None] * spec["vel"]).sum()
    assert temp == pytest.approx(spec["kT"], rel=5 * np.sqrt(2.0 / (3 * len(m))))
    # each particle's own Maxwell distribution: the light and the heavy half are equally hot
    light = m < np.median(m)
    for half in (light, ~light):
        assert MR.observables(spec["vel"][half], m[half])[1] == pytest.approx(spec["kT"], rel=5 * np.sqrt(2.0 / (3 * half.sum())))


def test_static_forces_and_observables(make_oracle):
    spec = small_melt()
    o = oracle_run(make_oracle, spec, [0])
    f, elj, _, _ = pair_reference(spec)
    assert rel_err(o.get_state("FORCE"), f) < STATIC
    obs = o.observe()
    ekin, temp, p = MR.observables(spec["vel"], spec["mass"])
    assert obs["ekin"] == pytest.approx(ekin, rel=STATIC) and obs["temperature"] == pytest.approx(temp, rel=STATIC)
    assert obs["epot_lj"] == pytest.approx(elj, rel=1e-11)
    assert np.array_equal(o.get_state("MASS"), spec["mass"])
    pscale = np.abs(spec["mass"][:, None] * spec["vel"]).sum()
    assert np.abs(np.asarray(obs["momentum"]) - p).max() < STATIC * pscale
    # and with a net momentum, so that the comparison is not one of two roundings of zero
    spec2 = dict(spec, vel=spec["vel"] + np.array([0.3, -0.2, 0.1]))
    o2 = oracle_run(make_oracle, spec2, [0])
    ekin2, temp2, p2 = MR.observables(spec2["vel"], spec["mass"])
    obs2 = o2.observe()
    assert rel_err(obs2["momentum"], p2) < STATIC and obs2["ekin"] == pytest.approx(ekin2, rel=STATIC)


MEASURED = dict(nve=(1.1e-16, 4.6e-15), berendsen=(2.1e-16, 5.8e-15), isokinetic=(3.2e-16, 6.0e-15), langevin=(1.0e-16, 0.0))


@pytest.mark.parametrize("kind,nsteps,th", [("nve", 60, None), ("berendsen", 40, ("berendsen", 0.7, 0.05)),
                                            ("isokinetic", 40, ("isokinetic", 0.7, 3))])
def test_oracle_melt_matches_numpy_verlet(make_oracle, kind, nsteps, th):
    spec = small_melt()
    o = oracle_run(make_oracle, spec, [nsteps], th)
    ref = MR.verlet(spec, nsteps, thermostat=th)
    ex, ev = rel_err(o.get_state("POS_UNFOLDED"), ref["x"]), rel_err(o.get_state("VEL"), ref["v"])
    print("oracle / mass_ref.verlet %s: POS_UNFOLDED %.2e VEL %.2e rebuilds %d" % (kind, ex, ev, o.timers()["rebuilds"]))
    if kind == "nve":
        assert o.timers()["rebuilds"] >= 3
    else:
        assert abs(o.observe()["temperature"] - 0.7) < abs(MR.observables(spec["vel"], spec["mass"])[1] - 0.7)    # it does thermostat
    assert ex < bound(MEASURED[kind][0]) and ev < bound(MEASURED[kind][1])
    assert rel_err(o.get_state("FORCE"), ref["f"]) < 1e-9
    obs = o.observe()
    ekin, temp, p = MR.observables(o.get_state("VEL"), spec["mass"])
    assert obs["ekin"] == pytest.approx(ekin, rel=STATIC) and obs["temperature"] == pytest.approx(temp, rel=STATIC)
    assert np.abs(np.asarray(obs["momentum"]) - p).max() < STATIC * np.abs(spec["mass"][:, None] * o.get_state("VEL")).sum()
    assert np.array_equal(o.get_state("MASS"), spec["mass"])


def test_kick_identity_recovers_the_masses_and_sees_a_swap(make_oracle):
    """mass_ref.kick_mass on the oracle's own read-backs: the input masses to 1e-9, in both ways of qualifying; exchanging the
    masses of two particles of one cell, or giving everybody the mean mass, in the claimed masses breaks the bound."""
    spec = small_melt()
    o = oracle_run(make_oracle, spec, [20, 0])
    v0, f0 = o.get_state("VEL"), o.get_state("FORCE")
    o.run(1)
    v1, f1 = o.get_state("VEL"), o.get_state("FORCE")
    for prec in (64, 32):
        err, worst, share = MR.kick_mass_error(v0, v1, f0, f1, spec["dt"], spec["mass"], prec)
        assert err < 1e-9 and worst <= 1.0 and share >= (0.95 if prec == 64 else 0.5), (prec, err, worst, share)
        a, b = MR.same_cell_pair(spec)
        for wrong in (MR.swapped(spec, a, b), MR.mean_mass(spec)):
            assert MR.kick_mass_error(v0, v1, f0, f1, spec["dt"], wrong["mass"], prec)[1] > 100.0


@pytest.mark.parametrize("groups", [None, (0, 2)])
def test_oracle_langevin_free_particles_match_numpy(make_oracle, groups):
    """The friction gamma m v and the noise sqrt(24 kT gamma m / dt) of every particle, restated with a Philox of its own;
    two run() calls: the opening evaluation of the second draws phase 0 of its first step."""
    spec = MR.free_particles(300, seed=81)
    th = ("langevin", 1.3, 2.0, 0x1234567890, list(groups) if groups else None)
    o = oracle_run(make_oracle, spec, [7, 5], th)
    a = MR.verlet(spec, 7, thermostat=th)
    b = MR.verlet(dict(spec, pos=a["x"], vel=a["v"]), 5, thermostat=th, step0=7)
    ex, ev = rel_err(o.get_state("POS_UNFOLDED"), b["x"]), rel_err(o.get_state("VEL"), b["v"])
    print("oracle / mass_ref.verlet langevin %s: POS_UNFOLDED %.2e VEL %.2e" % (groups, ex, ev))
    assert ex < bound(MEASURED["langevin"][0]) and ev < bound(MEASURED["langevin"][1])
    assert rel_err(o.get_state("FORCE"), b["f"]) < STATIC
    if groups:      # the unlisted type flies on untouched
        off = spec["types"] == 1
        assert np.array_equal(o.get_state("VEL")[off], spec["vel"][off])


def test_equipartition_under_langevin(make_oracle):
    """Three mass classes in one melt: after equilibration <m v^2> / 3 of every class is kT.  A noise or a friction that
    carried the mass in another power would heat the classes differently (friction gamma v instead of gamma m v: T ~ 1/m);
    two implementations that share the formula cannot see that in a trajectory comparison.  N_c = 576 per class, S = 4 samples
    3.2 / gamma apart: relative standard error sqrt(2 / (3 N_c S)) = 1.7 %, asserted within five of those."""
    gamma, kT = 5.0, 1.0
    spec = MR.with_masses(W.lj_melt(n=1728, seed=91, jitter=0.05, kT=kT, gamma=gamma), 92, classes=(0.4, 3.0, 25.0))
    o = make_oracle()
    W.apply(spec, o)
    o.run(400)                                     # 10 / gamma
    apart = int(np.ceil(3.2 / gamma / spec["dt"]))
    assert apart * spec["dt"] >= 3.0 / gamma
    S, temps = 4, {c: [] for c in (0.4, 3.0, 25.0)}
    for _ in range(S):
        o.run(apart)
        v = o.get_state("VEL")
        for c in temps:
            sel = spec["mass"] == c
            temps[c].append(MR.observables(v[sel], spec["mass"][sel])[1])
    nc = 576
    assert all((spec["mass"] == c).sum() == nc for c in temps)
    rse = np.sqrt(2.0 / (3 * nc * S))
    assert rse <= 0.02
    for c, t in temps.items():
        print("equipartition: class m = %-4g  <m v^2>/3 = %.4f  (%.2f standard errors from kT)" % (c, np.mean(t), (np.mean(t) - kT) / (rse * kT)))
    for c, t in temps.items():
        assert abs(np.mean(t) - kT) < 5 * rse * kT, (c, np.mean(t))


# ---- guards of the GPU configurations: CPU assertions on the reference (the oracle, which is what the GPU runs are held to) ----

GPU_TOL = {64: 1e-9, 32: 1e-4}          # the trajectory tolerances of tests/test_gpu_masses.py, single domain


@functools.lru_cache(maxsize=None)
def guard_figures(name):
    """For one configuration: what the reference's trajectory moves by (rel_err of POS_UNFOLDED and VEL after NSTEPS) when
    every mass becomes the mean mass and when two particles of one cell exchange theirs; the rebuild count of the true run."""
    from oracle import oracle
    oracle.build()
    spec = MR.CONFIGS[name]()
    a, b = MR.same_cell_pair(spec)
    out = {}
    for key, sp in (("true", spec), ("mean", MR.mean_mass(spec)), ("swap", MR.swapped(spec, a, b))):
        o = oracle.OracleEngine()
        sp = dict(sp)
        sp.setdefault("rebuild_criterion", 1)
        W.apply(sp, o, thermostat=False)
        o.run(MR.NSTEPS)
        out[key] = (o.get_state("POS_UNFOLDED"), o.get_state("VEL"), o.timers()["rebuilds"], o.get_state("POS"))
        o.close()
    t = out["true"]
    fig = dict(rebuilds=t[2], pair=(a, b), spec=spec, end_pos=t[3])
    for key in ("mean", "swap"):
        fig[key] = (rel_err(out[key][0], t[0]), rel_err(out[key][1], t[1]))
    return fig


def assert_guards(name, tol):
    """The three guards of one configuration for a comparison at tolerance `tol`."""
    fig = guard_figures(name)
    print("guards %s: mean mass moves POS %.2e VEL %.2e; swapping %r moves POS %.2e VEL %.2e; %d rebuilds"
          % ((name,) + fig["mean"] + (fig["pair"],) + fig["swap"] + (fig["rebuilds"],)))
    assert min(fig["mean"]) > 1e-2
    assert min(fig["swap"]) > 100 * tol
    assert fig["rebuilds"] >= 3
    return fig


@pytest.mark.parametrize("name", sorted(MR.CONFIGS))
def test_guards_of_the_gpu_configurations(name):
    assert_guards(name, GPU_TOL[32])
    if name == "slab":
        fig = guard_figures(name)
        for P in (2, 3):
            moved = (MR.slab_of(fig["spec"], fig["spec"]["pos"], P) != MR.slab_of(fig["spec"], fig["end_pos"], P)).sum()
            print("guards slab: %d particles end in another of %d slabs" % (moved, P))
            assert moved >= 20
