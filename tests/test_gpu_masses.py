"""Per-particle masses through every kernel that reads or writes one (v4[i].w): the half kicks, the Langevin force, the
kinetic-energy reduction behind the rescaling thermostats, every cell sort, the migration between slabs, and the routes
that change a mass (reaction, neighbour rule, ATRP, dissociation, dynamic-resolution completion, modify_particle).

Every system carries a mass per PARTICLE (mass_ref.with_masses: log-uniform in [0.4, 25], no two equal, none exact in
fp32).  The guards of tests/test_oracle_masses.py are asserted again at the top of the tests that use a configuration: the
reference trajectory moves by more than 1e-2 when all masses become the mean mass, by more than 100 tolerances when two
particles of one cell exchange theirs, and the run rebuilds its lists at least three times.

The kick identity (mass_ref.kick_mass: m = dt |f0 + f1| / (2 |v1 - v0|) over one NVE step, from read-backs alone) ties the
mass the device integrates with to the one CHEM_STATE_MASS reports, also on the routes the oracle does not have.
Largest kick_mass errors seen on an MI355X (relative, over the qualifying particles): fp64 4.2e-12 (bound 1e-9; the stiff
dimers of the dissociation route, 9e-14 in the melts); fp32 7.6e-6, at most 0.044 of its per-particle bound
4 (2 eps32 |v| / |v1 - v0| + 2e-5), with 70 % (dissociation) to 90 % of the particles qualifying.
fp32 trajectories after 120 steps of the melt: POS_UNFOLDED 2e-7 to 9e-7, VEL 1.7e-5 to 3.5e-5 (tolerance 1e-4).

CHEM_STATE_MASS reads the device's mass word back, not a host copy: the fp64 build returns the input to the bit, the fp32
build float(m) to the bit (`stored`).  The read-back therefore does follow the particle through every sort and migration."""
import functools

import numpy as np
import pytest

import mass_ref as MR
from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import sorted_events
from test_gpu_parity import TOL, _HUB, _run_ranks
from test_oracle_masses import GPU_TOL, assert_guards, thermostat_on

pytestmark = pytest.mark.gpu

TRAJ = GPU_TOL                           # {64: 1e-9, 32: 1e-4}: POS_UNFOLDED and VEL, single domain
TRAJ_RX = {64: 1e-8, 32: 2e-4}           # on slabs and with reactions
EKIN = {64: 1e-12, 32: 1e-6}
NSTEPS = MR.NSTEPS


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def apply(spec, eng, th=None, **opts):
    for k, v in opts.items():
        eng.set_option(k, v)
    h = W.apply(spec, eng, thermostat=False)
    thermostat_on(eng, th)
    return h


@functools.lru_cache(maxsize=None)
def config(name, criterion=1):
    return dict(MR.CONFIGS[name](), rebuild_criterion=criterion)


_ORACLE = {}


def oracle_traj(oracle_mod, key, spec, chunks, th=None, cap=0.0):
    """The oracle's trajectory of a configuration, computed once per session and left unchanged."""
    if key not in _ORACLE:
        o = oracle_mod.OracleEngine()
        apply(spec, o, th)
        if cap:
            o.cap_force(cap)
        for k in chunks:
            o.run(k)
        _ORACLE[key] = dict(x=o.get_state("POS_UNFOLDED"), v=o.get_state("VEL"), xf=o.get_state("POS"), f=o.get_state("FORCE"), obs=o.observe(), rebuilds=o.timers()["rebuilds"])
        o.close()
    return _ORACLE[key]


def stored(mass, prec):
    """What CHEM_STATE_MASS reads back: the mass word of the device, v4[i].w, in the precision of the build.  The fp64 build
    returns the input to the bit; the fp32 build returns float(m) to the bit (none of the masses here is exact in fp32, so a
    mass that had gone through a narrower or a second rounding on its way would show)."""
    m = np.asarray(mass, dtype=np.float64)
    return m if prec == 64 else m.astype(np.float32).astype(np.float64)


def check_observables(obs, vel, mass, prec):
    """observe() against the fp64 sums over the engine's own velocities and the input masses"""
    ekin, temp, p = MR.observables(vel, mass)
    assert obs["ekin"] == pytest.approx(ekin, rel=EKIN[prec]) and obs["temperature"] == pytest.approx(temp, rel=EKIN[prec])
    assert np.abs(np.asarray(obs["momentum"]) - p).max() < EKIN[prec] * np.abs(np.asarray(mass)[:, None] * vel).sum()


_KICK = {64: [0.0], 32: [0.0, 0.0]}


def check_kick(g, dt, prec, mass, label):
    """One more NVE step: the mass of the two half kicks, from VEL and FORCE before and after, equals `mass`."""
    g.run(0)
    v0, f0 = g.get_state("VEL"), g.get_state("FORCE")
    g.run(1)
    v1, f1 = g.get_state("VEL"), g.get_state("FORCE")
    err, worst, share = MR.kick_mass_error(v0, v1, f0, f1, dt, mass, prec)
    _KICK[prec][0] = max(_KICK[prec][0], err)
    if prec == 32:
        _KICK[32][1] = max(_KICK[32][1], worst)
    print("kick_mass %s fp%d: largest relative error %.3e = %.3f of its bound, %.3f of the particles qualify (largest so far %r)"
          % (label, prec, err, worst, share, _KICK[prec]))
    assert share >= (0.95 if prec == 64 else 0.5)
    assert worst <= 1.0, (err, worst)


def engine(make_gpu, prec, spec, th=None, **opts):
    g = make_gpu(prec)
    h = apply(spec, g, th, **opts)
    return g, h


# ---- a: paths ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("tiles", [1, 0])
@pytest.mark.parametrize("name", ["melt", "small_box"])
def test_nve_paths_match_oracle(make_gpu, oracle_mod, name, tiles, prec, criterion):
    assert_guards(name, TRAJ[prec])
    spec = config(name, criterion)
    ref = oracle_traj(oracle_mod, (name, criterion, "nve"), spec, [NSTEPS])
    assert ref["rebuilds"] >= 3
    g, _ = engine(make_gpu, prec, spec, tiles=tiles)
    g.run(NSTEPS)
    x, v = g.get_state("POS_UNFOLDED"), g.get_state("VEL")
    print("%s tiles %d fp%d criterion %d: POS_UNFOLDED %.2e VEL %.2e, %d rebuilds" % (name, tiles, prec, criterion, rel_err(x, ref["x"]), rel_err(v, ref["v"]), g.timers()["rebuilds"]))
    if prec == 64:
        assert g.timers()["rebuilds"] == ref["rebuilds"]
    assert np.array_equal(g.get_state("MASS"), stored(spec["mass"], prec))
    check_observables(g.observe(), v, spec["mass"], prec)
    assert rel_err(x, ref["x"]) < TRAJ[prec] and rel_err(v, ref["v"]) < TRAJ[prec]
    check_kick(g, spec["dt"], prec, spec["mass"], "%s tiles %d criterion %d" % (name, tiles, criterion))


# ---- b: bit-identity arms ----------------------------------------------------------------------------------------------------

def final_state(g):
    return {w: g.get_state(w) for w in ("POS", "VEL", "FORCE", "IMAGE", "MASS")}


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("arm", ["fuse_integrate", "skip_idle", "split_run"])
def test_bit_identity_arms(make_gpu, prec, arm):
    assert_guards("melt", 0.0)
    spec = config("melt")
    runs = {"fuse_integrate": [dict(fuse_integrate=0), dict(fuse_integrate=1)],
            "skip_idle": [dict(skip_idle=0), dict(skip_idle=1), dict(skip_idle=2)],
            "split_run": [dict(), dict()]}[arm]
    out = []
    for k, opts in enumerate(runs):
        g, _ = engine(make_gpu, prec, spec, **opts)
        if arm == "split_run" and k == 1:
            g.run(47); g.run(NSTEPS - 47)
        else:
            g.run(NSTEPS)
        out.append(final_state(g))
        assert g.timers()["rebuilds"] >= 3
    for o in out[1:]:
        for w in o:
            assert np.array_equal(o[w], out[0][w]), (arm, w, np.abs(o[w] - out[0][w]).max())


# ---- c: thermostats ------------------------------------------------------------------------------------------------------------

THERMO_STEPS = (35, 25)          # two run() calls: the opening evaluation of the second draws the Langevin phase 0
SEED = 0x5eed0123456789


def three_types(spec):
    """the melt with types dealt round robin and one LJ for every pair of them: thermal groups have something to select"""
    rc = spec["rc"]
    return dict(spec, types=(np.arange(spec["n"]) % 3).astype(np.int32), lj=[(a, b, 1.0, 1.0, rc) for a in range(3) for b in range(a, 3)])


THERMOSTATS = {
    "langevin": (("langevin", 1.4, 2.0, SEED, None), 0.0, False),
    "langevin_groups": (("langevin", 1.4, 2.0, SEED, [0, 2]), 0.0, True),
    "langevin_cap": (("langevin", 1.4, 2.0, SEED, None), 12.0, False),
    "berendsen": (("berendsen", 0.6, 0.05), 0.0, False),
    "isokinetic": (("isokinetic", 0.6, 3), 0.0, False),
    "svr": (("svr", 0.6, 0.05, 5), 0.0, False),
}


def thermo_on(eng, th, cap):
    if th[0] == "svr":
        eng.thermostat_svr(th[1], th[2], th[3])
    else:
        thermostat_on(eng, th)
    if cap:
        eng.cap_force(cap)


@pytest.mark.parametrize("kind,prec", [(k, 64) for k in THERMOSTATS] + [("langevin", 32), ("berendsen", 32)])
def test_thermostats_match_oracle(make_gpu, oracle_mod, kind, prec):
    assert_guards("melt", TRAJ[prec])
    th, cap, typed = THERMOSTATS[kind]
    spec = three_types(config("melt")) if typed else config("melt")
    key = ("melt", "thermo", kind)
    if key not in _ORACLE:
        o = oracle_mod.OracleEngine()
        apply(spec, o)
        thermo_on(o, th, cap)
        for k in THERMO_STEPS:
            o.run(k)
        _ORACLE[key] = dict(x=o.get_state("POS_UNFOLDED"), v=o.get_state("VEL"), obs=o.observe(), rebuilds=o.timers()["rebuilds"])
        o.close()
    ref = _ORACLE[key]
    assert ref["rebuilds"] >= 3
    if cap:                                                # the cap acts on some particles of a melt like this and not on all
        fn = np.linalg.norm(oracle_traj(oracle_mod, ("melt", 1, "nve"), config("melt"), [NSTEPS])["f"], axis=1)
        assert 0.05 < (fn > cap).mean() < 0.95
    g = make_gpu(prec)
    apply(spec, g)
    thermo_on(g, th, cap)
    for k in THERMO_STEPS:
        g.run(k)
    x, v = g.get_state("POS_UNFOLDED"), g.get_state("VEL")
    print("%s fp%d: POS_UNFOLDED %.2e VEL %.2e" % (kind, prec, rel_err(x, ref["x"]), rel_err(v, ref["v"])))
    assert np.array_equal(g.get_state("MASS"), stored(spec["mass"], prec))
    check_observables(g.observe(), v, spec["mass"], prec)
    assert g.observe()["ekin"] == pytest.approx(ref["obs"]["ekin"], rel=1e-9 if prec == 64 else 1e-4)
    assert rel_err(x, ref["x"]) < TRAJ[prec] and rel_err(v, ref["v"]) < TRAJ[prec]


@pytest.mark.parametrize("groups", [None, (0, 2)])
def test_langevin_free_particles_match_numpy(make_gpu, groups):
    """Against the numpy restatement directly (a reference that is not the oracle): friction gamma m v, noise
    sqrt(24 kT gamma m / dt) (u - 1/2) with a Philox of its own.  300 particles: a partial integrate block."""
    spec = MR.free_particles(300, seed=81)
    th = ("langevin", 1.3, 2.0, 0x1234567890, list(groups) if groups else None)
    a = MR.verlet(spec, 7, thermostat=th)
    b = MR.verlet(dict(spec, pos=a["x"], vel=a["v"]), 5, thermostat=th, step0=7)
    assert rel_err(MR.verlet(MR.mean_mass(spec), 7, thermostat=th)["v"], a["v"]) > 1e-2
    g = make_gpu(64)
    apply(spec, g, th)
    g.run(7); g.run(5)
    assert rel_err(g.get_state("POS_UNFOLDED"), b["x"]) < TRAJ[64] and rel_err(g.get_state("VEL"), b["v"]) < TRAJ[64]
    assert rel_err(g.get_state("FORCE"), b["f"]) < TOL[64]


# ---- d: slabs ------------------------------------------------------------------------------------------------------------------

def on_ranks(make_gpu, P, prec, body):
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        engs[r].comm_init_local(P, r, hub)
        return body(engs[r])
    return _run_ranks(P, rank)


@pytest.mark.parametrize("kind", ["nve", "berendsen"])
@pytest.mark.parametrize("P", [2, 3])
def test_slabs_carry_the_masses(make_gpu, oracle_mod, P, kind):
    fig = assert_guards("slab", TRAJ_RX[64])
    spec = config("slab")
    th = None if kind == "nve" else ("berendsen", 1.2, 0.05)
    ref = oracle_traj(oracle_mod, ("slab", kind), spec, [NSTEPS], th)
    moved = (MR.slab_of(spec, spec["pos"], P) != MR.slab_of(spec, ref["xf"], P)).sum()
    assert moved >= 20, moved

    def body(g):
        apply(spec, g, th)
        g.run(NSTEPS)
        return dict(x=g.get_state("POS_UNFOLDED"), v=g.get_state("VEL"), m=g.get_state("MASS"), obs=g.observe())
    for out in on_ranks(make_gpu, P, 64, body):
        print("slabs P %d %s: POS_UNFOLDED %.2e VEL %.2e (%d particles changed slab)" % (P, kind, rel_err(out["x"], ref["x"]), rel_err(out["v"], ref["v"]), moved))
        assert np.array_equal(out["m"], spec["mass"])
        check_observables(out["obs"], out["v"], spec["mass"], 64)
        assert out["obs"]["ekin"] == pytest.approx(ref["obs"]["ekin"], rel=1e-8)
        assert rel_err(out["x"], ref["x"]) < TRAJ_RX[64] and rel_err(out["v"], ref["v"]) < TRAJ_RX[64]


# ---- e: mass changes -----------------------------------------------------------------------------------------------------------

M1, M2 = 3.0 ** 0.5, 128.0 ** 0.5          # 1.732..., 11.31...: neither exact in fp32, both far from what they replace
A, B, C, D = 0, 1, 2, 3


def reactive(spec, restate):
    """A + B -> C:D (restate: A:B, the current types named again) on a two-type version of `spec`, harmonic bonds; every
    particle reacts at most once.  The new masses differ from the old ones and from each other."""
    rng = np.random.default_rng(5)
    rc = spec["rc"]
    rx = dict(type_1=A, type_2=B, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1, delta_1=1, delta_2=1, rate=1e9, cutoff=1.15,
              intramolecular=False, intraresidual=False, is_virtual=False, new_type_1=A if restate else C, new_type_2=B if restate else D,
              new_mass_1=M1, new_mass_2=M2)
    return dict(spec, types=rng.integers(0, 2, spec["n"]).astype(np.int32), state=np.zeros(spec["n"], np.int32),
                res_id=np.arange(1, spec["n"] + 1, dtype=np.int32), lj=[(a, b, 1.0, 1.0, rc) for a in range(4) for b in range(a, 4)], reaction_desc=rx)


def add_reaction(eng, spec, interval=10):
    hb = eng.list_create(2, "HARMONIC", False)
    eng.list_set_params(hb, [30.0, 0.97])
    eng.reaction_init(interval, True, 0, 77)
    eng.reaction_add(bond_list=hb, **spec["reaction_desc"])
    eng.reactions_enable(True)
    return hb


def reaction_mass_model(spec, events):
    """include/chem_mi355.h, chem_reaction_desc: new_mass is used when the type changes -- and only then"""
    rx = spec["reaction_desc"]
    types, mass = spec["types"].copy(), spec["mass"].copy()
    for _, ida, idb, _, _ in events:
        for pid, nt, nm in ((ida, rx["new_type_1"], rx["new_mass_1"]), (idb, rx["new_type_2"], rx["new_mass_2"])):
            if nt >= 0 and nt != types[pid - 1]:
                types[pid - 1], mass[pid - 1] = nt, nm
    return types, mass


def reaction_route(g, spec):
    add_reaction(g, spec)
    g.run(10)                      # the first reaction step
    g.run(45)                      # and four more, the first change 45 steps back
    g.reactions_enable(False)
    return g


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("restate", [False, True])
def test_route_reaction(make_gpu, make_oracle, restate, prec):
    """Routes 1 and 2.  restate: the reaction names the types the particles already have, with other masses -- the type
    does not change, so neither does the mass: on the device (what CHEM_STATE_MASS reads back and the kicks use) as in the host
    mirror and the oracle.  (k_react_apply used to write new_mass wherever a type was named: read-back and kicks then showed
    M1 / M2 on every reacted particle, the oracle and the mirror the old masses.)"""
    assert_guards("melt", TRAJ_RX[prec])
    spec = reactive(config("melt"), restate)
    g, _ = engine(make_gpu, prec, spec)
    reaction_route(g, spec)
    ev = sorted_events(g.get_events())
    types, mass = reaction_mass_model(spec, ev)
    changed = (mass != spec["mass"]).sum()
    print("reaction route (restate %s) fp%d: %d events, %d masses changed" % (restate, prec, len(ev), changed))
    assert len(ev) >= 100 and (changed == 0 if restate else changed == 2 * len(ev))
    assert np.array_equal(g.get_state("TYPE"), types)
    assert np.array_equal(g.get_state("MASS"), stored(mass, prec))
    if prec == 64:
        o = make_oracle()
        apply(spec, o)
        reaction_route(o, spec)
        assert [e[:4] for e in ev] == [e[:4] for e in sorted_events(o.get_events())]
        assert np.array_equal(o.get_state("MASS"), mass)
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < TRAJ_RX[64]
        assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < TRAJ_RX[64]
    check_observables(g.observe(), g.get_state("VEL"), mass, prec)
    check_kick(g, spec["dt"], prec, mass, "reaction restate %s" % restate)


def test_route_reaction_on_two_slabs(make_gpu, make_oracle):
    assert_guards("slab", TRAJ_RX[64])
    spec = reactive(config("slab"), False)
    o = make_oracle()
    apply(spec, o)
    reaction_route(o, spec)
    ev = sorted_events(o.get_events())
    types, mass = reaction_mass_model(spec, ev)
    assert len(ev) >= 100 and np.array_equal(o.get_state("MASS"), mass)

    def body(g):
        apply(spec, g)
        reaction_route(g, spec)
        out = dict(ev=sorted_events(g.get_events()), x=g.get_state("POS_UNFOLDED"), v=g.get_state("VEL"), m=g.get_state("MASS"), obs=g.observe())
        check_kick(g, spec["dt"], 64, out["m"], "reaction on two slabs")
        return out
    for out in on_ranks(make_gpu, 2, 64, body):
        assert [e[:4] for e in out["ev"]] == [e[:4] for e in ev]
        assert np.array_equal(out["m"], mass)
        check_observables(out["obs"], out["v"], mass, 64)
        assert rel_err(out["x"], o.get_state("POS_UNFOLDED")) < TRAJ_RX[64] and rel_err(out["v"], o.get_state("VEL")) < TRAJ_RX[64]


def test_route_neighbour_rule(make_gpu, make_oracle):
    """Route 3: the trimer melt of test_change_neighbours_property_matches_oracle with a mass per particle; the middle beads
    one bond from an event become PL with mass M1, the far ends two bonds away PA with mass M2."""
    MA, ML, PA, PL = 0, 1, 2, 3
    spec = W.trimer_melt(n_mol=216, seed=6, interval=20)
    spec["lj"] += [(PA, t, 1.0, 1.0, spec["rc"]) for t in (MA, ML, PA)] + [(PL, t, 1.0, 1.0, spec["rc"]) for t in (MA, ML, PA, PL)]
    spec = MR.with_masses(spec, 75)
    spec["rebuild_criterion"] = 1
    g, o = make_gpu(64), make_oracle()
    for e in (g, o):
        W.apply(spec, e, thermostat=False)
        e.reaction_neighbour_change(0, "both", ML, 1, PL, M1, new_state=1)
        e.reaction_neighbour_change(0, "both", MA, 2, PA, M2)
        e.run(20)
        e.run(45)
        e.reactions_enable(False)
    ty = g.get_state("TYPE")
    assert np.array_equal(ty, o.get_state("TYPE")) and (ty == PL).sum() >= 5 and (ty == PA).sum() >= 5
    # the rule: a particle whose type the rule changed carries the rule's mass, every other particle the mass it came with
    # (the reaction itself names no new type)
    mass = np.where(ty == PL, M1, np.where(ty == PA, M2, spec["mass"]))
    assert np.array_equal(g.get_state("MASS"), mass) and np.array_equal(o.get_state("MASS"), mass)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < TRAJ_RX[64]
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < TRAJ_RX[64]
    check_kick(g, spec["dt"], 64, mass, "neighbour rule")


def test_route_atrp(make_gpu, make_oracle):
    """Route 4: two centres, one flipping type 0 into type 1 with mass M1, one naming type 2 again with mass M2.  A flip
    sets type / mass / q to the centre's where the type differs; a centre that restates the type leaves the mass alone."""
    assert_guards("melt", TRAJ_RX[64])
    spec = three_types(config("melt"))
    spec["types"] = np.where(spec["types"] == 1, 0, spec["types"]).astype(np.int32)           # types 0 and 2; 1 only by a flip
    spec["state"] = np.zeros(spec["n"], np.int32)
    spec["atrp"] = dict(interval=10, num_particles=400, ratio_activator=0.5, ratio_deactivator=0.5, delta_catalyst=0.3, k_activate=1.6,
                        k_deactivate=0.6, select_from_all=True, seed=17,
                        centers=[dict(type_id=0, state=0, is_activator=False, new_type=1, new_mass=M1, delta_state=1),
                                 dict(type_id=2, state=0, is_activator=False, new_type=2, new_mass=M2, delta_state=1)])
    g, o = make_gpu(64), make_oracle()
    for e in (g, o):
        W.apply(spec, e, thermostat=False)
        e.run(10)
        e.run(45)
        e.atrp_disconnect()
    assert g.atrp_stats() == o.atrp_stats()
    st, ty = g.get_state("STATE"), g.get_state("TYPE")
    flipped = st == 1
    assert (flipped & (spec["types"] == 0)).sum() >= 20 and (flipped & (spec["types"] == 2)).sum() >= 20
    assert np.array_equal(ty, np.where(flipped & (spec["types"] == 0), 1, spec["types"])) and np.array_equal(ty, o.get_state("TYPE"))
    mass = np.where(flipped & (spec["types"] == 0), M1, spec["mass"])
    assert np.array_equal(g.get_state("MASS"), mass) and np.array_equal(o.get_state("MASS"), mass)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < TRAJ_RX[64]
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < TRAJ_RX[64]
    check_kick(g, spec["dt"], 64, mass, "atrp")


@pytest.mark.parametrize("prec", [64, 32])
def test_route_dissociation(make_gpu, prec):
    """Route 5: 1000 dimers (tests/test_gpu_dissociation.py), every fourth one stretched beyond the break distance; the role-1
    particle of a broken bond becomes type 2 with mass M1, the role-2 particle type 2 with mass M2 (every third list entry
    is stored the other way round, so that roles and list order differ).
    For the fp32 kick identity half of the particles must feel a force that matters beside their velocity.  The fragments of
    a broken dimer fly free (LJ sigma 0.4), so only a quarter is broken; a bonded particle oscillates with
    omega = sqrt(2 K / mu), and |v1 - v0| / |v| = dt omega |tan(phase)|, so K = 200 and dt = 0.004 put dt omega between 0.02
    (both particles at mass 25) and 0.2 (both at 0.4), and the thermal velocities (kT = 0.01) well below the oscillation's."""
    import test_gpu_dissociation as TD
    lengths = np.where(np.arange(1000) % 4 == 0, 1.3, 0.9)
    pos, types, bonds = TD.dimers(lengths)
    spec = TD.make_spec(pos, types, bonds)
    spec["lists"] = [dict(spec["lists"][0], params=[200.0, TD.R0])]
    spec = MR.with_masses(dict(spec, dt=0.004, kT=0.01), 76)
    g = make_gpu(prec)
    h = W.apply(spec, g, thermostat=False, reactions=False)
    g.reaction_init(1, True, 0, TD.SEED)
    g.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h[0], new_type_1=2, new_type_2=2, new_mass_1=M1, new_mass_2=M2, **TD.RX)
    g.reactions_enable(True)
    g.run(1)
    g.reactions_enable(False)
    ev = g.get_events()
    assert len(ev) == 250 and (ev["step"] == 1).all()
    mass = spec["mass"].copy()
    assert (spec["types"][ev["id_a"] - 1] == 0).all() and (spec["types"][ev["id_b"] - 1] == 1).all()
    mass[ev["id_a"] - 1], mass[ev["id_b"] - 1] = M1, M2
    g.run(45)
    assert np.array_equal(g.get_state("MASS"), stored(mass, prec))
    assert ((g.get_state("TYPE") == 2) == (mass != spec["mass"])).all()
    check_observables(g.observe(), g.get_state("VEL"), mass, prec)
    check_kick(g, spec["dt"], prec, mass, "dissociation")


@pytest.mark.parametrize("prec", [64, 32])
def test_route_resolution_completion(make_gpu, prec):
    """Route 6: nine type-1 particles ramp from lambda 0 at 1/8 per step; at step 8 they become type 0 with mass M2."""
    assert_guards("melt", TRAJ[prec])
    spec = config("melt")
    rc = spec["rc"]
    chosen = np.arange(40, spec["n"], 250)
    types = np.zeros(spec["n"], np.int32)
    types[chosen] = 1
    lam = np.where(types == 1, 0.0, 1.0)
    spec = dict(spec, types=types, lam=lam, lj=[(a, b, 1.0, 1.0, rc) for a in range(2) for b in range(a, 2)], resolution=[(0, 1, 0.0), (1, 1, 0.0)],
                res_rates=[dict(type_id=1, alpha=1 / 8, new_type=0, new_mass=M2, new_q=0.0)])
    g, _ = engine(make_gpu, prec, spec)
    g.run(7)
    assert np.array_equal(g.get_state("MASS"), stored(spec["mass"], prec)) and np.array_equal(g.get_state("TYPE"), types)
    g.run(1)
    mass = np.where(types == 1, M2, spec["mass"])
    assert len(chosen) == 9 and np.array_equal(g.get_state("MASS"), stored(mass, prec)) and (g.get_state("TYPE") == 0).all()
    g.run(45)
    assert np.array_equal(g.get_state("MASS"), stored(mass, prec))
    check_observables(g.observe(), g.get_state("VEL"), mass, prec)
    check_kick(g, spec["dt"], prec, mass, "resolution completion")


MODIFIED = {7: 13.37 ** 0.5, 512: 0.45 * 2 ** 0.5, 513: 21.0 ** 0.5, 2197: 2.0 ** 0.5}        # id: new mass (both sides of a block border, the last particle)


@pytest.mark.parametrize("prec", [64, 32])
def test_route_modify_particle(make_gpu, make_oracle, prec):
    """Route 7: modify_particle(id, "mass", m) between two runs."""
    assert_guards("melt", TRAJ[prec])
    spec = config("melt")
    g, o = make_gpu(prec), make_oracle()
    mass = spec["mass"].copy()
    for e in (g, o):
        apply(spec, e)
        e.run(20)
        for pid, m in MODIFIED.items():
            e.modify_particle(pid, "mass", m)
        e.run(45)
    for pid, m in MODIFIED.items():
        mass[pid - 1] = m
    assert np.array_equal(g.get_state("MASS"), stored(mass, prec)) and np.array_equal(o.get_state("MASS"), mass)
    check_observables(g.observe(), g.get_state("VEL"), mass, prec)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < TRAJ[prec]
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < TRAJ[prec]
    check_kick(g, spec["dt"], prec, mass, "modify_particle")


def test_route_modify_particle_on_two_slabs(make_gpu, oracle_mod):
    """Route 7 on two slabs, on three particles chosen from the oracle's own trajectory: one deep inside its slab, one in the
    boundary layer of its slab (the other rank holds a ghost copy of it) and one that changes slab after the change."""
    assert_guards("slab", TRAJ_RX[64])
    spec = config("slab")
    P, first, then = 2, 20, 100
    L = spec["box"][2]
    ref = oracle_traj(oracle_mod, ("slab", "nve"), spec, [NSTEPS])
    mid = oracle_traj(oracle_mod, ("slab", "nve", first), spec, [first])
    s_mid, s_end = MR.slab_of(spec, mid["xf"], P), MR.slab_of(spec, ref["xf"], P)
    zb = L * 6 / 12                                                      # the boundary between the two slabs (layers 0-5 | 6-11); the other is z = 0
    dist = np.minimum(np.abs(mid["xf"][:, 2] - zb), np.minimum(mid["xf"][:, 2], L - mid["xf"][:, 2]))
    inside = int(np.argmax(dist))
    layer = int(np.nonzero((dist > 0.5) & (dist < 1.0) & (s_mid == s_end))[0][0])
    o = None
    for cand in np.nonzero(s_mid != s_end)[0][:8]:                       # changed slab without the change: does it still, 1.5 times as heavy?
        pick = {int(spec["ids"][inside]): 2.0 ** 0.5, int(spec["ids"][layer]): 5.0 ** 0.5, int(spec["ids"][cand]): 1.5 * spec["mass"][cand]}
        o = oracle_mod.OracleEngine()
        apply(spec, o)
        o.run(first)
        for pid, m in pick.items():
            o.modify_particle(pid, "mass", m)
        o.run(then)
        if MR.slab_of(spec, o.get_state("POS"), P)[cand] != s_mid[cand]:
            break
        o.close()
        o = None
    assert o is not None, "no particle changes slab after its mass was changed"
    mass = spec["mass"].copy()
    for pid, m in pick.items():
        mass[pid - 1] = m
    xo, vo = o.get_state("POS_UNFOLDED"), o.get_state("VEL")
    o.close()

    def body(g):
        apply(spec, g)
        g.run(first)
        for pid, m in pick.items():
            g.modify_particle(pid, "mass", m)
        g.run(then)
        out = dict(x=g.get_state("POS_UNFOLDED"), v=g.get_state("VEL"), m=g.get_state("MASS"), obs=g.observe())
        check_kick(g, spec["dt"], 64, mass, "modify_particle on two slabs")
        return out
    for out in on_ranks(make_gpu, P, 64, body):
        assert np.array_equal(out["m"], mass)
        check_observables(out["obs"], out["v"], mass, 64)
        assert rel_err(out["x"], xo) < TRAJ_RX[64] and rel_err(out["v"], vo) < TRAJ_RX[64]
