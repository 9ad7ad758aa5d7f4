"""Region rules on the device (include/chem_mi355.h, chem_region_add ff.: FreezeRegion, ChangeParticleType) against
tests/region_ref.py.

The positions the reference needs are the engine's own: every system is run once in single steps, CHEM_STATE_POS read after
each and fed to region_ref, and once more in one call.  Changes (step, id, rule), stats, types and the whole state must agree
to the bit between the two runs, the logs and types with the reference.

Systems: jittered lattices, coordinates snapped to what both precisions hold exactly, region edges multiples of 1/8; rc 1.5,
skin 0.3; "t" 9.0^3 (five cells per axis: fused tile path, 512 particles), "c" 5.4^3 (three cells: per-cell lists, 216), "b"
4.5^3 (two cells: brute-force list, 125).  Types: 0 and 1 interact by LJ, 2 ("frozen") has no potential; no thermostat
unless said."""
import numpy as np
import pytest

import bonded_ref as B
import region_ref as G
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError

pytestmark = pytest.mark.gpu

RC, SKIN, DT = 1.5, 0.3, 0.002
BOXES = {"t": (9.0, 8), "c": (5.4, 6), "b": (4.5, 5)}      # edge, lattice points per axis
LJ = (1.0, 0.5, 1.3)
FROZEN = 2
MODES = {G.MODE_ALL: "all", G.MODE_PROB: "prob", G.MODE_NUM: "num", G.MODE_FRACTION: "fraction"}


def melt(shape, seed=1, kT=4.0, types=None):
    edge, m = BOXES[shape]
    rng = np.random.default_rng(seed)
    a = edge / m
    grid = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = (grid + 0.5) * a + rng.uniform(-0.1, 0.1, grid.shape)
    n = len(pos)
    ty = rng.integers(0, 2, n).astype(np.int32) if types is None else np.full(n, types, np.int32)
    spec = dict(n=n, box=[edge] * 3, rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, n + 1), types=ty, pos=pos,
                vel=rng.normal(0.0, np.sqrt(kT), (n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), kT=kT, gamma=0.0, seed=1,
                lj=[(0, 0) + LJ, (0, 1) + LJ, (1, 1) + LJ])
    return W.snap_to_grid(spec)


def slabs(edge, w, target, new, modes, **kw):
    """the six FreezeRegion slabs in the order -x, x, -y, y, -z, z"""
    out = []
    for d in range(3):
        for side in (0, 1):
            lo, hi = [0.0] * 3, [edge] * 3
            if side == 0:
                hi[d] = w
            else:
                lo[d] = edge - w
            mode, value, num = modes[len(out) % len(modes)]
            out.append(G.rule(lo, hi, target, new, mode=mode, value=value, num=num, seed=1000 + len(out), **kw))
    return out


def send_rules(g, rules, enable=True, **kw):
    idx = []
    for r in rules:
        k = g.region_add(r["lo"], r["hi"], r["target_type"], r["new_type"], interval=r["interval"], mode=MODES[r["mode"]], value=r["value"],
                         num=r["num"], seed=r["seed"], **kw)
        if enable and r["enabled"]:
            g.region_enable(k)
        idx.append(k)
    return idx


def logs(g):
    ch = [(int(c["step"]), int(c["id"]) - 1, int(c["rule"])) for c in g.region_changes()]
    st = [(int(s["step"]), int(s["rule"]), int(s["candidates"]), int(s["changed"])) for s in g.region_stats()]
    return ch, st


def state_of(g):
    return {k: g.get_state(k) for k in ("POS", "VEL", "TYPE", "STATE", "MASS")}


def stepwise_and_whole(make_gpu, prec, spec, rules, nsteps, setup=None, **kw):
    """(engine run in single steps, engine run in one call, positions per step, reference (changes, stats, types))"""
    g1, g2 = make_gpu(prec), make_gpu(prec)
    for g in (g1, g2):
        W.apply(spec, g, thermostat=spec["gamma"] > 0, reactions=False)
        if setup:
            setup(g)
        send_rules(g, rules, **kw)
    pos = {}
    for s in range(1, nsteps + 1):
        g1.run(1)
        pos[s] = g1.get_state("POS")
    g2.run(nsteps)
    ref = G.run(rules, pos, spec["types"], np.array(spec["box"]))
    return g1, g2, pos, ref


def assert_agree(g1, g2, ref):
    ch1, st1 = logs(g1)
    ch2, st2 = logs(g2)
    print("changes: %d in single steps, %d in one call, %d in the reference; stats rows %d / %d / %d" % (len(ch1), len(ch2), len(ref[0]), len(st1), len(st2), len(ref[1])))
    assert ch1 == ref[0] and st1 == ref[1]
    assert ch2 == ref[0] and st2 == ref[1]
    s1, s2 = state_of(g1), state_of(g2)
    assert np.array_equal(s1["TYPE"], ref[2]) and np.array_equal(s2["TYPE"], ref[2])
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), "run(1) x n and run(n) differ in " + k


# ---- 1: six directions, every mode, all three list paths, both precisions -------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["t", "c", "b"])
def test_six_directions_and_modes(make_gpu, prec, shape):
    """prob 0.5 on the -x slab, num smaller (2) and larger (10000) than the candidate count, fraction 0.5, all; resets on.
    Corner particles sit in two or three slabs: the first rule that takes one hides it from the later ones."""
    spec = melt(shape, seed=3)
    edge = spec["box"][0]
    modes = [(G.MODE_PROB, 0.5, 0), (G.MODE_NUM, 0.0, 2), (G.MODE_FRACTION, 0.5, 0), (G.MODE_ALL, 0.0, 0), (G.MODE_NUM, 0.0, 10000), (G.MODE_PROB, 0.5, 0)]
    rules = slabs(edge, 0.75, 1, FROZEN, modes)
    nsteps = 12
    g1, g2, pos, ref = stepwise_and_whole(make_gpu, prec, spec, rules, nsteps, reset_velocity=True, reset_force=True)
    assert_agree(g1, g2, ref)
    ch, st, ty = ref
    assert len({c[2] for c in ch}) == 6 and len({c[0] for c in ch}) > 3      # guard: every direction acted, on several steps
    first = G.fold(pos[1], np.array(spec["box"]))
    corner = [t for t in range(spec["n"]) if spec["types"][t] == 1 and sum(G.inside(r, first[t]) for r in rules) >= 2]
    assert corner, "guard: no particle in two slabs"
    assert len(ch) == len({c[1] for c in ch})      # nobody is changed twice: a changed particle no longer has the target type
    # resets: v == 0 exactly, and -- no thermostat, no potential on the new type -- the position stays, bit for bit
    v, x = g2.get_state("VEL"), g2.get_state("POS")
    for s, t, k in ch:
        assert np.all(v[t] == 0.0) and np.array_equal(x[t], pos[s][t])
    moved = [t for t in range(spec["n"]) if ty[t] != FROZEN]
    assert np.all(np.any(v[moved] != 0.0, axis=1))
    if shape == "t":
        firings, syncs = g2.region_counters()
        print("one call: %d firings, %d host synchronisations, %d steps with a change" % (firings, syncs, len({c[0] for c in ch})))
        assert firings == nsteps and syncs == len({c[0] for c in ch})


@pytest.mark.parametrize("prec", [64, 32])
def test_modes_on_a_hundred_candidates(make_gpu, prec):
    """Half the box, about 120 candidates of type 1, four rules one after the other on what the earlier ones leave: prob 0.5,
    num 7 (smaller than the count), fraction 0.25, num 10000 (larger than the count: everybody who is left)."""
    spec = melt("t", seed=17)
    edge = spec["box"][0]
    half = ([0, 0, 0], [4.5, edge, edge])
    rules = [G.rule(*half, 1, 3, mode=G.MODE_PROB, value=0.5, seed=31), G.rule(*half, 1, 4, mode=G.MODE_NUM, num=7, seed=32),
             G.rule(*half, 1, 5, mode=G.MODE_FRACTION, value=0.25, seed=33), G.rule(*half, 1, 6, mode=G.MODE_NUM, num=10000, seed=34, interval=2)]
    g1, g2, pos, ref = stepwise_and_whole(make_gpu, prec, spec, rules, 3)
    assert_agree(g1, g2, ref)
    first = [s for s in ref[1] if s[0] == 1]
    print("step 1: (rule, candidates, changed) =", [s[1:] for s in first])
    c0 = first[0][2]
    assert 90 <= c0 <= 150 and 0.3 * c0 < first[0][3] < 0.7 * c0
    left = c0 - first[0][3]
    assert first[1][1:] == (1, left, 7) and first[2][1:] == (2, left - 7, (left - 7) // 4) and len(first) == 3
    second = [s for s in ref[1] if s[0] == 2 and s[1] == 3]
    assert second and second[0][2] == second[0][3]      # num larger than the count: all of them


# ---- 2: faces, the fold, a corner ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_faces_fold_and_corner(make_gpu, prec):
    """Free flight in a box of 8 (dt v = 1/256 per step, exact in both precisions): A rests exactly on lo (inside), B exactly on
    hi (outside), C leaves through the upper x face and is caught by the -x region at the step its folded coordinate is 0.0,
    D rests in the corner of the -x and the -y region: the first takes it, the second no longer sees the target type."""
    edge, dt = 8.0, 1.0 / 256
    pos = np.array([[1.0, 4.0, 4.0], [2.0, 4.0, 4.0], [8.0 - 2.0 / 256, 4.0, 6.0], [0.25, 0.25, 4.0], [4.0, 4.0, 1.0], [4.0, 5.0, 1.0]])
    vel = np.zeros((6, 3)); vel[2, 0] = 1.0
    types = np.array([1, 1, 1, 1, 0, 0], np.int32)
    spec = dict(n=6, box=[edge] * 3, rc=RC, skin=SKIN, dt=dt, ids=np.arange(1, 7), types=types, pos=pos, vel=vel, mass=np.ones(6),
                state=np.zeros(6, np.int32), kT=0.0, gamma=0.0, seed=1, lj=[(0, 0) + LJ])
    rules = [G.rule([1.0, 3.0, 3.0], [2.0, 5.0, 5.0], 1, FROZEN), G.rule([0, 0, 0], [0.5, edge, edge], 1, 3), G.rule([0, 0, 0], [edge, 0.5, edge], 1, 4)]
    g1, g2, p, ref = stepwise_and_whole(make_gpu, prec, spec, rules, 4, reset_velocity=True, reset_force=True)
    assert_agree(g1, g2, ref)
    assert p[2][2, 0] == 0.0 and p[1][2, 0] == 8.0 - 1.0 / 256      # guard: C's folded coordinate is exactly 0 at step 2
    assert ref[0] == [(1, 0, 0), (1, 3, 1), (2, 2, 1)]
    assert ref[2].tolist() == [FROZEN, 1, 3, 3, 0, 0]


# ---- 3: the partner's stale half kick; a by-types slot ----------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_partner_keeps_a_constant_velocity(make_gpu, prec):
    """P (in the region) and Q (outside) of type 1 attract each other inside the cutoff.  P freezes at step 1; forces are not
    evaluated again there, so Q takes one more half kick from the stored force (v(2) != v(1)), and from the first evaluation
    after the change -- P has no potential any more -- its velocity stays what it is, bit for bit."""
    edge = 9.0
    pos = np.array([[0.5, 4.5, 4.5], [1.25, 4.5, 4.5], [6.0, 6.0, 6.0], [6.0, 7.0, 6.0]])
    types = np.array([1, 1, 0, 0], np.int32)
    spec = dict(n=4, box=[edge] * 3, rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, 5), types=types, pos=pos, vel=np.zeros((4, 3)), mass=np.ones(4),
                state=np.zeros(4, np.int32), kT=0.0, gamma=0.0, seed=1, lj=[(0, 0) + LJ, (1, 1) + LJ])
    rules = [G.rule([0, 0, 0], [0.75, edge, edge], 1, FROZEN)]
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    send_rules(g, rules, reset_velocity=True, reset_force=True)
    v = {}
    for s in range(1, 6):
        g.run(1)
        v[s] = g.get_state("VEL")
        f = g.get_state("FORCE")
        if s == 1:
            assert np.all(f[0] == 0.0) and f[1, 0] != 0.0      # the stored force: reset for P, kept for Q
    assert logs(g)[0] == [(1, 0, 0)]
    assert v[1][1, 0] != 0.0 and v[2][1, 0] != v[1][1, 0]      # the stale half kick
    assert v[2][1, 0] - v[1][1, 0] == pytest.approx(0.5 * v[1][1, 0], rel=1e-3)      # ... of the stored force: half of what the two half kicks of step 1 gave
    for s in (3, 4, 5):
        assert np.array_equal(v[s][1], v[2][1])
    assert np.all(v[5][0] == 0.0)
    # the same in one call
    h = make_gpu(prec)
    W.apply(spec, h, thermostat=False, reactions=False)
    send_rules(h, rules, reset_velocity=True, reset_force=True)
    h.run(5)
    assert np.array_equal(h.get_state("VEL"), v[5]) and np.array_equal(h.get_state("POS"), g.get_state("POS"))


@pytest.mark.parametrize("prec", [64, 32])
def test_by_types_bond_takes_the_slot_of_the_new_type(make_gpu, prec):
    """P - Q bonded in a by-types harmonic list with parameters for (1, 1) and (1, 2); P becomes type 2 at step 1: the force
    of the next evaluation is the (1, 2) slot's (tests/bonded_ref.py)."""
    edge = 9.0
    pos = np.array([[0.5, 4.5, 4.5], [1.5, 4.5, 4.5], [6.0, 6.0, 6.0], [6.0, 7.0, 6.0]])
    types = np.array([1, 1, 0, 0], np.int32)
    spec = dict(n=4, box=[edge] * 3, rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, 5), types=types, pos=pos, vel=np.zeros((4, 3)), mass=np.ones(4),
                state=np.zeros(4, np.int32), kT=0.0, gamma=0.0, seed=1, lj=[(0, 0) + LJ])
    typed = [((1, 1), [30.0, 0.9]), ((1, 2), [7.0, 1.2])]
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    h = g.list_create(2, "HARMONIC", True)
    for key, p in typed:
        g.list_set_params(h, p, types=key)
    g.list_add(h, [(1, 2)])
    send_rules(g, [G.rule([0, 0, 0], [0.75, edge, edge], 1, FROZEN)])
    lst = [dict(kind="HARMONIC", arity=2, ids=[1, 2], typed=typed)]
    g.run(1)
    assert g.get_state("TYPE").tolist() == [FROZEN, 1, 0, 0]
    x, f = g.get_state("POS"), g.get_state("FORCE")
    old = B.reference(x, spec["box"], types, lst)["force"]
    assert np.abs(f[:2] - old[:2]).max() <= (1e-10 if prec == 64 else 1e-4) * np.abs(old).max()      # step 1: still the (1, 1) slot
    g.run(1)
    x, f = g.get_state("POS"), g.get_state("FORCE")
    new = B.reference(x, spec["box"], g.get_state("TYPE"), lst)["force"]
    wrong = B.reference(x, spec["box"], types, lst)["force"]
    err = np.abs(f[:2] - new[:2]).max() / np.abs(new).max()
    print("prec %d: bond force against the (1, 2) slot %.3e, the (1, 1) slot is %.3e away" % (prec, err, np.abs(wrong - new).max() / np.abs(new).max()))
    assert err <= (1e-10 if prec == 64 else 1e-4) and np.abs(wrong - new).max() > 0.1 * np.abs(new).max()


# ---- 4: lambda stamp, thermal groups -------------------------------------------------------------------------------------------

def test_a_type_with_a_rate_is_restamped(make_gpu):
    spec = melt("c", seed=5)
    edge, alpha = spec["box"][0], 0.01
    rules = [G.rule([0, 0, 0], [0.75, edge, edge], 1, FROZEN, interval=3)]
    g = make_gpu(64)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.resolution_rate(FROZEN, alpha)
    g.set_resolution(spec["ids"], 0.5)
    send_rules(g, rules)
    g.run(7)
    ch = logs(g)[0]
    assert ch and {c[0] for c in ch} <= {3, 6}
    lam = g.get_state("LAMBDA")
    want = np.full(spec["n"], 0.5)
    for s, t, k in ch:
        want[t] = min(1.0, 0.5 + alpha * float(7 - s))
    assert np.array_equal(lam, want)


@pytest.mark.parametrize("prec", [64, 32])
def test_langevin_leaves_the_frozen_type_alone(make_gpu, prec):
    """Langevin on types 0 and 1 only (a run in pieces draws other noise at the start of a piece than a run in one call, so
    the two are not compared here): the logs against the reference on the stepped engine's own positions, and on both engines
    every frozen particle rests where it was caught, while the thermostat does move the others."""
    spec = dict(melt("t", seed=7), gamma=1.0, kT=1.0, thermal_types=[0, 1])
    edge = spec["box"][0]
    rules = slabs(edge, 0.75, 1, FROZEN, [(G.MODE_ALL, 0.0, 0)])
    g1, g2, pos, ref = stepwise_and_whole(make_gpu, prec, spec, rules, 8, reset_velocity=True, reset_force=True)
    ch, st = logs(g1)
    assert ch == ref[0] and st == ref[1] and len(ch) > 20
    x, v = g1.get_state("POS"), g1.get_state("VEL")
    for s, t, k in ch:
        assert np.array_equal(x[t], pos[s][t]) and np.all(v[t] == 0.0)
    ch2 = logs(g2)[0]
    assert len(ch2) > 20
    x2 = g2.get_state("POS")
    g2.run(4)
    v2, x3, ty2 = g2.get_state("VEL"), g2.get_state("POS"), g2.get_state("TYPE")
    for s, t, k in ch2:
        assert np.all(v2[t] == 0.0) and np.array_equal(x2[t], x3[t]) and ty2[t] == FROZEN
    assert np.all(np.any(x3[ty2 != FROZEN] != x2[ty2 != FROZEN], axis=1))


# ---- 5: interval, a rule enabled in the middle of a run, the whole-box rule by count ----------------------------------------------

@pytest.mark.parametrize("shape", ["t", "c"])
def test_interval_and_late_enable(make_gpu, shape):
    spec = melt(shape, seed=9)
    edge = spec["box"][0]
    rules = [G.rule([0, 0, 0], [edge, edge, edge], 1, 0, interval=3, mode=G.MODE_NUM, num=5, seed=77),      # ChangeParticleType's rule
             G.rule([0, 0, 0], [1.5, edge, edge], 0, FROZEN, interval=2, mode=G.MODE_PROB, value=0.25, seed=78)]
    g1, g2 = make_gpu(64), make_gpu(64)
    for g in (g1, g2):
        W.apply(spec, g, thermostat=False, reactions=False)
        send_rules(g, rules, enable=False)
        g.region_enable(0)
    pos = {}
    for s in range(1, 5):
        g1.run(1); pos[s] = g1.get_state("POS")
    g2.run(4)
    early = G.run(rules[:1], pos, spec["types"], np.array(spec["box"]))
    assert logs(g1)[0] == early[0] == logs(g2)[0] and [c[0] for c in early[0]] == [3] * 5
    for g in (g1, g2):
        g.region_enable(1)
    pos2 = {}
    for s in range(5, 13):
        g1.run(1); pos2[s] = g1.get_state("POS")
    g2.run(8)
    late = G.run(rules, pos2, early[2], np.array(spec["box"]))
    ref = (early[0] + late[0], early[1] + late[1], late[2])
    assert_agree(g1, g2, ref)
    assert {c[0] for c in late[0] if c[2] == 0} == {6, 9, 12} and {c[0] for c in late[0] if c[2] == 1} <= {6, 8, 10, 12} and any(c[2] == 1 for c in late[0])
    g2.region_enable(0, False); g2.region_enable(1, False)
    n = len(logs(g2)[0])
    g2.run(6)
    assert len(logs(g2)[0]) == n


# ---- 6: no synchronisation on empty firings; counters of a context without rules -----------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_empty_firings_do_not_synchronise(make_gpu, prec):
    """200 steps of the tile-path melt of type 0 with six slabs that wait for type 1: the only particles of type 1 rest in the
    middle of the box, out of everybody's cutoff.  200 firings, no host synchronisation, nothing changed -- and the trajectory is
    the one of a context without rules."""
    spec = melt("t", seed=11, kT=1.0, types=0)
    mid = [i for i in range(spec["n"]) if np.all(np.abs(spec["pos"][i] - 4.5) < 0.6)]
    assert mid
    keep = [i for i in range(spec["n"]) if i in mid[:1] or np.linalg.norm(spec["pos"][i] - spec["pos"][mid[0]]) > 2.0]
    spec = dict(spec, n=len(keep), ids=np.arange(1, len(keep) + 1), types=spec["types"][keep].copy(), pos=spec["pos"][keep], vel=spec["vel"][keep],
                mass=spec["mass"][keep], state=spec["state"][keep], lj=[(0, 0) + LJ])
    k1 = keep.index(mid[0])
    spec["types"][k1] = 1; spec["vel"][k1] = 0.0
    rules = slabs(9.0, 0.75, 1, FROZEN, [(G.MODE_PROB, 0.5, 0), (G.MODE_NUM, 0.0, 3), (G.MODE_FRACTION, 0.5, 0), (G.MODE_ALL, 0.0, 0)])
    g, plain = make_gpu(prec), make_gpu(prec)
    for e in (g, plain):
        W.apply(spec, e, thermostat=False, reactions=False)
    assert plain.region_counters() == (0, 0)
    send_rules(g, rules)
    g.run(200); plain.run(200)
    firings, syncs = g.region_counters()
    print("prec %d: %d firings, %d host synchronisations" % (prec, firings, syncs))
    assert (firings, syncs) == (200, 0)
    assert len(g.region_changes()) == 0 and len(g.region_stats()) == 0 and plain.region_counters() == (0, 0)
    for k in ("POS", "VEL", "TYPE"):
        assert np.array_equal(g.get_state(k), plain.get_state(k))


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu):
    g = make_gpu(64)
    W.apply(melt("c", seed=1), g, thermostat=False, reactions=False)
    good = dict(lo=[0, 0, 0], hi=[1, 1, 1], target_type=1, new_type=2)
    bad = [dict(target_type=-1), dict(target_type=_capi.CHEM_MAX_TYPES), dict(new_type=_capi.CHEM_MAX_TYPES), dict(new_type=-1),
           dict(lo=[2, 0, 0]), dict(hi=[1, float("inf"), 1]), dict(lo=[float("nan"), 0, 0]), dict(interval=0),
           dict(mode="prob", value=1.5), dict(mode="prob", value=-0.1), dict(mode="fraction", value=1.01), dict(mode="num", num=-1), dict(mode=4)]
    for b in bad:
        with pytest.raises(ChemError) as ei:
            g.region_add(**dict(good, **b))
        assert ei.value.code == _capi.EINVAL, b
    with pytest.raises(ChemError) as ei:
        g.region_enable(0)
    assert ei.value.code == _capi.EINVAL
    assert g.region_add(**good) == 0
    with pytest.raises(ChemError) as ei:
        g.comm_init_local(2, 0, 991)
    assert ei.value.code == _capi.ENOTIMPL
    h = make_gpu(64)
    W.apply(melt("t", seed=1), h, thermostat=False, reactions=False)
    h.comm_init_local(1, 0, 992)
    with pytest.raises(ChemError) as ei:
        h.region_add(**good)
    assert ei.value.code == _capi.ENOTIMPL


# ---- 8: checkpoint between two firings ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_checkpoint_between_two_firings(make_gpu, prec):
    spec = melt("t", seed=13)
    edge = spec["box"][0]
    rules = slabs(edge, 0.75, 1, FROZEN, [(G.MODE_PROB, 0.3, 0), (G.MODE_NUM, 0.0, 2)], interval=3)
    a, b = make_gpu(prec), make_gpu(prec)
    for g in (a, b):
        W.apply(spec, g, thermostat=False, reactions=False)
        send_rules(g, rules, reset_velocity=True, reset_force=True)
    a.run(4)
    n0 = len(logs(a)[0])
    assert n0 > 0
    b.checkpoint_load(a.checkpoint_save())
    assert len(b.region_changes()) == 0
    a.run(6); b.run(6)
    cha, chb = logs(a)[0], logs(b)[0]
    assert cha[n0:] == chb and len(chb) > 0      # (after a load the log holds what happened since)
    sa, sb = state_of(a), state_of(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
