"""Two conventions every other device test shares with the engine, taken away: particle ids that are not 1 .. N handed over in
ascending order, and scenes built in one orientation only.  Helpers: tests/invariance.py; scenes, protocols and the CPU side
(the helpers are involutions, the references and the oracle agree with them): tests/test_invariance_ref.py.

A. Names.   Three scenes (test_invariance_ref.bonded_scene, reactive_scene, resfix_scene), each entry point that takes or gives
            ids in one of them, and each scene's result differs from the run without that entry point (asserted).
  A1        ids 7 + cumsum(integers(1, 9)) -- the same ORDER, so the same tags -- with the rows shuffled: the device sees the
            input of the 1 .. N run and must return its bits: POS, VEL, FORCE, IMAGE, TYPE, STATE, RESID, MASS, CHARGE, LAMBDA,
            observe(), pressure and tensor, list sizes, rebuild counters, ATRP and region stats; events (every field, r2 to the
            bit), exclusions, Verlet pairs, list entries, fix sets, fix / join / removal logs and region changes after mapping
            the names back.  On the tile path, the per-cell list, the brute-force list, one slab that is its own neighbour, two
            and three slabs, in both precisions (fix sets, add_particles, checkpoints, dissociation and region rules: single
            domain, which is where the engine serves them).  A checkpoint of a renamed context restarts a renamed context bit
            for bit.  One fp64 run carries ids above 2^33.
  A2        the names reversed: every tag changes, so random streams and summation orders change; forces and energies at
            run(0) within 1e-12 of the largest force in fp64 (fewer than 100 terms per particle in another order) and
            TOL_MELT32 through helpers.force_error_without_cutoff_flips in fp32; 20 NVE steps within the project's trajectory
            tolerance (1e-9 / 2e-4); one rate-1e9, nearest, frozen reaction step of react_ref.chain (no two candidates share a
            distance: asserted on the CPU) gives the same pairs with r2 to the bit.
  refusals  an id inside a gap, given to every entry point that takes ids: CHEM_EINVAL on the host, seen by pytest.raises
            before any launch, and the context then runs exactly as a twin that never made the calls.
B. Orientation.  Both cyclic permutations of the axes and the reflection of each axis:
            the reaction zoo against react_ref on the turned scene (events with r2 to the bit, bonds, states, labels);
            aged_ref's closing pairs from rc + 0.99 skin, forces at the oldest-list step against exact_pairs at the engine's own
            positions with the tolerances of tests/test_gpu_aged_lists.py -- the slabs now cut what used to be x and y;
            an anisotropic melt of 5 x 6 x 7 cells (LJ, two tables, a bonded list): the pressure tensor part by part against
            ptensor_ref with the tolerances of tests/test_gpu_ptensor.py, and the orientations against each other through
            the component map.  No pair of any scene lies in the shell of its cutoff in any orientation (asserted on the CPU
            at the start positions and here at the engine's): fp32 is allowed no cutoff flip.

Findings this module was written against (fixed in chemlab_amd/csrc/chem_api.hip, kept as tests here):
  - chem_set_exclusions, chem_list_add and chem_reaction_restrict resolved ids while they changed the context: a call refused
    for its second id had already dropped the old exclusions / inserted the first entry without its graph edge.
  - the default res_id and CHEM_STATE_MOLID narrowed an id to int32 without a word; both now refuse ids beyond 32 bits by name.

Measured on an MI355X (the worst figure over paths and orientations; every test prints its own):
  A1   bit identity in every case: 26 to 29 arrays and records per rank; the reactive scene logs 2800 to 2900 events in 60 steps.
  A2   forces under reversed names: fp64 1.5e-16 of the largest force (bound 1e-12), fp32 8.2e-8 (TOL_MELT32 = 2e-5), no cutoff
       flip (one pair of the 216-particle box lies in the shell; it was decided the same way); 20 NVE steps: fp64 2.1e-16
       (1e-9), fp32 2.4e-6 (2e-4).  The reaction step: the same pairs, r2 to the bit, on every path.
  B    zoo: all 24 members (4 on the brute-force list) equal their reference in every orientation, path and precision.
       closing pairs at the oldest list: fp64 1.4e-14 (1e-10), fp32 1.2e-6 (2e-5), no pair in a shell.
       melt tensor, err / scale: fp64 kinetic 2.2e-15, non-bonded 7.4e-15, list 1.6e-15 (1e-10); fp32 kinetic 2.7e-15, non-bonded
       4.6e-8, list 2.2e-15 (2e-5); orientations against each other 2.1e-15 / 3.9e-8; two components of the non-bonded virial
       are at least 44 fp32 tolerances apart."""
import numpy as np
import pytest

import aged_ref as AR
import helpers as H
import invariance as I
import ptensor_ref as PT
import react_ref as RR
import test_invariance_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from test_gpu_aged_lists import _compare as aged_compare, _snapshot as aged_snapshot
from test_gpu_parity import TOL_MELT32, _run_ranks
from test_gpu_ptensor import check as tensor_check
from test_gpu_pressure import TOL as TOL_VIRIAL
from test_react_ref import _run_engine

pytestmark = pytest.mark.gpu

PATHS = {"tiles": (1, {}), "cells": (1, {"tiles": 0}), "brute": (1, {}), "dd_self": (1, {"dd_self": 1}), "P2": (2, {}), "P3": (3, {})}
SINGLE = ("tiles", "cells", "brute")
HOWS = [h for h, _ in I.ORIENTATIONS if h != "id"]
_OWN_HUB = [1 << 20]


def on_path(make_gpu, prec, path, body):
    """body(engine) on every rank of `path`; the ranks' results"""
    P, opts = PATHS[path]
    engs = [make_gpu(prec) for _ in range(P)]
    _OWN_HUB[0] += 1            # (ids of this module's own, far from the session counter of test_gpu_parity: other modules name fixed ids near it)
    hub = _OWN_HUB[0]

    def rank(r):
        g = engs[r]
        for k in sorted(opts, key=lambda k: k != "dd_self"):
            g.set_option(k, opts[k])
        if P > 1:
            g.comm_init_local(P, r, hub)
        return body(g)
    return _run_ranks(P, rank) if P > 1 else [rank(0)]


def scene(name, path):
    if name == "bonded":
        return S.bonded_scene("brute" if path == "brute" else "tiles")
    if name == "reactive":
        return S.reactive_scene(single_domain=path in SINGLE, n=256 if path == "brute" else 4000)
    return S.resfix_scene()


# ======================================================================================================================
# A1: the same order of names, shuffled rows
# ======================================================================================================================
def _a1(make_gpu, name, path, prec, renamed=None):
    spec = scene(name, path)
    ren, m = S.gapped(spec) if renamed is None else renamed(spec)
    assert m.keeps_order() and not np.array_equal(ren["ids"], np.sort(ren["ids"]))
    a = on_path(make_gpu, prec, path, lambda g: S.run_scene(g, spec))
    b = on_path(make_gpu, prec, path, lambda g: S.run_scene(g, ren))
    for r, ((a0, a1), (b0, b1)) in enumerate(zip(a, b)):
        S.same_under_names(a0, b0, m, "%s %s fp%d rank %d, first:" % (name, path, prec, r))
        S.same_under_names(a1, b1, m, "%s %s fp%d rank %d, last:" % (name, path, prec, r))
    a0, a1 = a[0]
    assert a1["step"] == sum(spec["run"]) and not np.array_equal(a1["POS"], a0["POS"]) and np.abs(a0["FORCE"]).max() > 0
    print("%s %s fp%d: bit identity in %d arrays and records on %d rank(s); %d events, %d excluded pairs, %d list pairs, counters %s" % (
        name, path, prec, len(a1), len(a), len(a1["events"]), len(a1["exclusions"]), len(a1["verlet"]), a1["counters"]))
    return spec, a, b


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
def test_bonded_melt_same_bits_under_new_names(make_gpu, path, prec):
    spec, a, _ = _a1(make_gpu, "bonded", path, prec)
    a0, a1 = a[0]
    assert all(len(a1["list %d" % i]) == len(l["ids"]) > 0 for i, l in enumerate(spec["lists"])) and len(a1["exclusions"]) == len(spec["exclusions"])
    assert not np.array_equal(a1["TYPE"], a0["TYPE"]) and not np.array_equal(a1["MASS"], a0["MASS"])      # modify_particle went in between


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
def test_reactive_melt_same_bits_under_new_names(make_gpu, path, prec):
    spec, a, _ = _a1(make_gpu, "reactive", path, prec)
    a1 = a[0][1]
    assert len(a1["events"]) > (50 if path != "brute" else 0) and len(a1["atrp"]) == 60 // 7
    if path != "brute":
        assert len(a1["list 0"]) > 0 and (a1["TYPE"] == S.E_).any()                       # spawned angles, a neighbour change
    if path in SINGLE:
        assert len(a1["region_changes"]) > 0


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ["tiles", "cells"])
def test_resolution_and_fixed_distances_same_bits_under_new_names(make_gpu, path, prec):
    spec, a, _ = _a1(make_gpu, "resfix", path, prec)
    a1 = a[0][1]
    lam = a1["LAMBDA"]
    assert len(a1["fix_log"]) > 0 and ((lam > 0) & (lam < 1)).sum() >= 40 and len(a1["ID"]) == spec["n"] + 8 and a1["ID"][-1] > spec["n"] + 8


@pytest.mark.parametrize("prec", [64, 32])
def test_checkpoint_of_a_renamed_context_restarts_a_renamed_context(make_gpu, prec):
    ren, m = S.gapped(S.resfix_scene())
    ga, gb = make_gpu(prec), make_gpu(prec)
    ha = S.apply_scene(ren, ga)
    ga.run(33)
    blob = ga.checkpoint_save()
    hb = S.apply_scene(dict(ren, vel=np.zeros_like(ren["vel"])), gb)
    gb.checkpoint_load(blob)
    assert gb.checkpoint_save() == blob
    ga.run(20)
    gb.run(20)
    a, b = S.collect(ga, ha), S.collect(gb, hb)
    a.pop("counters"), b.pop("counters")                  # (counters of a context's lifetime: not part of the saved state)
    S.same_under_names(a, b, I.IdMap(a["ID"], a["ID"]), "restart fp%d:" % prec)
    assert a["step"] == 53 and len(a["events"]) > 0 and a["events"]["id_a"].max() > ren["n"] and a["events"]["step"].max() > 33
    # and the blob of the 1 .. N context is refused by name: other ids
    gc = make_gpu(prec)
    S.apply_scene(S.resfix_scene(), gc)
    with pytest.raises(ChemError, match="the particle ids differ") as e:
        gc.checkpoint_load(blob)
    assert e.value.code == _capi.EINVAL


def test_ids_beyond_32_bits(make_gpu):
    """Every read-back carries ids as int64; the two int32 labels made of ids refuse such ids by name (include/chem_mi355.h,
    chem_set_particles)."""
    big = lambda spec: I.relabel(spec, 2 ** 33 + I.gapped_ids(len(I.all_ids(spec)), 2), np.random.default_rng(1).permutation(len(spec["ids"])))      # noqa: E731
    spec, a, b = _a1(make_gpu, "resfix", "tiles", 64, renamed=big)
    b1 = b[0][1]
    for k in ("events", "fix_log"):
        assert len(b1[k]) > 0 and all(b1[k][f].min() > 2 ** 33 for f in S.ID_FIELDS[k]), k
    assert b1["exclusions"].min() > 2 ** 33 and b1["verlet"].min() > 2 ** 33 and b1["fix 0"][0].min() > 2 ** 33 and b1["list reaction_bonds"].min() > 2 ** 33
    g = make_gpu(64)
    ren, m = big(scene("bonded", "brute"))
    with pytest.raises(ChemError, match="default res_id is the particle id") as e:
        S.apply_scene(dict(ren, res_id=None), g)
    assert e.value.code == _capi.EINVAL
    S.apply_scene(ren, g)
    top = int(ren["ids"].max())
    with pytest.raises(ChemError, match="default res_id is the particle id") as e:
        g.add_particles([top + 5], [0], [[1.0, 1.0, 1.0]], [1.0])
    assert e.value.code == _capi.EINVAL
    g.run(3)
    with pytest.raises(ChemError, match="CHEM_STATE_MOLID is an int32 read-back") as e:
        g.get_state("MOLID")
    assert e.value.code == _capi.EINVAL
    twin = make_gpu(64)
    S.apply_scene(ren, twin)
    twin.run(3)
    assert np.array_equal(g.get_state("POS"), twin.get_state("POS")) and g.n == ren["n"]
    # ids that fit keep both labels: the default res_id is the id, MOLID the lowest id of the cluster
    small, ms = S.gapped(scene("bonded", "brute"))
    gs = make_gpu(64)
    S.apply_scene(dict(small, res_id=None), gs)
    gs.run(0)
    assert np.array_equal(gs.get_state("RESID"), np.sort(small["ids"]))
    mol = gs.get_state("MOLID")
    chains = ms.fwd(np.arange(1, small["n"] + 1).reshape(-1, 6))
    assert np.array_equal(mol, np.repeat(chains.min(1), 6))


@pytest.mark.parametrize("name", ["bonded", "reactive", "resfix"])
def test_every_entry_point_matters(make_gpu, name):
    spec = scene(name, "tiles")
    full = S.run_scene(make_gpu(64), spec)[1]
    for what in S.ENTRY_POINTS[name]:
        assert S.differs(full, S.run_scene(make_gpu(64), S.without(spec, what))[1]), (name, what)


# ======================================================================================================================
# refusals
# ======================================================================================================================
def test_an_id_inside_a_gap_is_refused_everywhere_and_leaves_no_trace(make_gpu):
    spec, m = S.gapped(S.resfix_scene())
    ids = np.sort(I.all_ids(spec))
    k = int(np.nonzero(np.diff(ids[:spec["n"]]) > 1)[0][7])
    bad, top = int(ids[k] + 1), int(ids[-1])
    assert bad not in set(ids.tolist())
    isA = np.sort(spec["ids"][spec["types"] == S.A_])
    free = [int(i) for i in isA if i not in set(np.concatenate([f["pairs"].ravel() for f in spec["fix"]]).tolist())]
    g1, g2, g3, g4 = free[10], free[11], free[12], free[13]

    def setup():
        g = make_gpu(64)
        h = S.apply_scene(spec, g)
        h["l2"], h["l4"] = g.list_create(2, "HARMONIC", False), g.list_create(4, "DIH_NCOS", False)
        g.list_set_params(h["l2"], [30.0, 1.0])
        g.list_set_params(h["l4"], [0.5, 0.3, 3.0])
        return g, h
    g, h = setup()
    twin, ht = setup()
    calls = {
        "set_exclusions": lambda: g.set_exclusions([[g1, g2], [g3, bad]]),
        "list_add arity 2": lambda: g.list_add(h["l2"], [[g1, g2], [bad, g3]]),
        "list_add arity 3": lambda: g.list_add(h[0], [[g1, g2, g3], [g1, bad, g3]]),
        "list_add arity 4": lambda: g.list_add(h["l4"], [[g1, g2, g3, g4], [g1, g2, g3, bad]]),
        "modify_particle": lambda: g.modify_particle(bad, "TYPE", 1),
        "modify_particle lambda": lambda: g.modify_particle(bad, "LAMBDA", 0.5),
        "set_resolution": lambda: g.set_resolution([g1, bad], [0.5, 0.5]),
        "fix_add target": lambda: g.fix_add(h["fix"][0], [[g1, g2], [g3, bad]], 1.0),
        "fix_add anchor": lambda: g.fix_add(h["fix"][0], [[bad, g4]], 1.0),
        "reaction_restrict": lambda: g.reaction_restrict(1, [[g1, g2], [g1, bad]]),
        "add_particles": lambda: g.add_particles([bad], [S.E_], [[1.0, 1.0, 1.0]], [1.0], res_id=[1]),
        "set_exclusions below": lambda: g.set_exclusions([[g1, int(ids[0]) - 1]]),
        "list_add above": lambda: g.list_add(h["l2"], [[g1, top + 1]]),
    }
    for what, call in calls.items():                 # (a missing refusal fails here, before any launch)
        with pytest.raises(ChemError) as e:
            call()
        assert e.value.code == _capi.EINVAL, (what, str(e.value))
    g.run(25)
    twin.run(25)
    a, b = S.collect(g, h), S.collect(twin, ht)
    S.same_under_names(a, b, I.IdMap(a["ID"], a["ID"]), "after the refusals:")
    assert len(a["list l2"]) == 0 and len(a["list l4"]) == 0 and len(a["exclusions"]) >= len(spec["exclusions"]) and len(a["events"]) > 0


# ======================================================================================================================
# A2: the names reversed
# ======================================================================================================================
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
def test_reversed_names_same_forces_and_trajectory(make_gpu, path, prec):
    spec = dict(scene("bonded", path), run=(0, 20))
    spec.pop("modify")
    ren, m = S.reversed_names(spec)
    assert not m.keeps_order()
    shell = AR.exact_pairs(spec, spec["pos"])["shell_pairs"]
    a = on_path(make_gpu, prec, path, lambda g: S.run_scene(g, spec, thermostat=False))[0]
    b = on_path(make_gpu, prec, path, lambda g: S.run_scene(g, ren, thermostat=False))[0]
    back = np.argsort(m.inv(b[0]["ID"]))
    assert np.array_equal(m.inv(b[0]["ID"])[back], a[0]["ID"]) and not np.array_equal(back, np.arange(len(back)))
    fa, fb = a[0]["FORCE"], b[0]["FORCE"][back]
    fmax = np.abs(fa).max()
    if prec == 64:
        err, flips = np.abs(fb - fa).max() / fmax, 0
        assert err <= 1e-12, err
    else:
        err, flips = H.force_error_without_cutoff_flips(dict(spec, pos=a[0]["POS"]), fb, fa, TOL_MELT32, max_flips=shell)
        assert err < TOL_MELT32 and 0 <= flips <= shell, (err, flips, shell)
    oa, ob = a[0]["observe"], b[0]["observe"]
    etol = 1e-12 if prec == 64 else 2e-5
    sc = H.energy_scales(dict(spec, pos=a[0]["POS"]))
    assert abs(oa["epot_lj"] - ob["epot_lj"]) <= etol * sc["epot_lj"][0] + sc["epot_lj"][1] * (prec == 32)
    assert np.allclose(oa["epot_list"], ob["epot_list"], rtol=etol, atol=etol * max(np.abs(oa["epot_list"])))
    assert oa["ekin"] == pytest.approx(ob["ekin"], rel=etol) and oa["list_size"] == ob["list_size"]
    assert np.array_equal(H.canonical_pairs(m.inv(b[0]["exclusions"])), H.canonical_pairs(a[0]["exclusions"]))
    if prec == 64:
        assert np.array_equal(H.canonical_pairs(m.inv(b[0]["verlet"])), H.canonical_pairs(a[0]["verlet"]))
    terr = rel_err(b[1]["POS_UNFOLDED"][back], a[1]["POS_UNFOLDED"])
    assert terr < (1e-9 if prec == 64 else 2e-4), terr
    assert not np.array_equal(a[1]["POS"], a[0]["POS"])
    print("reversed names %s fp%d: force error %.2e of the largest (%d flips of %d shell pairs), 20 NVE steps %.2e" % (path, prec, err, flips, shell, terr))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ["tiles", "cells", "dd_self", "P2", "P3"])
def test_reversed_names_same_reaction_step(make_gpu, path, prec):
    spec, ren, m = S.reversed_chain()
    ref = RR.member("chain")[1]
    want = S.unordered_events([e for step in ref for e in step[0]])

    def body(g):
        got = _run_engine(g, ren)
        return g.get_events(), got[-1][1]
    for ev, snap in on_path(make_gpu, prec, path, body):
        got = S.unordered_events([(e["step"], e["id_a"], e["id_b"], e["reaction"], e["r2"]) for e in ev], m)
        assert got == want and len(want) > 50
        assert np.array_equal(snap["state"][::-1], ref[-1][2]["state"])
        assert np.array_equal(H.canonical_pairs(m.inv(snap["bonds"])), H.canonical_pairs(ref[-1][2]["bonds"]))


# ======================================================================================================================
# B: orientation
# ======================================================================================================================
ZOO_PATHS = ["tiles", "cells", "dd_self", "P2", "P3"]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ZOO_PATHS + ["brute"])
@pytest.mark.parametrize("how", HOWS)
def test_reaction_zoo_in_every_orientation(make_gpu, how, path, prec):
    """Every member of react_ref's zoo (the 4^3 members on the brute-force list) turned into orientation `how`: events with r2 to
    the bit, pad, bonds, spawned lists, STATE, TYPE, MASS, CHARGE, MOLID, RESID, exclusions and ATRP rows after every step against
    the reference run on the turned scene."""
    names = S.ZOO_BRUTE if path == "brute" else list(RR.ZOO)
    for name in names:
        spec, _ = S.oriented_member(name, how)

        def body(g):
            try:
                return _run_engine(g, spec)
            finally:
                g.close()
        for got in on_path(make_gpu, prec, path, body):
            S.against_oriented_reference(name, how, got)
    print("zoo %s %s fp%d: %d members equal their reference" % (how, path, prec, len(names)))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("how", HOWS)
def test_closing_pairs_in_every_orientation(make_gpu, how, path, prec):
    """aged_ref.tight_closing_pairs (the flat box on the brute-force list) turned: pairs rc + 0.99 skin apart when the list was
    built are inside rc ten steps later, no list build in between, and the forces hold every one of them."""
    spec, am = I.orient(S.tight_probes(flat=path == "brute"), how)
    M, cl, se = spec["M"], spec["closing"], spec["skin_eff"]

    def body(g):
        W.apply(spec, g, thermostat=False)
        g.run(0)
        out = [aged_snapshot(g)]
        for k in (M, 1):
            g.run(k)
            out.append(aged_snapshot(g))
        return out
    res = on_path(make_gpu, prec, path, body)
    for r in res[1:]:
        for u, w in zip(r, res[0]):
            assert all(np.array_equal(u[k], w[k]) for k in ("x", "v", "f"))
    s0, s1, s2 = res[0]
    assert s1["lreb"] == s0["lreb"] and s1["reb"] == s0["reb"]                        # the list of step 0 serves the M-th step
    r0, r1 = AR.pair_separations(spec, s0["xf"]), AR.pair_separations(spec, s1["xf"])
    assert r0[cl].min() > spec["rc"] + 0.98 * se and r1[cl].max() < spec["rc"] - 1e-4, (r0[cl].min(), r1[cl].max())
    part = np.repeat(cl, 2)
    errs = []
    for k, s in ((M, s1), (M + 1, s2)):
        errs.append(aged_compare(spec, s, prec, (how, path, prec, k))[0])
        ref = AR.exact_pairs(spec, s["xf"])
        assert ref["shell_pairs"] == 0
        assert np.abs(s["f"][part]).max(1).min() > 0.5 and np.abs(ref["f"][part]).max(1).min() > 0.5
    assert s2["lreb"] >= s1["lreb"] + 1
    print("closing pairs %s %s fp%d: force error at the oldest list %.2e, behind the rebuild %.2e" % (how, path, prec, *errs))


MELT_PATHS = ["tiles", "cells", "dd_self", "P2", "P3"]


def _melt_hows(path):
    """orientations of the 5 x 6 x 7 melt a path can run: three slabs need six cell layers along z"""
    hows = [h for h, _ in I.ORIENTATIONS]
    if path == "P3":
        base = S.aniso_melt()
        hows = [h for h in hows if np.floor(I.orient(base, h)[0]["box"][2] / (base["rc"] + base["skin"])) >= 6]
    return hows


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", MELT_PATHS)
def test_anisotropic_melt_tensor_in_every_orientation(make_gpu, path, prec):
    base = S.aniso_melt()
    hows = _melt_hows(path)
    assert len(hows) >= 5 and "id" in hows
    tol, seen = TOL_VIRIAL[prec], {}
    for how in hows:
        spec, am = I.orient(base, how)

        def body(g):
            W.apply(spec, g, thermostat=False, reactions=False)
            g.run(0)
            return g.pressure_tensor(), g.pressure(), g.get_state("POS"), g.get_state("VEL")
        out = on_path(make_gpu, prec, path, body)
        for r, (t, p, x, v) in enumerate(out):
            assert AR.exact_pairs(spec, x)["shell_pairs"] == 0                     # no pair that fp32 may decide the other way: no slack
            ref = PT.pressure_tensor(spec, x, v, lists=spec["lists"])
            assert ref["virial_nb_scale"].min() > 0 and ref["virial_list_scale"].min() > 0
            tensor_check(t, p, ref, prec, "melt %s %s rank %d" % (how, path, r), names=["harm"])
            assert all(np.array_equal(t[k], out[0][0][k]) for k in ("kinetic", "virial_nb", "virial_list", "virial", "tensor"))
        seen[how] = (am, out[0][0], ref)
    _, t0, ref0 = seen["id"]
    worst = 0.0
    for how, (am, t, _) in seen.items():
        for k, sc in (("kinetic", ref0["kinetic_scale"]), ("virial_nb", ref0["virial_nb_scale"]), ("virial_list", ref0["virial_list_scale"]), ("virial", ref0["scale"] - ref0["kinetic_scale"])):
            err = np.abs(am.back_tensor6(t[k]) - t0[k]) / sc
            worst = max(worst, float(err.max()))
            assert np.all(err <= tol), (how, k, err)
    v, s = ref0["virial_nb"], ref0["virial_nb_scale"]
    gap = min(abs(v[a] - v[b]) / (tol * max(s[a], s[b])) for a in range(6) for b in range(a + 1, 6))
    assert gap > 10.0, gap                                                          # any two components swapped would miss by more than ten tolerances
    print("melt %s fp%d: %d orientations agree through the component map within %.1e of the scale (two components are at least %.0f tolerances apart)" % (
        path, prec, len(seen), worst, gap))
