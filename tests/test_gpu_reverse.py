"""Reverse reactions on the device (include/chem_mi355.h, chem_reaction_remove_bond / chem_reaction_join) against
tests/reverse_ref.py (react_ref's events, the removal and join rules, fixdist_ref's sets and constraint) and
helpers.pair_reference (forces).

Systems: frozen units on a lattice of spacing rc + skin = 1.8 in the boxes "a" (9.0^3: five cells per axis, the least the
tile path takes; 125 units) and "c" (5.4^3: the per-cell path; 27 units) of tests/test_gpu_spline_tables.py, coordinates
snapped to what both precisions represent exactly.  A unit is an ester group Cp - E (bond 0.5), in every third unit
continued by a second C (Cp - E - C2), with a water W within the reaction cutoff 0.5 of Cp in two units of three: on the
+x side, across a face (the units of the first lattice plane), across a corner (the first unit), or exactly ON Cp (unit
(1, 1, 1)).  Units are 1.8 apart and every pair potential ends at 1.0, so only particles of one unit ever interact, and every
Cp has at most one W in reach: the events need no draw."""
import numpy as np
import pytest

import fixdist_ref as FX
import react_ref as RR
import reverse_ref as RV
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import force_error_without_cutoff_flips, pair_eval, pair_params, pair_reference
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks
from test_gpu_spline_tables import BOXES

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_MELT32}          # the force tolerances of tests/test_gpu_capped.py and test_gpu_dissociation.py
A, B, C, E, WAT, D, Z = 0, 1, 2, 3, 4, 5, 6
SPACING, CUT = 1.8, 0.5
LJ = [(A, Z, 1.0, 0.5, 1.0), (Z, C, 1.0, 0.45, 1.0)]
MASS = {t: 1.0 + 0.5 * t for t in range(16)}     # react_ref._spec's type_mass


def units(shape, water=True):
    """positions, types, the bonds of list 0 (every bond) and list 1 (Cp - E of the short units once more, reversed), and
    per unit a dict of particle indices (cp, e, c2 or None, w or None)"""
    box = np.array(BOXES[shape])
    k = int(round(box[0] / SPACING))
    pos, types, l0, l1, us = [], [], [], [], []

    def put(x, t):
        pos.append(x); types.append(t)
        return len(pos) - 1
    for c in np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3):
        base = 0.125 + SPACING * c
        v = int(c.sum()) % 3
        u = dict(cp=put(base, C), e=put(base + [0, 0.5, 0], E), c2=None, w=None, cell=tuple(int(x) for x in c))
        l0.append((u["cp"], u["e"]))
        if v == 1:
            u["c2"] = put(base + [0, 1.0, 0], C)
            l0.append((u["e"], u["c2"]))
        else:
            l1.append((u["e"], u["cp"]))
        if water and (v != 2 or u["cell"] == (1, 1, 1)):
            off = [0.25, 0, 0]
            if u["cell"] == (0, 0, 0):
                off = [-0.25, -0.25, -0.25]
            elif u["cell"] == (1, 1, 1):
                off = [0, 0, 0]
            elif c[0] == 0:
                off = [-0.25, 0, 0]
            u["w"] = put(base + off, WAT)
        us.append(u)
    return box, np.array(pos), np.array(types, np.int32), l0, l1, us


def make_spec(shape, reactions, interval=1, vel=None, water=True, lj=LJ):
    box, pos, types, l0, l1, us = units(shape, water)
    ids = lambda bonds: (np.array(bonds, np.int64) + 1).reshape(-1)      # noqa: E731
    lists = [dict(arity=2, kind="HARMONIC", params=[0.0, 0.5], ids=ids(l0)), dict(arity=2, kind="HARMONIC", params=[0.0, 0.5], ids=ids(l1))]
    spec = RR._spec(box, pos, types, reactions, interval=interval, vel=vel, lists=lists, exclusions=(np.array(l0, np.int64) + 1), lj=lj)
    spec["mass"] = np.array([MASS[t] for t in types])
    return W.snap_to_grid(spec), us


def rows(rec, *names):
    return [tuple(int(x[n]) for n in names) for x in rec]


def ev_rows(ev):
    return [(int(e["step"]), int(e["id_a"]), int(e["id_b"]), int(e["reaction"])) for e in ev]


HYDRO = dict(type_1=C, type_2=WAT, cutoff=CUT, is_virtual=True, new_type_1=A, new_type_2=D)


# ---- (a) removal -----------------------------------------------------------------------------------------------------------------

def removal_pair(make_gpu, shape, prec, unexclude):
    spec, us = make_spec(shape, [HYDRO])
    g = make_gpu(prec)
    h = W.apply(spec, g, thermostat=False)
    g.reaction_neighbour_change(0, "type_1", E, 1, Z, MASS[Z])             # E -> Z in the same step: the rules still match C:E
    g.reaction_remove_bond(0, "type_1", C, 1, C, E, unexclude)
    g.reaction_remove_bond(0, "both", C, 2, E, C, unexclude)               # role 2 is a W: its type never equals the anchor type
    g.reaction_remove_bond(0, "type_1", C, 1, E, C, not unexclude)         # finds what the first rule found: nothing new
    m = RV.Reverse(spec)
    for lvl, t1, t2, ux in ((1, C, E, unexclude), (2, E, C, unexclude), (1, E, C, not unexclude)):
        m.rm_rules.append(dict(reaction=0, invoke_on=1 if lvl == 1 else 3, anchor_type=C, nb_level=lvl, type_1=t1, type_2=t2, unexclude=int(ux)))

    def nb_change(events):
        for a, b, r in events:
            for nb in m.ref.graph[a]:
                if m.ref.type[nb] == E:
                    m.ref.type[nb] = Z; m.ref.mass[nb] = MASS[Z]
    ev, recs, _ = m.step(1, after_events=nb_change)
    return g, h, m, spec, us, ev, recs


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
@pytest.mark.parametrize("unexclude", [True, False])
def test_removal(make_gpu, shape, prec, unexclude):
    g, h, m, spec, us, ev, recs = removal_pair(make_gpu, shape, prec, unexclude)
    nw = sum(u["w"] is not None for u in us)
    nlong = sum(u["w"] is not None and u["c2"] is not None for u in us)
    nshort = nw - nlong
    assert len(ev) == nw and len(recs) == nlong * 2 + nshort * 2 and nlong >= 3 and nshort >= 3      # (short units: the pair is in two lists)
    g.run(1)
    assert ev_rows(g.get_events()) == [e[:4] for e in ev]
    assert rows(g.reaction_removed(), "step", "id_near", "id_far", "list", "reaction") == recs == m.removed
    for li in (h[0], h[1], h["reaction_bonds"]):
        assert np.array_equal(g.get_list(li), m.list_ids(li))
    snap = m.ref.snapshot()
    assert np.array_equal(g.get_state("MOLID"), snap["molid"]) and np.array_equal(g.get_state("RESID"), snap["resid"])
    assert np.array_equal(g.get_exclusions(), snap["excl"])
    assert np.array_equal(g.get_state("TYPE"), snap["type"]) and np.allclose(g.get_state("MASS"), snap["mass"])
    # one more step: the freed pairs feel the pair potential if their exclusion was lifted, and do not if it was kept
    g.run(1)
    x, f = g.get_state("POS"), g.get_state("FORCE")
    now = dict(spec, pos=x, types=snap["type"])
    ref, _, _, _ = pair_reference(now)
    prm, L = pair_params(now), np.array(spec["box"])
    for a, b in snap["excl"] - 1:                                           # pair_reference knows no exclusions: take them out
        p = prm.get((int(snap["type"][a]), int(snap["type"][b])))
        if p is None:
            continue
        d = x[a] - x[b]
        d -= L * np.rint(d / L)
        ff, _ = pair_eval(p, (d * d).sum())
        ref[a] -= ff * d; ref[b] += ff * d
    freed = sorted({(r[1] - 1, r[2] - 1) for r in recs})
    fmax = np.abs(ref).max()
    print("prec %d %s unexclude %d: %d freed pairs, largest reference force %.3e" % (prec, shape, unexclude, len(freed), fmax))
    if not unexclude:
        assert fmax < 1e-9 and np.abs(f).max() == 0.0                       # every pair in reach is still excluded
        return
    assert all(np.abs(ref[a]).max() > 1.0 for a, b in freed)                # every freed pair does feel a force in the reference
    if prec == 64:
        err, flips = rel_err(f, ref), 0
    else:
        err, flips = force_error_without_cutoff_flips(now, f, ref, TOL_F[32], max_flips=0)
    print("force rel err %.3e flips %d (bound %.1e)" % (err, flips, TOL_F[prec]))
    assert err < TOL_F[prec] and flips == 0


# ---- (b) join --------------------------------------------------------------------------------------------------------------------

JOIN_D = 0.375
ONCE = dict(type_1=C, type_2=WAT, cutoff=CUT, is_virtual=True, delta_1=1, delta_2=1)      # no type change: the join alone asks for a rebuild


def join_system(shape):
    box, pos, types, l0, l1, us = units(shape)
    vel = np.zeros((len(pos), 3))
    for u in us:
        if u["c2"] is not None and u["w"] is not None and u["cell"][0] > 0:
            vel[u["cp"]] = [0.5, -0.25, 0.125]                              # moving anchors (free flight: nothing acts on a C)
    spec, us = make_spec(shape, [ONCE], vel=vel)
    return spec, us, vel


def join_engine(make_gpu, spec, us, prec, rule):
    g = make_gpu(prec)
    W.apply(spec, g, thermostat=False)
    taken = next(u for u in us if u["w"] is not None and u["cell"][0] > 1 and u["c2"] is None)
    h0 = g.fix_create()
    # this water is a target already: its join is refused.  (It rides where it is: an entry that moved it at the first drift would
    # meet the displacement criterion one step later, and the rebuild count below would no longer be the join's alone.)
    sep = FX.min_image(spec["pos"][taken["w"]] - spec["pos"][taken["e"]], np.array(spec["box"]))
    d0 = float(np.sqrt((sep * sep).sum()))
    g.fix_add(h0, [(taken["e"] + 1, taken["w"] + 1)], d0)
    hj = g.fix_create()
    if rule:
        g.reaction_join(0, "type_1", hj, JOIN_D)
    return g, h0, hj, dict(taken, d0=d0)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_join(make_gpu, shape, prec):
    spec, us, vel = join_system(shape)
    g, h0, hj, taken = join_engine(make_gpu, spec, us, prec, True)
    g0, _, _, _ = join_engine(make_gpu, spec, us, prec, False)
    m = RV.Reverse(spec)
    assert m.sets.create() == h0 and m.sets.add(h0, [(taken["e"], taken["w"])], taken["d0"]) and m.sets.create() == hj
    m.join_rules.append((0, 1, hj, JOIN_D))
    box, L, dt = np.array(spec["box"]), max(spec["box"]), spec["dt"]
    g.run(0); g0.run(0)
    x0 = g.get_state("POS_UNFOLDED")
    before, before0 = g.timers()["list_rebuilds"], g0.timers()["list_rebuilds"]
    g.run(1); g0.run(1)
    ev, _, added = m.step(1, pos=g0.get_state("POS"))
    assert ev_rows(g.get_events()) == [e[:4] for e in ev] == ev_rows(g0.get_events())
    assert rows(g.fix_joins(), "step", "set", "anchor_id", "target_id", "cause") == m.joins
    causes = [j[4] for j in m.joins]
    assert causes.count(RV.CAUSE_REFUSED) == 1 and causes.count(RV.CAUSE_JOINED) == len(ev) - 1 == len(added)
    assert len(g.fix_log()) == 0
    ids, dist = g.fix_get(hj)
    assert [(a - 1, t - 1, d) for (a, t), d in zip(ids.tolist(), dist.tolist())] == [e[:3] for e in m.sets.entries(hj)] == added
    # the target's position and velocity right after the reaction step
    x1, v1 = RV.place(x0 + dt * vel, vel, added, box)
    xg, vg = g.get_state("POS_UNFOLDED"), g.get_state("VEL")
    bound = 1e-12 * L if prec == 64 else 8 * 2.0 ** -24 * L
    t_idx, a_idx = np.array([e[1] for e in added]), np.array([e[0] for e in added])
    moved = np.linalg.norm(xg[t_idx] - (x0 + dt * vel)[t_idx], axis=1)
    print("prec %d %s: %d joined, position error %.3e (bound %.3e), targets moved by %.3e .. %.3e" % (prec, shape, len(added), np.abs(xg - x1)[np.arange(len(xg)) != taken["w"]].max(), bound, moved.min(), moved.max()))
    free = np.arange(len(xg)) != taken["w"]                                 # (the refused water rides on its own anchor)
    assert np.abs(xg - x1)[free].max() <= bound and np.array_equal(vg[t_idx], vg[a_idx]) and np.array_equal(vg[a_idx], vel[a_idx])
    assert moved.min() > 0.05                                               # from 0.25 (0.433 at the corner: 0.058; 0 on the anchor) to 0.375
    on = next(u for u in us if u["cell"] == (1, 1, 1))
    assert np.abs(xg[on["w"]] - (xg[on["cp"]] + [JOIN_D, 0, 0])).max() <= bound      # |u| = 0: along +x
    crossing = [u for u in us if u["w"] is not None and u["cell"][0] == 0]
    assert len(crossing) >= 3 and all(x0[u["w"]][0] > x0[u["cp"]][0] + 1.0 for u in crossing)      # (stored on the far side of the box)

    def check_distances(what):
        x = g.get_state("POS_UNFOLDED")
        err = np.abs(FX.distances(x, added, box) - JOIN_D)
        b = 1e-12 * JOIN_D if prec == 64 else 8 * 2.0 ** -24 * L            # the bound of tests/test_gpu_fix_distances.py
        print("%s: largest | |x_t - x_a| - d | = %.3e (bound %.3e)" % (what, err.max(), b))
        assert err.max() <= b
    check_distances("after the reaction step")
    # k more steps with moving anchors; the join forced one rebuild and no more
    g.run(10); g0.run(10)
    check_distances("ten steps later")
    vg = g.get_state("VEL")
    assert np.array_equal(vg[t_idx], vg[a_idx]) and np.abs(vg[t_idx]).max() == 0.5
    x11 = g.get_state("POS_UNFOLDED")
    mv = [u for u in us if np.abs(vel[u["cp"]]).max() > 0]
    assert len(mv) >= 2 and all(np.abs((x11 - xg)[u["w"]] - 10 * dt * vel[u["cp"]]).max() <= 10 * bound for u in mv)
    extra = (g.timers()["list_rebuilds"] - before) - (g0.timers()["list_rebuilds"] - before0)
    print("list rebuilds: %d with the join rule, %d without" % (g.timers()["list_rebuilds"] - before, g0.timers()["list_rebuilds"] - before0))
    assert extra == 1
    assert g.fix_count(hj) == len(added) and len(g.fix_joins()) == len(m.joins)


# ---- (c) the full cycle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_full_cycle(make_gpu, shape, prec):
    """condensation A + B -> C:E releases the dummy as a water (lambda 0); hydrolysis C:E + W -> A + B takes the bond out and
    joins the water as a dummy (lambda 0.5); the next condensation releases that water; four reaction steps, rates infinite"""
    box = np.array(BOXES[shape])
    k = int(round(box[0] / SPACING))
    pos, types = [], []
    for c in np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3):
        base = 0.125 + SPACING * c
        if int(c.sum()) % 2 == 0:
            pos += [base, base + [0.375, 0, 0], base + [0, 0.25, 0]]; types += [A, B, D]
        else:
            pos += [base, base + [0.375, 0, 0]]; types += [A, A]              # bystanders
    types = np.array(types, np.int32)
    # (intraresidual: the first condensation merged the two residue ids, and a removal does not undo that)
    cond = dict(type_1=A, type_2=B, cutoff=CUT, new_type_1=C, new_type_2=E, intraresidual=True)
    hydro = dict(HYDRO)
    spec = RR._spec(box, np.array(pos), types, [cond, hydro], interval=1, lj=LJ)
    spec["mass"] = np.array([MASS[t] for t in types])
    spec = W.snap_to_grid(spec)
    n = len(types)
    acid, dummy = np.nonzero(types == A)[0], np.nonzero(types == D)[0]
    owner = {int(d): int(d) - 2 for d in dummy}
    g = make_gpu(prec)
    h = W.apply(spec, g, thermostat=False)
    hs = g.fix_create(A, D)
    g.fix_add(hs, [(owner[d] + 1, d + 1) for d in owner], 0.25)
    g.fix_postprocess(hs, D, WAT, MASS[WAT], 0.0, -1, 0.0)
    g.reaction_release(0, "type_1", hs, 1)
    g.reaction_neighbour_change(1, "type_1", E, 1, B, MASS[B])
    g.reaction_remove_bond(1, "type_1", C, 1, C, E, True)
    g.reaction_join(1, "type_1", hs, 0.25)
    g.reaction_set_resolution(1, "type_2", 0.5)
    m = RV.Reverse(spec)
    assert m.sets.create(A, D) == hs and m.sets.add(hs, [(owner[d], d) for d in owner], 0.25)
    m.sets.rules = [(0, 1, hs, 1)]
    m.rm_rules.append(dict(reaction=1, invoke_on=1, anchor_type=C, nb_level=1, type_1=C, type_2=E, unexclude=1))
    m.join_rules.append((1, 1, hs, 0.25))
    lam = np.ones(n)

    def nb_change(events):
        for a, b, r in events:
            if r == 1:
                for nb in m.ref.graph[a]:
                    if m.ref.type[nb] == E:
                        m.ref.type[nb] = B; m.ref.mass[nb] = MASS[B]
    counts = []
    for step in range(1, 5):
        ev, recs, added = m.step(step, pos=g.get_state("POS"), after_events=nb_change)
        for s_, a, b, r, _ in ev:
            if r == 1:
                lam[b - 1] = 0.5
        rel = m.sets.release_by_reaction([x for s_, a, b, r, _ in ev if r == 0 for x in ((0, 1, a - 1), (0, 2, b - 1))], step)
        for r_ in rel:
            t = r_[3]
            assert m.ref.type[t] == D
            m.ref.type[t] = WAT; m.ref.mass[t] = MASS[WAT]; lam[t] = 0.0
        assert m.sets.release_by_type(m.ref.type, step) == []
        g.run(1)
        counts.append((len(ev), len(recs), len(added), len(rel)))
        assert ev_rows(g.get_events()) == [e[:4] for e in m.ref.events]
        assert g.fix_count(hs) == len(m.sets.entries(hs))
        assert np.array_equal(g.get_state("TYPE"), m.ref.type) and np.array_equal(g.get_state("LAMBDA"), lam)
        assert np.array_equal(g.get_list(h["reaction_bonds"]), m.list_ids(m.bond_list))
    nu = len(dummy)
    print("events, removals, joins, releases per step:", counts)
    assert counts == [(nu, 0, 0, nu), (nu, nu, nu, 0), (nu, 0, 0, nu), (nu, nu, nu, 0)] and nu == {"a": 63, "c": 14}[shape]
    assert rows(g.fix_log(), "step", "set", "anchor_id", "target_id", "cause") == [(s_, h_, a + 1, t + 1, c) for s_, h_, a, t, c in m.sets.records()]
    assert rows(g.fix_joins(), "step", "set", "anchor_id", "target_id", "cause") == m.joins
    assert rows(g.reaction_removed(), "step", "id_near", "id_far", "list", "reaction") == m.removed
    ids, dist = g.fix_get(hs)
    assert [(a - 1, t - 1, d) for (a, t), d in zip(ids.tolist(), dist.tolist())] == [e[:3] for e in m.sets.entries(hs)]
    snap = m.ref.snapshot()
    assert np.array_equal(g.get_exclusions(), snap["excl"]) and np.array_equal(g.get_state("MOLID"), snap["molid"])
    assert np.allclose(g.get_state("MASS"), m.ref.mass)
    assert (m.ref.type[acid] == A).all() and (m.ref.type[dummy] == D).all()      # back where the cycle began


# ---- (d) refusals ------------------------------------------------------------------------------------------------------------------

def refused(code, call, *words):
    with pytest.raises(ChemError) as e:
        call()
    assert e.value.code == code and len(str(e.value)) > 20
    for w in words:
        assert w in str(e.value)


def test_refusals(make_gpu):
    spec, us = make_spec("c", [HYDRO])
    g = make_gpu(64)
    W.apply(spec, g, thermostat=False)
    d = g.dissociation_add(C, E, 0, 0, 0, 1, 0, 1, 0.0, 0.0, 0)
    hs = g.fix_create()
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(5, "type_1", C, 1, C, E), "chem_reaction_add")
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(d, "type_1", C, 1, C, E), "chem_reaction_add")      # a dissociation's index
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(0, 0, C, 1, C, E), "invoke_on")
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(0, 4, C, 1, C, E), "invoke_on")
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(0, "type_1", C, 0, C, E), "nb_level")
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(0, "type_1", -1, 1, C, E), "type")
    refused(_capi.EINVAL, lambda: g.reaction_remove_bond(0, "type_1", C, 1, C, 16), "type")
    refused(_capi.EINVAL, lambda: g._ck(g.api.reaction_remove_bond(g.ctx, None)), "null")
    refused(_capi.EINVAL, lambda: g.reaction_join(5, "type_1", hs, 0.25), "chem_reaction_add")
    refused(_capi.EINVAL, lambda: g.reaction_join(0, 3, hs, 0.25), "role")
    refused(_capi.EINVAL, lambda: g.reaction_join(0, "type_1", hs + 1, 0.25), "unknown set")
    for bad in (0.0, -0.25, float("inf"), float("nan")):
        refused(_capi.EINVAL, lambda: g.reaction_join(0, "type_1", hs, bad), "positive")
    assert len(g.reaction_removed()) == 0 and len(g.fix_joins()) == 0
    g.run(1)                                                                 # none of the refused rules was kept
    assert len(g.get_events()) > 0 and len(g.reaction_removed()) == 0 and len(g.fix_joins()) == 0 and g.fix_count(hs) == 0
    # two in-process ranks: no rules under a decomposition, and no decomposition over rules
    engs = [make_gpu(64) for _ in range(2)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(rk):
        e = engs[rk]
        e.comm_init_local(2, rk, hub)
        W.apply(spec, e, thermostat=False)
        refused(_capi.ENOTIMPL, lambda: e.reaction_remove_bond(0, "type_1", C, 1, C, E), "decomposed")
        refused(_capi.ENOTIMPL, lambda: e.reaction_join(0, "type_1", 0, 0.25), "decomposed")
        return True
    assert _run_ranks(2, rank) == [True, True]
    for wire in (lambda e: e.reaction_remove_bond(0, "type_1", C, 1, C, E), lambda e: e.reaction_join(0, "type_1", e.fix_create(), 0.25)):
        e = make_gpu(64)
        W.apply(spec, e, thermostat=False)
        wire(e)
        refused(_capi.ENOTIMPL, lambda: e.comm_init_local(2, 0, hub + 1000), "decomposed")


# ---- (e) no regression -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_rules_that_no_event_reaches_change_nothing(make_gpu, shape, prec):
    """reaction 1 (B + B) never fires: rules on it leave the trajectory bit for bit what it is without them, while reaction 0
    goes on firing"""
    box, pos, types, l0, l1, us = units(shape)
    rng = np.random.default_rng(5)
    vel = rng.normal(0.0, 0.5, (len(pos), 3))
    never = dict(type_1=B, type_2=B, cutoff=CUT)
    # (no bond is removed here, so the pairs of LJ stay excluded: two more pairs make the particles interact, the second C of a
    # long unit with its own and with the next unit's first one, before the event (C - C) and after it (A - C))
    spec, us = make_spec(shape, [HYDRO, never], interval=3, vel=vel, lj=LJ + [(C, C, 1.0, 0.7, 1.2), (A, C, 1.0, 0.7, 1.2)])
    out = []
    for with_rules in (False, True):
        g = make_gpu(prec)
        W.apply(spec, g, thermostat=False)
        g.reaction_neighbour_change(0, "type_1", E, 1, Z, MASS[Z])
        hs = g.fix_create()
        if with_rules:
            g.reaction_remove_bond(1, "both", B, 1, C, E, True)
            g.reaction_remove_bond(0, "type_2", C, 1, C, E, True)          # role 2 of reaction 0 is a W, never a C: no visit
            g.reaction_join(1, "type_1", hs, 0.25)
        g.run(7)
        g.run(14)
        assert len(g.get_events()) > 0 and len(g.reaction_removed()) == 0 and len(g.fix_joins()) == 0
        out.append((g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("FORCE"), ev_rows(g.get_events()), g.get_state("TYPE")))
    for p, q in zip(*out):
        assert np.array_equal(p, q)
    assert np.abs(out[0][2]).max() > 0.1                                     # (the particles do interact: the trajectories are no free flights)
