"""The zoo of tests/react_ref.py on the CPU: every member's own conditions, asserted on the numpy reference alone, and the
oracle's association step against that reference -- events with r2 to the bit, bond list, states, types, masses, cluster and
residue labels and exclusions after every reaction step; for the members that restrict, constrain, spawn tuples, change
neighbours, flag intra-cluster events or run the ATRP activator also pad, charges, the spawned lists and the ATRP stats rows.
_setup_extras issues the set-up calls workloads.apply does not know.  tests/test_gpu_reaction_step.py runs the same members on
the device."""
import numpy as np
import pytest

import react_ref as RR
from chemlab_amd import workloads as W


def _setup_extras(e, spec):
    """The calls of spec["ext"] that workloads.apply does not issue: options, restrictions, constraints and neighbour rules, each
    kind in the order of the spec (reaction indices are those reaction_add returned: 0, 1, ...), and the by-types lists.
    Returns the handles of those lists: {"typed<k>": handle}."""
    ext, h = spec.get("ext", {}), {}
    for k, l in enumerate(ext.get("typed_lists", [])):
        h["typed%d" % k] = e.list_create(l["arity"], l["kind"], True)
        for types, p in l["typed"]:
            e.list_set_params(h["typed%d" % k], p, types=types)
        e.list_add(h["typed%d" % k], l["ids"])
    for k, v in ext.get("options", {}).items():
        e.set_option(k, v)
    for r, pairs in ext.get("restrict", []):
        e.reaction_restrict(r, pairs)
    for c in ext.get("constraint", []):
        e.reaction_constraint(*c)
    for rl in ext.get("nb_change", []):
        mode, val = rl.get("set_state", 0), rl.get("new_state", 0)
        e.reaction_neighbour_change(rl["reaction"], rl["invoke_on"], rl["old_type"], rl["nb_level"], rl["new_type"], rl["new_mass"], rl.get("new_q", 0.0),
                                    new_state=val if mode == 1 else None, incr_state=val if mode == 2 else None, state_window=rl.get("window"))
    return h


def _run_engine(e, spec):
    """[(events so far, snapshot)] after each run() call: one reaction interval, or spec["run_each"] steps."""
    h = W.apply(spec, e)
    h.update(_setup_extras(e, spec))
    out = []
    for _ in range(spec["steps"]):
        e.run(spec.get("run_each", spec["reaction"]["interval"]))
        out.append((RR.engine_events(e.get_events()), RR.engine_snapshot(e, h, spec)))
    return out


def check_against_reference(name, got):
    spec, ref = RR.member(name)
    want_ev = []
    for k, ((ev, info, snap), (gev, gsnap)) in enumerate(zip(ref, got)):
        want_ev += RR.ref_events(ev)
        assert gev == want_ev, (name, k, len(gev), len(want_ev), sorted(set(gev) ^ set(want_ev))[:6])
        for key, val in snap.items():
            assert np.array_equal(np.asarray(gsnap[key]), val), (name, k, key)


@pytest.mark.parametrize("name", list(RR.ZOO) + list(RR.SMALL))
def test_zoo_positions_are_exact_in_both_precisions(name):
    spec, _ = RR.member(name)
    assert RR.on_grid(spec)
    assert np.array_equal(W.snap_to_grid(spec)["pos"], spec["pos"])
    assert len(spec["ids"]) <= 2000
    assert all(np.log2(x) == int(np.log2(x)) for x in spec["box"])


@pytest.mark.parametrize("name", list(RR.ZOO) + list(RR.SMALL))
def test_oracle_matches_reference(make_oracle, name):
    spec, ref = RR.member(name)
    check_against_reference(name, _run_engine(make_oracle(), spec))
    print("%s: N %d, events per step %s, candidates %s, rounds %s" % (name, len(spec["ids"]), [len(r[0]) for r in ref],
                                                                        [r[1].get("candidates") for r in ref], [r[1].get("rounds") for r in ref]))


# ---- the zoo's own conditions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "chain_aniso"])
def test_chain_needs_at_least_four_host_batches(name):
    spec, ref = RR.member(name)
    ev, info, _ = ref[0]
    print("%s: %d particles, %d candidates, %d survivors, %d events, %d rounds" % (name, len(spec["ids"]), info["candidates"], info["survivors"],
                                                                                len(ev), info["rounds"]))
    assert len(spec["ids"]) >= 160 and info["rounds"] >= 32
    # a pure chain: consecutive ids only, every d2 different, one periodic face crossed
    assert all(abs(a - b) == 1 for _, a, b, _, _ in ev) and info["distinct_d2"] == len(ev)
    gaps = np.diff(RR.snake(), axis=0)
    assert np.abs(gaps).sum(1).max() < RR.CHAIN_CUT and np.asarray(RR.snake())[:, 0].max() > spec["box"][0]


def test_ties_every_block_distance_is_one_bit_pattern():
    spec, ref = RR.member("ties")
    ev, info, _ = ref[0]
    blk = {d2 for _, _, _, r, d2 in ev if r < 2}
    dup = sum(1 for c in info["cand"] if c[2] == 1)
    print("ties: %d candidates (%d of the duplicate reaction), %d events, %d distinct d2 on the block" % (info["candidates"], dup, len(ev), len(blk)))
    assert len(blk) == 1 and dup > 500 and not any(r == 1 for _, _, _, r, _ in ev)
    # the satellites: ids behind the block, gaps on the cutoff (no), on the minimum (yes), inside the minimum (no), inside the cutoff (yes)
    n = len(spec["ids"])
    sat = {(a, b): d2 for _, a, b, r, d2 in ev if r == 2}
    assert sat == {(n - 5, n - 4): RR.SAT_MIN ** 2, (n - 1, n): (RR.SAT_CUT - RR.GRID) ** 2}
    d2 = [RR.dist2(np.asarray(spec["box"]), spec["pos"][k], spec["pos"][k + 1:k + 2])[0] for k in range(n - 8, n, 2)]
    assert d2[0] == RR.SAT_CUT ** 2 and d2[1] == RR.SAT_MIN ** 2 and d2[2] < RR.SAT_MIN ** 2


def test_ties16_only_reactions_0_and_15_match():
    _, ref = RR.member("ties16")
    ev, info, _ = ref[0]
    by = {r: sum(1 for e in ev if e[3] == r) for r in range(16)}
    cby = {r: sum(1 for c in info["cand"] if c[2] == r) for r in range(16)}
    print("ties16: events per reaction %s, candidates per reaction %s" % (by, cby))
    assert by[15] == 4 and by[0] > 60 and sum(by.values()) == by[0] + by[15]
    assert cby[0] == 540 and cby[15] == 544 and sum(cby.values()) == 1084


@pytest.mark.parametrize("name", ["roles", "roles_4"])
def test_roles_outcomes_by_construction(name):
    spec, ref = RR.member(name)
    ev, _, snap = ref[0]
    got = {(min(a, b), max(a, b)): (a, b, r) for _, a, b, r, _ in ev}
    # slot order of the builder: role-1 states 1 2 4 5, role-2 states -1 0 1, then (same res, same molecule) for both flag values, excluded
    want = {1: None, 3: 0, 5: 0, 7: None, 9: None, 11: 0, 13: None,       # windows
            15: None, 17: None, 20: 1, 22: 1, 25: None}                   # flags, exclusion (the molecules hold a third particle)
    for lo, r in want.items():
        assert (got.get((lo, lo + 1)) or (None, None, None))[2] == r, (lo, r, got.get((lo, lo + 1)))
    assert all(a > b for a, b, _ in got.values())            # the lower tag holds the type_2 role everywhere
    L = np.asarray(spec["box"])
    crossed = {int((np.abs(spec["pos"][a - 1] - spec["pos"][b - 1]) > 0.5 * L).sum()) for a, b, _ in got.values()}
    print("%s: %d events, pairs crossing %s periodic planes" % (name, len(ev), sorted(crossed)))
    assert crossed == {0, 1, 2, 3}
    # a named type that the particle already has keeps its mass: role 2 stays type 1 with mass 1, role 1 becomes type 2 with mass 2
    a, b, _ = got[(3, 4)]
    assert snap["type"][a - 1] == 2 and snap["mass"][a - 1] == 2.0 and snap["type"][b - 1] == 1 and snap["mass"][b - 1] == 1.0


def test_cascade_particles_react_repeatedly_and_rings_are_refused():
    for name in ("cascade_chain", "cascade_ties", "cascade_roles", "cascade_chain_intra", "cascade_ties_intra"):
        _, ref = RR.member(name)
        per = [len(r[0]) for r in ref]
        bonds = [tuple(sorted(b)) for b in ref[-1][2]["bonds"].tolist()]
        print("%s: events per step %s, largest state %d" % (name, per, ref[-1][2]["state"].max()))
        assert len(per) == 4 and len(set(bonds)) == len(bonds)
        if name != "cascade_roles":          # (isolated pairs: one event each, then the pair is bonded)
            assert per[1] > 0 and ref[-1][2]["state"].max() >= 2
        if "ties" in name:                   # the chain is bonded end to end after two steps, the block goes on
            assert per[2] > 0 and ref[-1][2]["state"].max() >= 3
        if name == "cascade_ties_intra":     # ... ring after ring; without the flag the block is one molecule after three steps
            assert min(per) > 0 and ref[-1][2]["state"].max() == 4
    n = {name: sum(len(r[0]) for r in RR.member(name)[1]) for name in ("cascade_ties", "cascade_ties_intra")}
    assert n["cascade_ties_intra"] > n["cascade_ties"]       # ring closures exist and intramolecular = False refuses them


def test_random_mode_and_max_per_interval():
    _, ref = RR.member("random")
    _, ref7 = RR.member("random_max7")
    ev, info, _ = ref[0]
    print("random: %d candidates of 699 pairs, %d events; with max_per_interval = 7: %d" % (info["candidates"], len(ev), len(ref7[0][0])))
    assert 250 < info["candidates"] < 450 and len(ev) > 60
    assert len(ref7[0][0]) == 7 and set(ref7[0][0]) <= set(ev)


def test_cluster_fits_the_documented_capacity_and_refusal_does_not():
    spec, ref = RR.member("cluster")
    info = ref[0][1]
    cap = RR.cand_capacity(len(spec["ids"]))
    cell = np.floor(spec["pos"] / (32.0 / 17.0)).astype(int)
    per = {}
    for c in info["cand"]:
        key = tuple(cell[min(c[0], c[1])] // 3)
        per[key] = per.get(key, 0) + 1
    print("cluster: %d candidates, capacity %d; per block of 3 x 3 x 3 cells (informative): %s" % (info["candidates"], cap, sorted(per.values())))
    assert info["candidates"] == 540 <= cap
    r16 = RR.Reference(RR.cluster(16))
    assert len(r16.candidates(3)) == 16 * 540 > cap


# ---- the members for what hangs onto a reaction: their conditions, on the reference alone ---------------------------------------
def _pairs(ev):
    return {(min(a, b), max(a, b)): r for _, a, b, r, _ in ev}


def test_restrict_conditions():
    spec, ref = RR.member("restrict")
    l0, _ = RR.restrict_lists()
    n = len(spec["ids"])
    listed = {(min(p), max(p)) for p in l0.tolist()}
    got = _pairs(ref[0][0])
    free = _pairs(RR.Reference(RR.restrict(restricted=False)).step(3)[0])
    ev0, ev1 = {p for p, r in got.items() if r == 0}, {p for p, r in got.items() if r == 1}
    L = np.asarray(spec["box"])
    far = {p for p in listed if RR.dist2(L, spec["pos"][p[0] - 1], spec["pos"][p[1] - 1:p[1]])[0] >= RR.BLOCK_CUT ** 2}
    deg = np.bincount(l0.ravel(), minlength=n + 1)
    print("restrict: %d listed pairs (%d written high id first, %d beyond the cutoff), most partners %d, ids without a row %d; events %d of reaction 0, "
          "%d of reaction 1; without the lists %d of reaction 0" % (len(listed), int((l0[:, 0] > l0[:, 1]).sum()), len(far), deg.max(), int((deg[1:] == 0).sum()),
                                                                    len(ev0), len(ev1), sum(1 for r in free.values() if r == 0)))
    assert ev0 and ev0 <= listed and not (far & ev0) and len(far) == 2
    assert ev1 == {p for p, r in free.items() if r == 1} and len(ev1) > 20            # the unrestricted reaction is untouched
    assert (l0[:, 0] > l0[:, 1]).sum() >= 5 and (l0[:, 0] < l0[:, 1]).sum() >= 5
    assert any(p[0] > p[1] and (min(p), max(p)) in ev0 for p in l0.tolist())            # a pair written high id first reacts
    assert deg.max() >= 3 and deg[n] == 0 and (deg[1:] == 0).sum() > 100                # several partners; empty rows, the last tag among them
    x, sat = RR.RESTRICT_X, RR.RESTRICT_SAT
    assert sat == n and free[(x, sat)] == 0 and (x, sat) not in got                     # without the list X takes the nearer satellite ...
    assert got[(RR._blk(4, 0, 0), x)] == 0                                              # ... with it the listed partner, a lattice step away


def test_restrict16_conditions():
    spec, ref = RR.member("restrict16")
    l0, l15 = (set((min(p), max(p)) for p in l.tolist()) for l in RR.restrict_lists())
    got = _pairs(ref[0][0])
    by = {r: {p for p, q in got.items() if q == r} for r in set(got.values())}
    print("restrict16: %d pairs listed for row 0 only, %d for row 15 only, %d for both; events %s" % (len(l0 - l15), len(l15 - l0), len(l0 & l15),
                                                                                                   {r: len(v) for r, v in by.items()}))
    assert set(by) == {0, 15} and by[0] <= l0 and by[15] <= l15 - l0                    # a pair listed for both goes to reaction 0
    assert by[0] & (l0 - l15) and by[0] & (l0 & l15) and len(by[15]) >= 5


@pytest.mark.parametrize("name", ["constraint", "constraint_4"])
def test_constraint_outcomes_by_construction(name):
    spec, ref = RR.member(name)
    got = {min(a, b): (a, b, r) for _, a, b, r, _ in ref[0][0]}
    want = spec["expect"]
    assert {lo: (got[lo][2] if lo in got else None) for lo in want} == want
    assert all(a > b for a, b, r in got.values() if r < 2)                             # reactions 0, 1: the lower tag holds the type_2 role
    assert all(a < b for a, b, r in got.values() if r >= 2)                            # A + A: the forward assignment
    L = np.asarray(spec["box"])
    crossed = {int((np.abs(spec["pos"][a - 1] - spec["pos"][b - 1]) > 0.5 * L).sum()) for a, b, _ in got.values()}
    # with the first call alone (the constraint of reaction 1 on role 1) other pairs react: the second call replaced it
    first = {min(a, b) for _, a, b, r, _ in RR.Reference(RR.constraint(spec["box"], spec["box"][0] / 4.0, second_call=False)).step(3)[0] if r == 1}
    now = {lo for lo, (_, _, r) in got.items() if r == 1}
    deg = np.bincount(np.asarray(spec["lists"][0]["ids"]).ravel())
    print("%s: %d particles, %d pairs, %d accepted (per reaction %s), crossing %s planes, most bonded partners %d; reaction 1 under the first call alone: %d pairs, "
          "%d of them not now" % (name, len(spec["ids"]), len(want), len(got), [sum(1 for g in got.values() if g[2] == r) for r in range(4)], sorted(crossed),
                                  deg.max(), len(first), len(first - now)))
    assert crossed == {0, 1, 2, 3} and deg.max() == 7 and first - now and now - first  # (the hub: seven bonded partners, one more than a TagRow holds inline)
    assert sum(1 for w in want.values() if w is None) >= 20 and all(sum(1 for w in want.values() if w == r) >= (10 if r < 2 else 1) for r in range(4))


def test_constraint_cascade_conditions():
    spec, ref = RR.member("constraint_cascade")
    when = {}
    for k, (ev, _, _) in enumerate(ref):
        for _, a, b, r, _ in ev:
            if r == 0:
                when[a] = k + 1
    want = spec["expect"]
    assert {a: when.get(a) for a in want} == want
    n_rule = [len(r[1]["nb_changed"]) for r in ref]
    print("constraint_cascade: A + B accepted in step 2: %d, in step 3: %d, never: %d; neighbour-rule changes per step %s, events per step %s" % (
        sum(1 for w in want.values() if w == 2), sum(1 for w in want.values() if w == 3), sum(1 for w in want.values() if w is None), n_rule, [len(r[0]) for r in ref]))
    assert n_rule[0] >= 10 and n_rule[1:] == [0, 0]
    assert all(sum(1 for w in want.values() if w == v) >= 10 for v in (2, 3, None))
    # the rule sets a state and reads none: no window, set_state = 1
    assert all(rl["set_state"] == 1 and rl.get("window") is None for rl in spec["ext"]["nb_change"])
    # without the constraint every A + B pair reacts in step 2
    free = RR.Reference(dict(spec, ext=dict(spec["ext"], constraint=[])))
    free.step(3)
    assert sum(1 for e in free.step(6)[0] if e[3] == 0) == len(want)


def test_exchange_conditions():
    spec, ref = RR.member("exchange")
    count = {}
    for ev, _, _ in ref:
        for _, a, b, r, _ in ev:
            count[b] = count.get(b, 0) + 1
    want = spec["expect"]
    assert {c: count.get(c, 0) for c in want} == want
    snap = ref[-1][2]
    print("exchange: %d dimers, exchanges per step %s, B retyped to type 7: %d, charges set: %d, bonds made: %d" % (
        len(want), [len(r[0]) for r in ref], int((snap["type"] == 7).sum()), int((snap["charge"] != 0).sum()), len(snap["bonds"])))
    assert len(want) >= 40 and [len(r[0]) for r in ref] == sorted([len(r[0]) for r in ref], reverse=True) and len(ref[2][0]) == 0 < len(ref[1][0])
    assert len(snap["bonds"]) == 0 and (snap["type"] == 7).sum() == (snap["charge"] == 0.25).sum() == (snap["mass"] == 4.5).sum() >= 10
    assert sorted(set(want.values())) == [0, 1, 2]


@pytest.mark.parametrize("name", ["nbchange", "nbchange_4"])
def test_nbchange_conditions(name):
    spec, ref = RR.member(name)
    (ev1, i1, s1), (ev2, i2, s2) = ref
    t0, st0 = np.asarray(spec["types"]), np.asarray(spec["state"])
    ty, st, q, mass = s2["type"], s2["state"], s2["charge"], s2["mass"]
    P = lambda i: i - 1      # noqa: E731  (index of an id)
    seen = dict(chain=0, ring=0, shared=0, mismatch=0, step2=0)
    edges = set()
    for a, kind in spec["kinds"].items():
        seen[kind] += 1
        if kind == "ring":                               # r0 r1 r2 r3 r4 r5 = a .. a + 5
            assert [ty[P(a + k)] for k in range(6)] == [0, 6, 15, 10, 15, 1] and st[P(a + 1)] == 7
        elif kind == "shared":                           # a1 b1 a2 b2 S: both visits found S inside [0, 2)
            assert ty[P(a + 4)] == 12 and st[P(a + 4)] == 2 and s1["state"][P(a + 4)] == 2
        else:                                            # a b t1 t2 t3 s1 s2 s3 [q]
            if t0[P(a + 2)] == 4:                        # X -> Y -> Z inside one visit
                assert (ty[P(a + 2)], st[P(a + 2)], q[P(a + 2)], mass[P(a + 2)]) == (6, 7, 0.125, 4.0)
            else:
                seen["mismatch"] += 1
                assert (ty[P(a + 2)], st[P(a + 2)], q[P(a + 2)], mass[P(a + 2)]) == (6, 0, 0.0, 1.0)
            assert (ty[P(a + 3)], st[P(a + 3)]) == (7, 3)                                  # t2: a W two bonds from A; rule 2 is invoked on role 2 only
            assert ty[P(a + 4)] == ty[P(a + 7)] == 10 and q[P(a + 4)] == -0.5              # level 3 from both roles
            w0 = st0[P(a + 6)]
            edges.add(int(w0))
            assert (ty[P(a + 6)], st[P(a + 6)]) == ((8, w0 + 1) if RR.NB_WIN[0] <= w0 < RR.NB_WIN[1] else (7, w0))
            if t0[P(a + 5)] == 11:                       # T -> P in step 1; P + Q in step 2 retypes A through the bond of step 1
                seen["step2"] += 1
                assert (s1["type"][P(a + 5)], s1["state"][P(a + 5)]) == (2, 1) and (s1["type"][P(a)], s1["state"][P(a)]) == (0, 1)
                assert (ty[P(a + 5)], st[P(a + 5)]) == (2, 2) and (ty[P(a)], st[P(a)], mass[P(a)]) == (6, 11, 4.0)
            else:
                assert (ty[P(a)], st[P(a)]) == (0, 1)
    rules = [sorted({r for _, r in i["nb_changed"]}) for i in (i1, i2)]
    print("%s: %d particles, cells %s, events per step %s, rule hits per step %s by rules %s, new bonds in step 2: %d" % (
        name, len(spec["ids"]), seen, [len(ev1), len(ev2)], [len(i1["nb_changed"]), len(i2["nb_changed"])], rules, len(s2["bonds"]) - len(s1["bonds"])))
    assert edges == set(RR._EDGE_STATES) and min(seen.values()) >= 4
    assert rules == [[0, 1, 2, 3, 4, 6, 7], [8]]                                           # rule 5 (level 4 in a six-ring) never hits
    assert {e[3] for e in ev1} == {0} and {e[3] for e in ev2} == {1} and len(s2["bonds"]) == len(s1["bonds"]) == len(ev1)
    assert {rl["invoke_on"] for rl in spec["ext"]["nb_change"]} == {1, 2, 3} and {rl.get("set_state", 0) for rl in spec["ext"]["nb_change"]} == {0, 1, 2}
    assert {rl["nb_level"] for rl in spec["ext"]["nb_change"]} == {1, 2, 3, 4}
    # the rule order decides: with rules 0 and 1 swapped an X stops at Y
    sw = dict(spec, ext=dict(nb_change=[spec["ext"]["nb_change"][k] for k in (1, 0, 2, 3, 4, 5, 6, 7, 8)]))
    r = RR.Reference(sw)
    r.step(3)
    assert (r.type == 5).sum() == (t0 == 4).sum() > 0 and (s1["type"] == 5).sum() == 0


def test_spawn_conditions():
    spec, ref = RR.member("spawn")
    r0 = RR.Reference(spec)
    kinds = spec["kinds"]
    nk = {k: sum(1 for v in kinds.values() if v == k) for k in ("line", "flank", "ring")}
    both = {a: set(RR.SPAWN_REG[i]) & set(RR.SPAWN_REG[i + 1]) for a, i in ((3, 1), (4, 3))}
    cnt = dict(rev3=0, rev4=0, both3=0, both4=0, dup=0, by_event=0, not_by_rule=0, second_list=0)
    before = np.asarray(spec["types"])
    x, L = spec["pos"], np.asarray(spec["box"])
    for k, (ev, info, snap) in enumerate(ref):
        seen = set()
        for t, ty, li, rev, new in info["spawned"]:
            a = len(t)
            cnt["rev%d" % a] += rev and ty != ty[::-1]
            cnt["both%d" % a] += (ty in both[a] or ty[::-1] in both[a]) and li in (1, 3)       # registered in both lists: the lower handle took it
            cnt["second_list"] += li in (2, 4)
            cnt["dup"] += (not new) and min(t, t[::-1]) in seen                                 # found again by another bond of the same step
            seen.add(min(t, t[::-1]))
            cnt["by_event"] += r0.match(tuple(int(before[p]) for p in t)) != (li, rev)          # the types before the step's events would not have matched so
            cnt["not_by_rule"] += r0.match(tuple(int(snap["type"][p]) for p in t)) != (li, rev)  # ... nor would those the neighbour rule left
            # no tuple is near a singular geometry: the force comparison keeps the tolerance of the well-conditioned molecules
            d = [_minimg(x[t[i + 1]] - x[t[i]], L) for i in range(a - 1)]
            n = [np.cross(d[i], d[i + 1]) for i in range(a - 2)]
            assert all(np.linalg.norm(v) > 0.3 * np.linalg.norm(d[i]) * np.linalg.norm(d[i + 1]) for i, v in enumerate(n)), (t, "collinear")
            if a == 4:
                assert abs(np.dot(n[0], n[1])) < 0.97 * np.linalg.norm(n[0]) * np.linalg.norm(n[1]), (t, "planar")
        before = snap["type"]
    per = [[sum(1 for s in r[1]["spawned"] if len(s[0]) == a and s[4]) for a in (3, 4)] for r in ref]
    print("spawn: %d particles, cells %s, events per step %s, (angles, dihedrals) inserted per step %s, conditions %s" % (
        len(spec["ids"]), nk, [len(r[0]) for r in ref], per, {k: int(v) for k, v in cnt.items()}))
    assert min(nk.values()) >= 12 and all(min(p) > 0 for p in per)
    assert cnt["dup"] == nk["flank"] and min(cnt.values()) > 0
    # every list holds what the log says, once; a ring gives two angles and three dihedrals
    final = ref[-1][2]
    for li in (1, 2, 3, 4):
        rows = [tuple(r) for r in final["list%d" % li].tolist()]
        assert len(rows) == len({min(r, r[::-1]) for r in rows}) == sum(1 for r in ref for s in r[1]["spawned"] if s[2] == li and s[4]) > 0
    ring = {i for i, v in kinds.items() if v == "ring"}
    in_ring = lambda row: any(i <= row[0] < i + 6 for i in ring)      # noqa: E731
    assert sum(1 for li in (1, 2) for r in final["list%d" % li].tolist() if in_ring(r)) == 2 * nk["ring"]
    assert sum(1 for li in (3, 4) for r in final["list%d" % li].tolist() if in_ring(r)) == 3 * nk["ring"]
    # 1-3 and 1-4 exclusions: exactly the (first, last) pairs of the inserted tuples beside the bonds
    want = {tuple(sorted(p)) for p in np.asarray(spec["exclusions"]).tolist()} | {tuple(sorted(p)) for p in final["bonds"].tolist()}
    want |= {(min(r[0], r[-1]), max(r[0], r[-1])) for li in (1, 2, 3, 4) for r in final["list%d" % li].tolist()}
    assert {tuple(p) for p in final["excl"].tolist()} == want


def bonded_reference(spec, snap):
    """bonded_ref.reference on the reference's own lists and types after a step: the lists of the spec, then the reaction bonds."""
    import bonded_ref as B
    lists = [dict(kind=l["kind"], arity=l["arity"], params=l["params"], ids=snap["list%d" % i] if l["arity"] > 2 else l["ids"])
             for i, l in enumerate(spec["lists"])]
    lists += spec.get("ext", {}).get("typed_lists", [])
    lists.append(dict(kind=spec["reaction"]["bond"][0], arity=2, params=spec["reaction"]["bond"][1], ids=snap["bonds"]))
    return B.reference(spec["pos"], spec["box"], snap["type"], lists, mol=spec["cell"])


def run_with_forces(e, spec):
    """([(FORCE, epot of every list of the spec, of the by-types lists and of the reaction bonds, sizes of the spec's lists)] after each
    reaction step, POS at the end)."""
    h = W.apply(spec, e)
    h.update(_setup_extras(e, spec))
    keys = list(range(len(spec["lists"]))) + ["typed%d" % k for k in range(len(spec.get("ext", {}).get("typed_lists", [])))] + ["reaction_bonds"]
    out = []
    for _ in range(spec["steps"]):
        e.run(spec["reaction"]["interval"])
        e.run(0)
        obs = e.observe()
        out.append((e.get_state("FORCE"), [obs["epot_list"][h[k]] for k in keys], [obs["list_size"][h[k]] for k in range(len(spec["lists"]))]))
    return out, e.get_state("POS")


def check_forces(spec, ref, out, pos, tol_f, tol_e, label):
    import bonded_ref as B
    assert np.array_equal(pos, spec["pos"])                      # masses of 2^80: nothing moved
    for k, ((f, e, size), (_, _, snap)) in enumerate(zip(out, ref)):
        w = bonded_reference(spec, snap)
        assert size == [len(snap["list%d" % i]) if l["arity"] > 2 else len(l["ids"]) for i, l in enumerate(spec["lists"])], (k, size)
        err = B.molecule_errors(f, w["force"], spec["cell"])
        print("%s step %d: largest force error relative to the cell's largest component %.2e, energies %s" % (label, k + 1, (err / w["fmax"]).max(), e))
        assert (w["fmax"] > 0).all() and (err <= tol_f * w["fmax"]).all(), (label, k, (err / w["fmax"]).max())
        for got, ex in zip(e, w["energy"]):
            assert got == pytest.approx(ex, **tol_e), (label, k, e, w["energy"])


FORCE_MEMBERS = ("spawn", "nbchange_typed")


@pytest.mark.parametrize("name", FORCE_MEMBERS)
def test_forces_on_the_oracle(make_oracle, name):
    """The force comparison of tests/test_gpu_reaction_step.py, run on the oracle with the fp64 tolerances of tests/test_gpu_bonded.py."""
    spec, ref = RR.member(name)
    out, pos = run_with_forces(make_oracle(), spec)
    check_forces(spec, ref, out, pos, 1e-10, dict(rel=1e-11, abs=1e-11), "oracle " + name)


@pytest.mark.parametrize("name", ["atrp", "atrp_centres"])
def test_atrp_conditions(name):
    spec, ref = RR.member(name)
    rows = ref[-1][2]["atrp"]
    fired = [k + 1 for k, r in enumerate(ref) if "atrp" in r[1]]
    reacted = [k + 1 for k, r in enumerate(ref) if "candidates" in r[1]]
    ends_before = {}
    for k, (ev, info, snap) in enumerate(ref):
        for _, a, b, r, _ in ev:
            ends_before[a] = k + 1
    pool = len(spec["ids"]) if spec["atrp"]["select_from_all"] else None
    print("%s: firings at %s, reaction steps at %s, events per reaction step %s, activated %s, deactivated %s, selected %s of candidates %s, activator share %s" % (
        name, fired, reacted, [len(ref[k - 1][0]) for k in reacted], rows[:, 3].astype(int).tolist(), rows[:, 4].astype(int).tolist(),
        rows[:, 2].astype(int).tolist(), rows[:, 1].astype(int).tolist(), rows[:, 5].tolist()))
    assert fired == [2, 4, 6, 8, 10, 12] and reacted == [3, 6, 9, 12] and rows[:, 0].tolist() == [2.0, 4.0, 6.0, 8.0, 10.0, 12.0]
    assert all(r[2] == min(40, pool if pool else r[1]) for r in rows) and (pool or rows[:, 1].max()) > 40      # num_particles is smaller than the pool
    assert rows[:, 5].min() == 0.0 and rows[:, 3].sum() > 3 and rows[:, 4].sum() > 0                            # the clamp at 0 is reached; both directions occur
    # only an activation makes an end reactive: every role-1 particle of an event was type 0 through the activator or as a bonded monomer
    t0 = np.asarray(spec["types"])
    assert not (t0 == 0).any() and sum(len(r[0]) for r in ref) >= 4 and len(ref[1][0]) == 0
    # ... a monomer bonded at one reaction step is the active end of the next, and the rule retyped the old end
    final = ref[-1][2]
    assert (final["type"] == 3).sum() == len(final["bonds"]) > 0 and all(final["type"][a - 1] == 3 for a, _ in final["bonds"].tolist())
    assert any(ends_before.get(b) for a, b in final["bonds"].tolist())                                         # a chain grew twice
    # both fall on steps 6 and 12: the firing sees the states and types the reaction step of that step left
    assert len(ref[5][0]) > 0 or len(ref[11][0]) > 0


def _minimg(d, L):
    return d - L * np.rint(d / L)


def test_intra_flag_conditions():
    _, on = RR.member("intra_flag")
    _, off = RR.member("cascade_ties_intra")
    pads = [r[1]["pad"] for r in on]
    print("intra_flag: events per step %s, of them inside one molecule %s" % ([len(p) for p in pads], [sum(p) for p in pads]))
    assert pads[0] and not any(pads[0])                                                # step 1: nothing is bonded yet
    later = [x for p in pads[1:] for x in p]
    assert 0 in later and 1 in later and any(0 in p and 1 in p for p in pads[1:])      # steps 2 to 4: both values, in one step too
    for (ev1, _, s1), (ev0, _, s0) in zip(on, off):                                    # the option changes nothing else
        assert ev1 == ev0 and not s0["pad"].any()
        assert all(np.array_equal(s1[k], s0[k]) for k in s0 if k != "pad")


# ---- member 8: closing pairs, on the oracle's own positions ---------------------------------------------------------------
def check_closing(e, spec):
    """Runs `interval` steps without a rebuild and compares the events with the reference evaluated at the positions read back."""
    h = W.apply(spec, e)
    e.run(0)
    x0, t0 = e.get_state("POS_UNFOLDED"), e.timers()
    e.run(spec["reaction"]["interval"])
    x1, t1 = e.get_state("POS_UNFOLDED"), e.timers()
    assert t1["rebuilds"] == t0["rebuilds"] and t1["list_rebuilds"] == t0["list_rebuilds"], (t0, t1)
    assert np.abs(x1 - x0).max() >= 0.44 * RR.SKIN
    ref = RR.Reference(spec)
    ev, info = ref.step(spec["reaction"]["interval"], pos=e.get_state("POS"))
    L = np.asarray(spec["box"])
    for k in range(0, len(spec["ids"]), 2):
        d2 = RR.dist2(L, e.get_state("POS")[k], e.get_state("POS")[k + 1:k + 2])[0]
        assert abs(d2 / RR.RC ** 2 - 1.0) > 1e-9
    want = [(k + 1, k + 2) for k in np.nonzero(spec["closing"])[0] * 2]
    assert sorted((min(a, b), max(a, b)) for _, a, b, _, _ in ev) == want and len(want) == 51
    got = RR.engine_events(e.get_events())
    assert [g[:4] for g in got] == [w[:4] for w in RR.ref_events(ev)]
    assert got == RR.ref_events(ev)      # minimgD with a power-of-two box is exact: r2 to the bit
    assert np.array_equal(e.get_list(h["reaction_bonds"]), np.asarray([(a, b) for _, a, b, _, _ in ev]))
    return got


@pytest.mark.parametrize("crit", [0, 1])
def test_closing_pairs_on_the_oracle(make_oracle, crit):
    spec = RR.closing_pairs()
    spec["rebuild_criterion"] = crit
    L = np.asarray(spec["box"])
    cells = np.floor(spec["pos"] / (L / 17.0)).astype(int) % 17
    assert all((cells[k] != cells[k + 1]).any() for k in range(0, len(cells), 2))      # partners start in different cells
    d = spec["pos"][0::2] - spec["pos"][1::2]
    assert int((np.abs(d) > 0.5 * L).any(1).sum()) >= 20                               # ... many of them across a periodic face
    check_closing(make_oracle(), spec)
