"""The zoo of tests/react_ref.py on the CPU: every member's own conditions, asserted on the numpy reference alone, and the
oracle's association step against that reference -- events with r2 to the bit, bond list, states, types, masses, cluster and
residue labels and exclusions after every reaction step.  tests/test_gpu_reaction_step.py runs the same members on the device."""
import numpy as np
import pytest

import react_ref as RR
from chemlab_amd import workloads as W


def _run_engine(e, spec):
    """[(events so far, snapshot)] after each reaction step."""
    h = W.apply(spec, e)
    out = []
    for _ in range(spec["steps"]):
        e.run(spec["reaction"]["interval"])
        out.append((RR.engine_events(e.get_events()), RR.engine_snapshot(e, h)))
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
                                                                        [r[1]["candidates"] for r in ref], [r[1]["rounds"] for r in ref]))


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
