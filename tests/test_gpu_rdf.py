"""Radial distribution functions accumulated on the device (chem_rdf_*), in both precisions, on every list path (LDS tiles, the
per-cell list, the brute-force list, a slab that is its own neighbour, two and three slabs through comm_init_local): every count
against tests/rdf_ref.py -- a plain O(N^2) numpy restatement of the rule set -- at positions, types, labels and box read back from
the engine.  Exact integer equality; `density` within 4 ulp.  On slabs every rank must return the same global integers."""
import ctypes

import numpy as np
import pytest

import aged_ref as AR
import rdf_ref as RR
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from test_gpu_parity import _run_ranks

pytestmark = pytest.mark.gpu

PATHS = {"tiles": (1, {}), "cells": (1, {"tiles": 0}), "brute": (1, {}), "dd_self": (1, {"dd_self": 1}), "P2": (2, {}), "P3": (3, {})}
SLABS = ("dd_self", "P2", "P3")
SEL4 = [(-1, -1), (0, 0), (0, 1), (1, 1)]
PREC = [64, 32]
_OWN_HUB = [1 << 21]           # hub ids of this module's own, far from those other modules name


def _engine(make_gpu, prec, path, spec, **kw):
    """One engine on a single-domain path (or the slab that is its own neighbour), set up."""
    g = make_gpu(prec)
    for k, v in PATHS[path][1].items():
        g.set_option(k, v)
    h = W.apply(spec, g, **kw)
    return g, h


def _on(make_gpu, prec, path, spec, body, **kw):
    """body(engine, handles) on every rank of `path` (threads, one context each); the ranks' results.  Read-backs and rdf() are
    collective on slabs: every rank makes the same calls."""
    P, opts = PATHS[path]
    engs = [make_gpu(prec) for _ in range(P)]
    _OWN_HUB[0] += 1
    hub = _OWN_HUB[0]

    def rank(r):
        g = engs[r]
        for k, v in opts.items():
            g.set_option(k, v)
        if P > 1:
            g.comm_init_local(P, r, hub)
        return body(g, W.apply(spec, g, **kw))
    return _run_ranks(P, rank) if P > 1 else [rank(0)]


def _same_rdf(res, key="rdf"):
    """Every rank holds the same global integers and normalisers."""
    for r in res[1:]:
        a, b = r[key], res[0][key]
        assert a["frames"] == b["frames"] and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["pairs"], b["pairs"])
        assert np.array_equal(a["density"].view(np.uint64), b["density"].view(np.uint64))
    return res[0]


def _frame(g):
    return dict(box=g.box(), pos=g.get_state("POS"), types=g.get_state("TYPE"), mol=g.get_state("MOLID"))


def _add(acc, f, types=None, mol=None):
    return acc.add(f["box"], f["pos"], f["types"] if types is None else types, f["mol"] if mol is None else mol)


def _equal(got, acc, what):
    assert got["frames"] == acc.frames, (what, got["frames"], acc.frames)
    assert [int(v) for v in got["pairs"]] == acc.pairs, (what, got["pairs"], acc.pairs)
    bad = np.argwhere(got["counts"] != acc.counts)
    assert len(bad) == 0, (what, len(bad), bad[:5], got["counts"][tuple(bad[0])], acc.counts[tuple(bad[0])])
    for s in range(len(acc.sel)):
        assert RR.ulps(got["density"][s], acc.density[s]) <= 4, (what, s, got["density"][s], acc.density[s])


def _path_is(g, path):
    """The engine is on the tile path or not, as the case wants (the box decides between the per-cell and the brute-force list)."""
    out = (ctypes.c_int32 * 8)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    assert (out[0] > 0) == (path == "tiles" or path in SLABS), (path, list(out))
    if path in ("cells", "brute"):
        assert (out[1] < 3) == (path == "brute"), (path, list(out))


def trimers(path):
    """Two types, bonds, angles and their exclusions (workloads.trimer_melt without its reaction): 3000 particles in 11 x 6 x 6
    cells for the tile and per-cell paths, 81 in a box under three cells across for the brute-force list."""
    return W.trimer_melt(n_mol=27 if path == "brute" else 1000, reactive=False)


def thermal(path):
    """One type, no bonds: aged_ref's melts (2197 particles in 5 x 5 x 5 cells; the 343-particle box of the brute-force list,
    whose ids are not its tags; the 5 x 5 x 12-cell slab box, about 3100 particles, for one, two and three slabs), given a second
    type.  The slab melt also gets exclusions -- every one of its first 300 particles with its nearest neighbour -- so that
    excluded pairs, some of them across a slab boundary, are among the pairs to count."""
    name = "small_box" if path == "brute" else ("slab" if path in SLABS else "melt2197")
    spec = dict(AR.melt_spec(name, 0))
    spec["types"] = (np.arange(len(spec["ids"])) % 3 == 0).astype(np.int32)
    rc = spec["rc"]
    spec["lj"] = [(0, 0, 1.0, 1.0, rc), (0, 1, 1.0, 1.0, rc), (1, 1, 1.0, 1.0, rc)]
    if path in SLABS:
        L, x, ids = np.asarray(spec["box"], dtype=np.float64), np.asarray(spec["pos"], dtype=np.float64), np.asarray(spec["ids"])
        ex = set()
        for i in range(300):
            d2 = RR.dist2(L, x[i], x)
            d2[i] = np.inf
            j = int(np.argmin(d2))
            assert d2[j] < rc * rc
            ex.add((int(min(ids[i], ids[j])), int(max(ids[i], ids[j]))))
        spec["exclusions"] = np.array(sorted(ex), dtype=np.int64)
    return spec


# ---- single frames ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("path", ["tiles", "cells", "brute"])      # (the slab paths: test_bonded_melt_on_slabs_with_labels_across_the_boundaries)
def test_bonded_melt_single_frame_with_excluded_pairs(make_gpu, path, prec):
    """Selectors (-1,-1), (0,0), (0,1), (1,1) with the molecule split, a frame before anything ran and one after 20 steps: every
    count equals the reference, and the bond-length peak -- excluded pairs -- is there, all of it intramolecular."""
    spec = trimers(path)
    g, _ = _engine(make_gpu, prec, path, spec)
    g.rdf_init(spec["rc"], 64, SEL4, split_molecules=True)
    acc = RR.Accumulator(spec["rc"], 64, SEL4, split=True)
    g.rdf_sample()
    _path_is(g, path)
    got = g.rdf()
    _equal(got, _add(acc, _frame(g)), (path, prec, "first frame"))
    nmol = len(spec["ids"]) // 3
    peak = (got["edges"][:-1] < 1.1) & (got["edges"][1:] > 0.85)                   # bonds of 0.97 +- 0.04 at the start
    assert got["counts"][2, 0, peak].sum() == 2 * nmol == got["counts"][2, 0].sum()      # every MA-ML bond, an excluded pair, counted once
    assert got["counts"][1, 0].sum() == nmol                                          # the 1-3 pairs MA .. MA
    assert got["g"].shape == (4, 2, 64) and got["g"][2, 0, peak].max() > 0 and got["r"].shape == (64,)
    g.run(20)
    g.rdf_sample()
    got = g.rdf()
    _equal(got, _add(acc, _frame(g)), (path, prec, "second frame"))
    assert got["counts"][2, 0].sum() == 4 * nmol
    print("%s fp%d: %d pairs inside r_max in two frames, %d of them intramolecular" % (path, prec, got["counts"][0].sum(), got["counts"][0, 0].sum()))


def slab_trimers():
    """workloads.trimer_melt's system -- MA-ML-MA trimers, harmonic bonds and angles, their exclusions, the end-group coupling
    MA + MA that forms bonds -- laid out for slabs: 8 x 8 x 12 trimers ALONG z in a box of 14.88 x 14.88 x 37.2, i.e. 5 x 5 x 12
    cells (twelve layers of 3.1 for two and three slabs), 2304 particles.  Every trimer has its middle bead on a layer boundary, so
    bonds and 1-3 pairs lie across every boundary between slabs and across the periodic face; the MA ends of neighbours along z start 1.16 apart, inside the reaction
    radius of 1.2, so the first reaction step bonds trimers into chains that cross the slab boundaries too."""
    base = W.trimer_melt(n_mol=8, reactive=True, interval=10)
    rng = np.random.default_rng(11)
    nx, ny, nz, cell = 8, 8, 12, np.array([1.86, 1.86, 3.1])
    n_mol = nx * ny * nz
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    centres = (g + np.array([0.5, 0.5, 1.0])) * cell       # the middle bead on a layer boundary (a layer is 3.1 thick): every trimer straddles one
    dirs = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.03, 0.03, (n_mol, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    pos = np.stack([centres - 0.97 * dirs, centres, centres + 0.97 * dirs], 1).reshape(-1, 3) + rng.uniform(-0.01, 0.01, (3 * n_mol, 3))
    n = 3 * n_mol
    b0 = np.arange(n_mol) * 3 + 1
    bonds = np.concatenate([np.stack([b0, b0 + 1], 1), np.stack([b0 + 1, b0 + 2], 1)])
    angles = np.stack([b0, b0 + 1, b0 + 2], 1)
    mass = np.ones(n)
    box = (np.array([nx, ny, nz]) * cell).tolist()
    spec = dict(base, name="slab_trimers", n=n, box=box, ids=np.arange(1, n + 1), types=np.tile(np.array([0, 1, 0], np.int32), n_mol),
                pos=pos % np.array(box), vel=W._maxwell(rng, n, base["kT"], mass), mass=mass, state=np.zeros(n, np.int32),
                res_id=(np.arange(n) // 3 + 1).astype(np.int32), exclusions=np.concatenate([bonds, np.stack([b0, b0 + 2], 1)]),
                lists=[dict(base["lists"][0], ids=bonds), dict(base["lists"][1], ids=angles)])
    return spec, bonds


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("path", list(SLABS))
def test_bonded_melt_on_slabs_with_labels_across_the_boundaries(make_gpu, path, prec):
    """The bonded two-type melt on dd_self, P2 and P3: SEL4 with the molecule split, a frame before anything ran, and one behind
    the first reaction step (step 10), which merges labels.  Exact equality with the reference at the read-back positions,
    types and labels, the same integers on every rank.  The bond peak is in the intramolecular part; bonded pairs lie across
    the slab boundaries (and, for dd_self, across the periodic face, where the partner is the slab's own ghost)."""
    import mass_ref
    spec, bonds = slab_trimers()
    nmol = spec["n"] // 3

    def body(g, h):
        g.rdf_init(spec["rc"], 64, SEL4, split_molecules=True)
        g.rdf_sample()
        _path_is(g, path)
        first = dict(frame=_frame(g), rdf=g.rdf())
        g.rdf_reset()
        g.run(12)
        g.rdf_sample()
        return dict(first=first["rdf"], frame0=first["frame"], rdf=g.rdf(), frame=_frame(g), nev=len(g.get_events()),
                    nb=len(g.get_list(h["reaction_bonds"])))
    res = _on(make_gpu, prec, path, spec, body)
    _same_rdf(res, "first")
    r0 = _same_rdf(res)
    # bonded pairs whose members different ranks own (two and three slabs), or that cross the periodic z face (every path)
    P = PATHS[path][0]
    x = r0["frame0"]["pos"]
    ia, ib = bonds[:, 0] - 1, bonds[:, 1] - 1
    across_face = int((np.abs(x[ia, 2] - x[ib, 2]) > 0.5 * spec["box"][2]).sum())
    assert across_face >= 32
    if P > 1:
        own = mass_ref.slab_of(spec, x, P)
        assert int((own[ia] != own[ib]).sum()) >= 32 * (P - 1), (path, int((own[ia] != own[ib]).sum()))
    got = r0["first"]
    _equal(got, _add(RR.Accumulator(spec["rc"], 64, SEL4, split=True), r0["frame0"]), (path, prec, "first frame"))
    peak = (got["edges"][:-1] < 1.1) & (got["edges"][1:] > 0.85)
    assert got["counts"][2, 0, peak].sum() == 2 * nmol == got["counts"][2, 0].sum()      # every MA-ML bond, wherever its partner lives
    assert got["counts"][1, 0].sum() == nmol and got["counts"][2, 1, peak].sum() == 0      # the 1-3 pairs; no unbonded MA-ML pair that close
    # behind the reaction step: chains of trimers, labels merged on every rank
    got = r0["rdf"]
    assert r0["nev"] > 0 and r0["nb"] == r0["nev"] and len(set(r0["frame"]["mol"])) < nmol
    _equal(got, _add(RR.Accumulator(spec["rc"], 64, SEL4, split=True), r0["frame"]), (path, prec, "behind the reaction step"))
    assert got["counts"][1, 0].sum() >= nmol + r0["nev"]                                   # MA .. MA: the 1-3 pairs and the new MA-MA bonds
    print("%s fp%d: %d bonds across the periodic face, %d reaction bonds, %d molecules left" % (path, prec, across_face, r0["nb"], len(set(r0["frame"]["mol"]))))


def lattice(path):
    """A simple-cubic lattice of spacing 1 in a box whose edge is a power of two (16; 4 for the brute-force list): every coordinate a
    multiple of 2^-10, every d2 exact in both precisions.  r_max = 2, 32 bins: nbins / r_max = 16, so the shells at d2 = 1 sit
    exactly on e[16] (they go up), those at d2 = 4 exactly on e[32] (dropped); every face, edge and corner of the box is crossed,
    and on two and three slabs (twelve cell layers of 8/3 along z) lattice neighbours straddle every slab boundary."""
    k = 4 if path == "brute" else 16
    kz = 2 * k if path in SLABS else k
    g1 = np.arange(k)
    pos = np.stack(np.meshgrid(g1, g1, np.arange(kz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64) + 0.25
    # an edge zoo on top: pairs a bin edge apart along x and z, across the face at x = 0, and one 2^-10 short of an edge
    zoo = []
    for c, u, d in (([2.5, 2.5, 2.5], [1, 0, 0], 0.5), ([3.5, 2.5, 0.5], [0, 1, 0], 0.5 - 2.0 ** -10), ([0.5, 1.5, 0.5], [-1, 0, 0], 0.75),
                    ([1.5, 0.5, 1.5], [0, 0, 1], 0.8125)):
        zoo += [np.array(c), np.array(c) + d * np.array(u, dtype=np.float64)]
    pos = np.concatenate([pos, np.array(zoo) % k])
    n = len(pos)
    return dict(name="lattice", n=n, box=[float(k), float(k), float(kz)], rc=2.0, skin=0.5, dt=0.001, ids=np.arange(1, n + 1), types=(np.arange(n) % 2).astype(np.int32),
                pos=pos, vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32),
                lj=[(0, 0, 1e-6, 0.5, 2.0), (0, 1, 1e-6, 0.5, 2.0), (1, 1, 1e-6, 0.5, 2.0)], kT=0.0, gamma=0.0, seed=1, nlat=k * k * kz)


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("path", list(PATHS))
def test_lattice_shells_and_pairs_on_bin_edges(make_gpu, path, prec):
    spec = lattice(path)

    def body(g, _):
        g.rdf_init(2.0, 32, [(-1, -1), (0, 1)])
        g.rdf_sample()
        _path_is(g, path)
        return dict(frame=_frame(g), rdf=g.rdf())
    r0 = _same_rdf(_on(make_gpu, prec, path, spec, body))
    f, got = r0["frame"], r0["rdf"]
    assert np.array_equal(f["pos"], spec["pos"])                      # the engine holds these coordinates exactly
    _equal(got, _add(RR.Accumulator(2.0, 32, [(-1, -1), (0, 1)]), f), (path, prec))
    # the lattice alone, by hand: 6, 12, 8 neighbours per site at d2 = 1, 2, 3; d2 = 4 = e2[32] is not counted
    lat = RR.Accumulator(2.0, 32).add(f["box"], f["pos"][:spec["nlat"]], f["types"][:spec["nlat"]])
    e2 = RR.edges2(2.0, 32)
    want = np.zeros(32, np.uint64)
    for d2, per in ((1.0, 6), (2.0, 12), (3.0, 8)):
        want[int(RR.bin_of(np.array([d2]), e2)[0])] += spec["nlat"] * per // 2
    assert np.array_equal(lat.counts[0, 0], want) and want[16] == 3 * spec["nlat"] and want[31] == 0
    assert got["counts"][0, 0, 16] >= want[16]


# ---- sampling inside a run -------------------------------------------------------------------------------------------------------

K_STEPS = 40
_TWIN = {}


def _twin(make_gpu, path, prec):
    """The reference run of the thermal melt: run(1) forty times, a frame read back after every step; the steps at which the
    list was rebuilt, the final state."""
    key = (path, prec)
    if key not in _TWIN:
        spec = thermal(path)

        def body(g, _):
            g.run(0)
            frames, lreb = [_frame(g)], [g.timers()["list_rebuilds"]]
            for _k in range(K_STEPS):
                g.run(1)
                frames.append(_frame(g))
                lreb.append(g.timers()["list_rebuilds"])
            return dict(frames=frames, lreb=lreb, end=_end_state(g))
        r0 = _on(make_gpu, prec, path, spec, body, thermostat=False)[0]
        _, oldest = AR.check_steps(r0["lreb"])
        oldest = [s for s in oldest if 4 <= s <= K_STEPS // 2]
        assert oldest, r0["lreb"]
        _TWIN[key] = dict(spec=spec, frames=r0["frames"], lreb=r0["lreb"], every=oldest[0], end=r0["end"])
    return _TWIN[key]


def _end_state(g):
    t = g.timers()
    ev = g.get_events()
    return dict(pos=g.get_state("POS"), img=g.get_state("IMAGE"), vel=g.get_state("VEL"), f=g.get_state("FORCE"),
                ev=[tuple(e) for e in ev.tolist()], reb=t["rebuilds"], lreb=t["list_rebuilds"])


def _same_state(a, b, what):
    for k in ("pos", "img", "vel", "f"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["ev"] == b["ev"] and (a["reb"], a["lreb"]) == (b["reb"], b["lreb"]), (what, a["reb"], b["reb"], a["lreb"], b["lreb"])


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("path", list(PATHS))
def test_sample_every_over_an_aged_list_in_pieces_and_without_perturbing(make_gpu, path, prec):
    """sample_every(e) inside one run(40) that spans several list builds, e an oldest-list step of the twin run (the step in
    front of a list build), so the frames at e, 2e, ... include one taken from the list at its oldest.  The accumulators equal
    the sum of the reference frames at the twin's positions.  run(a); run(b) gives the same accumulators bit for bit, and the
    trajectory, events and rebuild counters are those of a run that never sampled."""
    tw = _twin(make_gpu, path, prec)
    spec, e = tw["spec"], tw["every"]
    assert tw["lreb"][-1] - tw["lreb"][0] >= 3 and tw["lreb"][e + 1] == tw["lreb"][e] + 1, (e, tw["lreb"])
    sel = [(-1, -1), (0, 1), (1, 1)]
    acc = RR.Accumulator(spec["rc"], 100, sel, split=True)
    for s in range(e, K_STEPS + 1, e):
        _add(acc, tw["frames"][s])

    def sampled(pieces):
        def body(g, _):
            g.rdf_init(spec["rc"], 100, sel, split_molecules=True)
            g.rdf_sample_every(e)
            for p in pieces:
                g.run(p)
            return dict(rdf=g.rdf(), end=_end_state(g))
        r0 = _same_rdf(_on(make_gpu, prec, path, spec, body, thermostat=False))
        return r0["end"], r0["rdf"]
    enda, whole = sampled([K_STEPS])
    _equal(whole, acc, (path, prec, "run(40)", e))
    assert whole["frames"] == K_STEPS // e >= 2
    if path in SLABS:                                       # the excluded pairs are inside r_max: counted like any other
        assert len(spec["exclusions"]) >= 150
    _same_state(enda, tw["end"], (path, prec, "sampled against never sampled"))
    endb, parts = sampled([e, 1, K_STEPS - e - 1])          # a piece ends on a sampled step; the next does not sample its start
    assert parts["frames"] == whole["frames"] and np.array_equal(parts["counts"], whole["counts"])
    assert np.array_equal(parts["pairs"], whole["pairs"]) and np.array_equal(parts["density"].view(np.uint64), whole["density"].view(np.uint64))
    _same_state(endb, tw["end"], (path, prec, "pieces"))
    print("%s fp%d: frames every %d steps over %d list builds, %d pairs counted" % (path, prec, e, tw["lreb"][-1] - tw["lreb"][0], whole["counts"][0].sum()))


def _joined_pairs_histogram(bonds, ids, frame, r_max, nbins):
    """The histogram of all pairs inside r_max that the bonds join into one cluster, built from the bond list alone (no labels)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tag = {int(i): k for k, i in enumerate(ids)}
    a, b = [tag[int(v)] for v in bonds[:, 0]], [tag[int(v)] for v in bonds[:, 1]]
    n = len(ids)
    _, lab = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)), directed=False)
    e2, L, x = RR.edges2(r_max, nbins), np.asarray(frame["box"]), frame["pos"]
    out = np.zeros(nbins, np.uint64)
    members = {}
    for k in set(a) | set(b):
        members.setdefault(int(lab[k]), []).append(k)
    for m in members.values():
        for u in range(len(m)):
            for v in range(u + 1, len(m)):
                k = int(RR.bin_of(RR.dist2(L, x[m[u]], x[m[v]][None, :]), e2)[0])
                if k >= 0:
                    out[k] += 1
    return out


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("path", ["tiles", "cells"])
def test_reactions_move_types_and_labels(make_gpu, path, prec):
    """The chain-growth melt of smoke() (4000 particles, a reaction step every 10 steps; the first one only changes types and
    states, the second one at step 20 also forms the first bonds): frames inside the run at step 20 -- in front of that step's
    reactions, so with the types and labels its scan reads -- and at step 21, behind them.  The selectors follow the new types;
    the intramolecular part grows by exactly the pairs the new bonds join: it was empty, and behind the reaction it equals the
    histogram of the pairs inside the clusters of the bond list, built from that list without the labels.  (A cluster of three
    joins three pairs with two bonds, so the count is not the number of bonds.)  The system is the melt smoke() runs -- reactions
    that change types, a virtual one, a bond-forming one -- shortened to 4000 particles; react_ref's chains form no clusters
    beyond pairs and change no types.  On the tile scan and on the list scan of the per-cell path."""
    spec = W.reactive_melt(n=4000, seed=21, interval=10)
    sel = [(-1, -1), (0, 1), (0, 2), (1, 2)]
    t, ht = _engine(make_gpu, prec, path, spec)
    t.run(19)
    before = _frame(t)
    t.run(1)
    at20 = _frame(t)
    t.run(1)
    at21 = _frame(t)
    bonds = t.get_list(ht["reaction_bonds"])
    nbonds = len(bonds)
    assert nbonds > 0 and (at20["types"] != before["types"]).sum() > 0 and len(set(before["mol"])) == 4000 > len(set(at20["mol"]))
    g, _ = _engine(make_gpu, prec, path, spec)
    g.rdf_init(1.5, 30, sel, split_molecules=True)
    g.run(19)
    g.rdf_sample_every(1)
    g.run(1)
    f20 = g.rdf()
    _equal(f20, _add(RR.Accumulator(1.5, 30, sel, split=True), at20, types=before["types"], mol=before["mol"]), (prec, "step 20"))
    assert f20["counts"][:, 0].sum() == 0 and f20["counts"][2].sum() > 0            # nothing bonded yet; the D of step 10 are there
    g.rdf_reset()
    g.run(1)
    f21 = g.rdf()
    _equal(f21, _add(RR.Accumulator(1.5, 30, sel, split=True), at21), (prec, "step 21"))
    joined = _joined_pairs_histogram(bonds, t.get_state("ID"), at21, 1.5, 30)
    assert np.array_equal(f21["counts"][0, 0], joined) and joined.sum() >= nbonds and not np.array_equal(f21["counts"][2], f20["counts"][2])
    assert np.array_equal(g.get_state("POS"), at21["pos"]) and np.array_equal(g.get_state("TYPE"), at21["types"])
    g.rdf_sample_every(0)
    g.rdf_reset()
    g.rdf_sample()                                                                      # the explicit frame sees the same state
    _equal(g.rdf(), _add(RR.Accumulator(1.5, 30, sel, split=True), at21), (prec, "explicit"))


@pytest.mark.parametrize("prec", PREC)
def test_density_follows_the_box_of_a_barostat(make_gpu, prec):
    """Berendsen barostat: V_f is the box the forces of the sampled step were evaluated in, i.e. chem_get_box in front of that
    step's scaling.  An explicit frame at the end is compared count by count at the scaled positions."""
    spec = thermal("tiles")
    g, _ = _engine(make_gpu, prec, "tiles", spec, thermostat=False)
    g.barostat_berendsen(2.0, 0.5)
    g.rdf_init(2.0, 40, SEL4)
    g.rdf_sample_every(1)
    acc = RR.Accumulator(2.0, 40, SEL4)
    boxes = []
    for _ in range(4):
        boxes.append(g.box())
        g.run(1)
    assert len({tuple(b) for b in boxes}) == 4
    got = g.rdf()
    types = g.get_state("TYPE")
    want = [np.float64(0.0)] * 4
    for b in boxes:
        for s, sl in enumerate(SEL4):
            want[s] = want[s] + np.float64(RR.norm_pairs(sl, types)) / (b[0] * b[1] * b[2])
    assert got["frames"] == 4 and [int(v) for v in got["pairs"]] == [4 * RR.norm_pairs(sl, types) for sl in SEL4]
    for s in range(4):
        assert RR.ulps(got["density"][s], want[s]) <= 4, (s, got["density"][s], want[s])
    # The histograms of frames taken inside the run.  The positions of such a frame cannot be read back: the step's scaling comes
    # behind it.  Undoing the scaling (x / mu in the box of the step before) reproduces them to rounding -- 1e-15 relative in
    # fp64, half a fixed-point unit (L / 2^32 = 3e-9) per coordinate in fp32 -- so the cumulative histogram N(d2 < e2[k]) of the
    # frame must lie between the reference's at edges moved by -tol and +tol, tol = 1e-10 (fp64) and 1e-6 (fp32) relative: a pair
    # lost or counted twice moves it by one everywhere behind that pair.
    tol = 1e-10 if prec == 64 else 1e-6
    e2 = RR.edges2(2.0, 40)
    for _k in range(2):
        g.rdf_reset()
        b0 = g.box()
        g.run(1)
        got = g.rdf()
        f = _frame(g)
        mu = f["box"] / b0
        assert got["frames"] == 1 and abs(mu[0] - 1.0) > 1e-6
        x = f["pos"] / mu
        d2 = np.concatenate([RR.dist2(b0, x[i], x[i + 1:]) for i in range(len(x) - 1)])
        d2 = np.sort(d2[d2 < 1.01 * e2[-1]])
        cum = np.cumsum(got["counts"][0, 0].astype(np.int64))
        lo, hi = np.searchsorted(d2, e2[1:] * (1.0 - tol), side="left"), np.searchsorted(d2, e2[1:] * (1.0 + tol), side="left")
        assert (lo <= cum).all() and (cum <= hi).all() and (hi - lo).max() <= 8, (prec, cum - lo, hi - cum)
    g.rdf_sample_every(0)
    g.rdf_reset()
    g.rdf_sample()
    _equal(g.rdf(), _add(acc, _frame(g)), (prec, "explicit frame in the scaled box"))


# ---- reset, re-init, off; refusals; checkpoint ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PREC)
def test_reset_reinit_and_off(make_gpu, prec):
    spec = thermal("tiles")
    g, _ = _engine(make_gpu, prec, "tiles", spec, thermostat=False)
    g.rdf_init(2.5, 50, SEL4)
    g.rdf_sample_every(2)
    g.run(4)
    assert g.rdf()["frames"] == 2
    g.rdf_reset()
    z = g.rdf()
    assert z["frames"] == 0 and z["counts"].sum() == 0 and not z["pairs"].any() and not z["density"].any() and not z["g"].any()
    g.run(2)
    assert g.rdf()["frames"] == 1                                     # the configuration and the cadence stay
    g.rdf_init(1.25, 1024, [(0, 1)] * 8, split_molecules=True)       # other bins, the largest histogram; sampling inside the run is off again
    g.run(2)
    assert g.rdf()["frames"] == 0
    g.rdf_sample()
    acc = _add(RR.Accumulator(1.25, 1024, [(0, 1)] * 8, split=True), _frame(g))
    got = g.rdf()
    _equal(got, acc, (prec, "re-init"))
    assert got["counts"].shape == (8, 2, 1024) and np.array_equal(got["counts"][0], got["counts"][7])
    g.rdf_init(1.0, 1, [])                                            # off: the buffers are gone
    for call in (g.rdf, g.rdf_sample, g.rdf_reset, lambda: g.rdf_sample_every(1)):
        with pytest.raises(ChemError) as ei:
            call()
        assert ei.value.code == _capi.ESTATE
    g.run(32)
    h, _ = _engine(make_gpu, prec, "tiles", spec, thermostat=False)      # a context that never sampled
    h.run(40)
    _same_state(_end_state(g), _end_state(h), (prec, "after off"))


def test_refusals(make_gpu):
    spec = thermal("tiles")
    g, _ = _engine(make_gpu, 64, "tiles", spec, thermostat=False)
    for call, what in ((g.rdf, "rdf_get"), (g.rdf_sample, "rdf_sample"), (lambda: g.rdf_sample_every(1), "rdf_sample_every"), (g.rdf_reset, "rdf_reset")):
        with pytest.raises(ChemError) as ei:
            call()
        assert ei.value.code == _capi.ESTATE and what + " before chem_rdf_init" in str(ei.value)
    for args, word in (((0.0, 10, [(-1, -1)]), "r_max"), ((-1.0, 10, [(-1, -1)]), "r_max"), ((float("nan"), 10, [(-1, -1)]), "r_max"),
                       ((float("inf"), 10, [(-1, -1)]), "r_max"), ((2.0, 0, [(-1, -1)]), "nbins"), ((2.0, 1025, [(-1, -1)]), "nbins"),
                       ((2.0, 10, [(-1, -1)] * 9), "npairs"), ((2.0, 10, [(0, 16)]), "type"), ((2.0, 10, [(-2, 0)]), "type")):
        with pytest.raises(ChemError) as ei:
            g.rdf_init(*args)
        assert ei.value.code == _capi.EINVAL and word in str(ei.value), (args, str(ei.value))
    with pytest.raises(ChemError) as ei:
        g.rdf()                                                       # a refused init configures nothing
    assert ei.value.code == _capi.ESTATE
    g.rdf_init(spec["rc"] + 0.25, 10)                                 # accepted: the cutoff can still be set
    for call in (g.rdf_sample, lambda: (g.rdf_sample_every(1), g.run(1))):
        with pytest.raises(ChemError) as ei:
            call()
        assert ei.value.code == _capi.EINVAL and "2.75" in str(ei.value) and "2.5" in str(ei.value) and "max_cutoff" in str(ei.value)
    g.rdf_sample_every(0)
    g.rdf_init(spec["rc"], 10)
    g.rdf_sample()
    res = _capi.RdfResult()
    buf = np.zeros(9, np.uint64)
    assert g.api.rdf_get(g.ctx, _capi.C.byref(res), buf.ctypes.data_as(_capi.C.POINTER(_capi.C.c_uint64)), 9) == _capi.ENOSPC
    assert not buf.any()
    # the all-pairs pass of the paths without tiles is O(N^2): refused by name above 65536 particles
    big = W.lj_melt(n=4 * 26 ** 3, seed=5)
    assert big["n"] > 65536
    h, _ = _engine(make_gpu, 32, "cells", big, thermostat=False)
    h.rdf_init(big["rc"], 10)
    with pytest.raises(ChemError) as ei:
        h.rdf_sample()
    assert ei.value.code == _capi.EINVAL and "65536" in str(ei.value) and "all-pairs" in str(ei.value)
    # a decomposed context is always on the tile path (the engine refuses a slab with tiles = 0 itself), so rdf has no refusal of its own there
    d = make_gpu(64)
    d.set_option("dd_self", 1)
    d.set_option("tiles", 0)
    W.apply(thermal("dd_self"), d, thermostat=False)
    d.rdf_init(2.0, 10)
    with pytest.raises(ChemError) as ei:
        d.rdf_sample()
    assert ei.value.code == _capi.EINVAL and "domain decomposition needs the LDS-staged tiles" in str(ei.value)


@pytest.mark.parametrize("prec", PREC)
def test_a_checkpoint_does_not_hold_the_accumulators(make_gpu, prec):
    """A save in the middle of a sampled run writes the bytes the same run without sampling writes; a load leaves the accumulators
    and the configuration alone."""
    spec = thermal("tiles")
    g, _ = _engine(make_gpu, prec, "tiles", spec, thermostat=False)
    h, _ = _engine(make_gpu, prec, "tiles", spec, thermostat=False)
    g.rdf_init(2.0, 20, SEL4)
    g.rdf_sample_every(3)
    g.run(7)
    h.run(7)
    blob = g.checkpoint_save()
    assert blob == h.checkpoint_save()
    mid = g.rdf()
    assert mid["frames"] == 2
    g.run(5)
    h.run(5)
    _same_state(_end_state(g), _end_state(h), (prec, "after the save"))
    assert g.rdf()["frames"] == 4
    kept = g.rdf()
    g.checkpoint_load(blob)
    back = g.rdf()
    assert back["frames"] == 4 and np.array_equal(back["counts"], kept["counts"]) and back["counts"].sum() > 0
    assert np.array_equal(back["pairs"], kept["pairs"]) and np.array_equal(back["density"].view(np.uint64), kept["density"].view(np.uint64))
    assert (back["r_max"], back["nbins"], back["split"], back["counts"].shape) == (2.0, 20, False, (4, 1, 20))      # the configuration stays
    assert g.step == 7
    g.run(1)                                                          # step 8: the cadence of 3 stays, no frame
    assert g.rdf()["frames"] == 4
    g.run(1)                                                          # step 9 again: its frame is taken again, on top of what was there
    after = g.rdf()
    assert after["frames"] == 5 and (after["counts"] >= back["counts"]).all() and after["counts"].sum() > back["counts"].sum()
