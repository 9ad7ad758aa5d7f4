"""Anisotropic boxes, empty regions and cell-count thresholds: the HIP path where the rest of the suite never goes.

Every other GPU parity test runs on a near-cubic, homogeneously filled box.  The engine chooses its list / force path per
axis from floor(L_d / (rc + skin)) (brute force below 3 cells on any axis, per-cell kernels below 5, LDS tiles from 5), sizes
its tile and slab capacities from MEAN occupancies, and in the fp32 build keeps positions as int32 fixed point with a
per-axis scale.  Here: a ladder of cell counts on and between the thresholds, filled uniformly or with a droplet that wraps
the corner; films and droplets under the slab decomposition, with ranks that own nothing; reactions and bonded terms
beside vacuum; 60 particles in the headline box.  Static results are compared with numpy (helpers.brute_pairs,
helpers.pair_reference: all pairs, minimum image, no cells) because the oracle shares the engine's cell scheme;
tests/test_oracle_geometry.py checks the oracle against the same numpy results on the CPU, trajectories use the oracle.
"""
import ctypes

import numpy as np
import pytest

import helpers as H
from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import force_error_without_cutoff_flips, sorted_events
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks, both

pytestmark = pytest.mark.gpu

_ID = lambda nc: "%dx%dx%d" % tuple(nc)      # noqa: E731


def _path(g):
    """(tile count, cells along x) of the engine's geometry: no tiles on the per-cell and brute-force paths, no cells on the
    brute-force path (Box::nc = 0)."""
    out = (ctypes.c_int32 * 6)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    return int(out[0]), int(out[1])


def _ntiles(g):
    return _path(g)[0]


def _check_static(g, spec, ref, prec, what):
    """List, forces, epot_lj and virial_nb of the engine (run(0) done) against numpy."""
    diff = H.list_difference(g.get_verlet_pairs(), spec)
    if prec == 64:
        assert not diff, (what, sorted(diff)[:5])
    else:
        assert diff <= spec["shell_pairs"], (what, sorted(diff - spec["shell_pairs"])[:5])
    f, elj, _, vir = ref
    fg = g.get_state("FORCE")
    if prec == 64:
        err = rel_err(fg, f)
        print("%s fp64: force %.2e" % (what, err))
        assert err < TOL[64], (what, err)
    else:
        err, flips = force_error_without_cutoff_flips(spec, fg, f, TOL_MELT32, max_flips=len(spec["shell_pairs"]))
        print("%s fp32: force %.2e, %d flips" % (what, err, flips))
        assert err < TOL_MELT32 and 0 <= flips <= len(spec["shell_pairs"]), (what, err, flips)
    og = g.observe()
    print("%s fp%d: epot_lj %.2e virial_nb %.2e" % (what, prec, abs(og["epot_lj"] / elj - 1), abs(og["virial_nb"] / vir - 1)))
    assert og["epot_lj"] == pytest.approx(elj, rel=1e-10 if prec == 64 else 2e-5), what
    assert og["virial_nb"] == pytest.approx(vir, rel=1e-10 if prec == 64 else 2e-5), what


# ---- (a) the cell-count ladder, static ----------------------------------------------------------------------------------
_VARIANTS = [(nc, {}) for nc in H.LADDER_BOXES]
_VARIANTS += [(nc, opt) for nc in H.LADDER["tiles"] for opt in ({"tiles": 0}, {"fused_rebuild": 0})]
_VARIANTS += [((12, 5, 5), {"tile_split": 11})]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("fill", ["uniform", "corner_droplet"])
@pytest.mark.parametrize("frac", [0.5, 0.0])
@pytest.mark.parametrize("nc,opts", _VARIANTS, ids=lambda v: _ID(v) if isinstance(v, tuple) else ("+".join("%s=%d" % kv for kv in v.items()) or "default"))
def test_geometry_ladder_static_against_numpy(make_gpu, nc, opts, frac, fill, prec):
    """Boxes of (nc + frac) cells per axis, frac 0.5 and 0.0 (an edge that is an exact multiple of rc + skin): two cells on an
    axis (brute force), three or four (per-cell kernels, among them (3, 40, 3) and the mixed (3, 5, 9)), five and more (LDS
    tiles, with rows whose last tile is partial in x, y and z at once: (5, 6, 7), (7, 5, 5), (5, 5, 23)).  The tile boxes also
    with tiles off, with the unfused rebuild chain and, (12, 5, 5), with narrow tiles at the end of a row.  ntiles says
    which path ran."""
    spec = H.ladder_spec(nc, frac, fill)
    g = make_gpu(prec)
    for k, v in opts.items():
        g.set_option(k, v)
    W.apply(spec, g)
    g.run(0)
    ntiles, ncx = _path(g)
    assert (ntiles > 0) == (min(nc) >= 5 and opts.get("tiles", 1) != 0), (nc, opts, ntiles)
    assert ncx == (nc[0] if min(nc) >= 3 else 0), (nc, ncx)         # two cells on an axis: the brute-force list, not the per-cell kernels
    _check_static(g, spec, H.geometry_reference("ladder", nc, frac, fill), prec, (nc, frac, fill, opts))


def test_geometry_ladder_plan_is_the_host_headers(make_gpu, tmp_path):
    """CtxT runs the plan of chem_geom_host.hpp: after run(0) the six numbers of chem_debug_tiles (tiles, cells along x, wide
    tiles per row, narrow width, tile rows, tile capacity) are what tests/host/geometry_harness.cpp makes of the same box,
    cutoff, skin and particle count, with an unlimited LDS budget (stencils of at most 1800 slots).  The ladder's boxes hold a
    few hundred particles: the smallest that reach the brute-force, per-cell and tile paths; tests/test_host_geometry.py
    checks the header's rules themselves on the CPU."""
    exe = H.compile_geometry_harness(tmp_path)
    variants = [(nc, {}) for nc in H.LADDER_BOXES] + [((12, 5, 5), {"tile_split": 11})]
    assert len(variants) == 13
    specs = [H.ladder_spec(nc, 0.5, "uniform") for nc, _ in variants]
    plans = H.run_harness(exe, [H.plan_line(spec, **opts) for spec, (_, opts) in zip(specs, variants)])
    for spec, (nc, opts), plan in zip(specs, variants, plans):
        g = make_gpu(32)
        for k, v in opts.items():
            g.set_option(k, v)
        W.apply(spec, g)
        g.run(0)
        out = (ctypes.c_int32 * 6)()
        g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
        assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
        assert plan[0] == "tiles" and list(out) == [int(v) for v in plan[1:7]], (nc, opts, list(out), plan)
        assert 0 <= out[5] <= 1800


# ---- (b) the ladder, dynamic ----------------------------------------------------------------------------------------------
_TRAJ = {}


def _oracle_run(make_oracle, key, spec, steps, **kw):
    """The oracle's state after run(0) and after `steps` steps, computed once per spec for all the tests that use it."""
    if key not in _TRAJ:
        o = make_oracle()
        W.apply(spec, o, **kw)
        o.run(0)
        res = dict(obs0=o.observe())
        o.run(steps)
        res.update(x=o.get_state("POS_UNFOLDED"), v=o.get_state("VEL"), img=o.get_state("IMAGE"), reb=o.timers()["rebuilds"])
        _TRAJ[key] = res
    return _TRAJ[key]


def _check_trajectory(prec, x, v, img, reb, ref, what, band=True):
    err = rel_err(x, ref["x"])
    print("%s fp%d: POS_UNFOLDED %.2e VEL %.2e rebuilds %d / %d" % (what, prec, err, rel_err(v, ref["v"]), reb, ref["reb"]))
    if prec == 64:
        assert np.array_equal(img, ref["img"]), what
        assert err < 1e-8, (what, err)
        assert rel_err(v, ref["v"]) < 1e-6, what
        if band:      # the sweep's band for the rebuild count (single domain: on slabs the host's direct rebuilds count too)
            assert ref["reb"] <= reb <= ref["reb"] + 4, (what, reb, ref["reb"])
    else:
        assert err < 2e-4, (what, err)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("frac", [0.5, 0.0])
@pytest.mark.parametrize("nc", H.LADDER_BOXES, ids=_ID)
def test_geometry_ladder_droplet_trajectory(make_gpu, make_oracle, nc, frac, prec):
    """The droplet boxes of the ladder, 300 NVE steps (20 to 35 rebuilds, dozens of particles through a face -- asserted on
    the oracle in tests/test_oracle_geometry.py): images, unfolded positions, velocities and the rebuild count."""
    spec = H.ladder_spec(nc, frac, "corner_droplet")
    ref = _oracle_run(make_oracle, ("ladder", nc, frac), spec, H.LADDER_STEPS)
    g = make_gpu(prec)
    W.apply(spec, g)
    g.run(H.LADDER_STEPS)
    _check_trajectory(prec, g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("IMAGE"), g.timers()["rebuilds"], ref, (nc, frac))


# ---- (c) empty regions under the slab decomposition -------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name", ["self_film_z", "self_film_x", "self_droplet"])
def test_geometry_slab_self_films_and_droplet(make_gpu, make_oracle, name, prec):
    """(5, 5, 23) cells as ONE slab that is its own z-neighbour: a film across the periodic z face, a film across the x face
    (empty cell columns in every layer, ghost layers included), a droplet on the corner.  G, the migration buffers and the
    slab capacity come from the mean layer occupancy n / 23; the film's layers hold 11 times that."""
    spec = H.slab_spec(name)
    ref = _oracle_run(make_oracle, ("slab", name), spec, H.LADDER_STEPS)
    g = make_gpu(prec)
    g.set_option("dd_self", 1)
    W.apply(spec, g)
    g.run(0)
    assert _ntiles(g) > 0
    _check_static(g, spec, H.geometry_reference("slab", name), prec, name)
    assert g.observe()["ekin"] == pytest.approx(ref["obs0"]["ekin"], rel=1e-12 if prec == 64 else 1e-6)
    g.run(H.LADDER_STEPS)
    x, v, img = g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("IMAGE")
    _check_trajectory(prec, x, v, img, g.timers()["rebuilds"], ref, name, band=False)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name", ["empty_rank_P2", "empty_rank_P3", "face_P2", "face_P3"])
def test_geometry_slab_ranks_that_own_nothing(make_gpu, make_oracle, name, prec):
    """Two and three slabs in this process, a film two layers thick with a bulk velocity of 7 along z.  empty_rank: the film
    ends 0.2 layers below the boundary of rank 0 and rank 1, every other rank owns NOTHING at step 0; within the run rank 1
    receives its first particles by migration and rank 0 is emptied (rank 2 of three stays empty throughout, with two empty
    ghost layers).  face: the film straddles the periodic z face, owned by rank P-1 and rank 0, and ends on rank 0 with an
    image increment.  tests/test_oracle_geometry.py asserts both journeys on the oracle's trajectory.

    A real count of 0, read from chem_api.hip before this ran: upload_particles leaves n = 0 with the capacities intact
    (they come from nglob); rebuild_dd sizes k_bin, k_place and k_copyback with max(1, ...) and guards k_append_arrivals and
    k_ghost_rtag by their counts, k_scan_cells / k_sort_gather / k_layer_counts / k_ghost_cells / k_tile_desc / the list and
    force launches are sized by cells or tiles, the exchanges carry zero-byte messages next to the fixed-size headers.
    NOT clamped: launch_integrate (cdiv(n, kIntPerBlock) blocks), k_kinetic in observe and rescale_velocities, k_bonded --
    a grid of 0 blocks, which the runtime refuses without launching; hipLaunchKernelGGL's status is not read, there is
    nothing for those kernels to do, and the per-step decision of an empty rank (fold words, block maxima) reads zeros.
    So an empty rank neither faults nor leaves its neighbours waiting; this test is the evidence on the device."""
    P = H.SLAB_CASES[name][4][0]
    spec = H.slab_spec(name)
    ref = _oracle_run(make_oracle, ("slab", name), spec, H.LADDER_STEPS)
    numpy_ref = H.geometry_reference("slab", name)
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        W.apply(spec, g)
        g.run(0)
        res = dict(vp=g.get_verlet_pairs(), f=g.get_state("FORCE"), obs=g.observe())
        g.run(H.LADDER_STEPS)
        res.update(x=g.get_state("POS_UNFOLDED"), v=g.get_state("VEL"), img=g.get_state("IMAGE"), reb=g.timers()["rebuilds"])
        return res
    out = _run_ranks(P, rank)

    class _Static:      # what _check_static reads of an engine, from the values rank r returned
        def __init__(self, r): self.r = r
        def get_verlet_pairs(self): return self.r["vp"]
        def get_state(self, what): return self.r["f"]
        def observe(self): return self.r["obs"]
    for r in range(P):
        _check_static(_Static(out[r]), spec, numpy_ref, prec, (name, r))
        assert out[r]["obs"]["epot_lj"] == pytest.approx(ref["obs0"]["epot_lj"], rel=1e-10 if prec == 64 else 2e-5)
        assert out[r]["obs"]["ekin"] == pytest.approx(ref["obs0"]["ekin"], rel=1e-12 if prec == 64 else 1e-6)
        _check_trajectory(prec, out[r]["x"], out[r]["v"], out[r]["img"], out[r]["reb"], ref, (name, r), band=False)


# ---- (d) reactions and bonded terms beside vacuum ---------------------------------------------------------------------
def _film_of_reactive_melt():
    spec = W.reactive_melt(n=4096, seed=41, interval=10)
    spec["box"] = [spec["box"][0], spec["box"][1], 2.5 * spec["box"][2]]       # positions untouched: a free-standing film
    spec["rebuild_criterion"] = 1
    return spec


def _reactive_result(g, h):
    return dict(ev=sorted_events(g.get_events()), bonds=g.get_list(h["reaction_bonds"]), st=g.get_state("STATE"), ty=g.get_state("TYPE"),
                x=g.get_state("POS_UNFOLDED"))


def _oracle_reactive(make_oracle):
    if "reactive" not in _TRAJ:
        spec = _film_of_reactive_melt()
        o = make_oracle()
        h = W.apply(spec, o)
        for _ in range(4):
            o.run(10)
        _TRAJ["reactive"] = _reactive_result(o, h)
    return _TRAJ["reactive"]


@pytest.mark.parametrize("mode", ["single", "dd_self", "P2", "single_fp32"])
def test_geometry_reactive_film_beside_vacuum(make_gpu, make_oracle, mode):
    """reactive_melt (4096 monomers, Langevin, four reaction steps) in a box 2.5 times as long along z: 6 x 6 x 15 cells of
    which 9 layers are empty, cells 2.5 times fuller than the mean the tile capacity is sized from, candidates at a free
    surface; with two slabs rank 1 owns nothing at step 0."""
    spec = _film_of_reactive_melt()
    ref = _oracle_reactive(make_oracle)
    assert len(ref["ev"]) > 500
    prec = 32 if mode == "single_fp32" else 64
    P = 2 if mode == "P2" else 1
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        if mode == "dd_self":
            g.set_option("dd_self", 1)
        if P > 1:
            g.comm_init_local(P, r, hub)
        h = W.apply(spec, g)
        for _ in range(4):
            g.run(10)
        return _reactive_result(g, h)
    for res in (_run_ranks(P, rank) if P > 1 else [rank(0)]):
        sg, so = set(e[:4] for e in res["ev"]), set(e[:4] for e in ref["ev"])
        print("reactive film %s: %d events, %d differ, POS_UNFOLDED %.2e" % (mode, len(so), len(sg ^ so), rel_err(res["x"], ref["x"])))
        if prec == 64:
            assert [e[:4] for e in res["ev"]] == [e[:4] for e in ref["ev"]]
            assert np.array_equal(res["bonds"], ref["bonds"])
            assert np.array_equal(res["st"], ref["st"]) and np.array_equal(res["ty"], ref["ty"])
            assert rel_err(res["x"], ref["x"]) < 1e-8
        else:
            assert len(sg ^ so) <= max(4, len(so) // 100), (len(sg ^ so), len(so))


@pytest.mark.parametrize("prec", [64, 32])
def test_geometry_trimer_melt_in_a_box_doubled_along_x_and_z(make_gpu, make_oracle, prec):
    """trimer_melt (bonds, angles, exclusions, end-group coupling) filling a quarter of its box: the molecules at the free
    surfaces have their bonded partners and excluded pairs beside empty cells.  Tolerances: fp64 those of
    test_random_trimer_melt_topology_matches_oracle (lists bit for bit, positions 1e-8, epot_list 1e-8) and TOL[64] for the
    forces; fp32 the suite's own for K = 30 bonds -- forces TOL_MELT32 with cutoff decisions set apart, epot_list 1e-5 as in
    test_tabulated_and_bonded_polymer, positions 2e-4."""
    spec = W.trimer_melt(n_mol=512, seed=43, interval=20)
    spec["box"] = [2 * spec["box"][0], spec["box"][1], 2 * spec["box"][2]]
    g, o, h = both(make_gpu, make_oracle, spec, prec)
    g.run(0); o.run(0)
    fg, fo = g.get_state("FORCE"), o.get_state("FORCE")
    og, oo = g.observe(), o.observe()
    if prec == 64:
        print("trimer fp64: force %.2e" % rel_err(fg, fo))
        assert rel_err(fg, fo) < TOL[64]
        assert np.allclose(og["epot_list"], oo["epot_list"], rtol=1e-8)
    else:
        # (run(0) under Langevin leaves the same keyed noise in both forces; the pair part is what differs)
        err, flips = force_error_without_cutoff_flips(spec, fg, fo, TOL_MELT32, max_flips=8)
        print("trimer fp32: force %.2e, %d flips" % (err, flips))
        assert err < TOL_MELT32 and 0 <= flips <= 8, (err, flips)
        assert np.allclose(og["epot_list"], oo["epot_list"], rtol=1e-5)
    assert og["list_size"] == oo["list_size"]
    g.run(60); o.run(60)
    err = rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED"))
    print("trimer fp%d: POS_UNFOLDED %.2e after 60 steps, %d events" % (prec, err, len(o.get_events())))
    assert len(o.get_events()) > 5
    if prec == 64:
        assert [e[:4] for e in sorted_events(g.get_events())] == [e[:4] for e in sorted_events(o.get_events())]
        for k in (0, 1, "reaction_bonds"):
            assert np.array_equal(g.get_list(h[k]), o.get_list(h[k])), k
        assert np.array_equal(g.get_exclusions(), o.get_exclusions())
        assert err < 1e-8
        assert np.allclose(g.observe()["epot_list"], o.observe()["epot_list"], rtol=1e-8)
    else:
        assert err < 2e-4


# ---- (e) the big sparse box ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
def test_geometry_cluster_in_the_headline_box(make_gpu, make_oracle, prec):
    """57 particles around the corner of a box of edge 108 (38 cells per axis, about 2200 tiles, all but eight of them
    empty).  At this edge an absolute fp32 coordinate has an ulp of 7.6e-6; the tile-local staging of the fixed-point
    positions is what keeps the fp32 forces within TOL[32], and nothing tests it more cheaply.  Then 200 steps."""
    spec = H.cluster_spec()
    f, elj, _, vir = H.geometry_reference("cluster")
    ref = _oracle_run(make_oracle, ("cluster",), spec, 200)
    g = make_gpu(prec)
    W.apply(spec, g)
    g.run(0)
    assert _ntiles(g) > 2000
    assert not H.list_difference(g.get_verlet_pairs(), spec)          # (min_gap is 2e-3 here: no shell)
    err = rel_err(g.get_state("FORCE"), f)
    print("cluster fp%d: force %.2e" % (prec, err))
    assert err < TOL[prec], err
    og = g.observe()
    assert og["epot_lj"] == pytest.approx(elj, rel=1e-10 if prec == 64 else 2e-5)
    assert og["virial_nb"] == pytest.approx(vir, rel=1e-10 if prec == 64 else 2e-5)
    g.run(200)
    _check_trajectory(prec, g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("IMAGE"), g.timers()["rebuilds"], ref, "cluster")


def test_geometry_cluster_forces_do_not_depend_on_where_it_sits_fp32(make_gpu):
    """The same cluster translated by half a box on every axis: the pair geometry is unchanged, only the absolute coordinates
    (and the tiles that hold them) differ -- fp32 forces agree within 2 * TOL[32]."""
    spec = H.cluster_spec()
    L = np.asarray(spec["box"])
    moved = dict(spec, pos=np.mod(np.asarray(spec["pos"]) + 0.5 * L, L))
    a, b = make_gpu(32), make_gpu(32)
    W.apply(spec, a); W.apply(moved, b)
    a.run(0); b.run(0)
    err = rel_err(b.get_state("FORCE"), a.get_state("FORCE"))
    print("cluster fp32: corner against centre %.2e" % err)
    assert err < 2 * TOL[32], err
