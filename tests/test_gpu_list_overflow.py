"""The cooperative overflow sweep of the list build (option coop_overflow, dev_nlist_tile_f32) changes no result.

A tile of the flagship holds ~578 home particles on a 512-lane workgroup; the ones behind the last full pass are swept by
nine lanes each instead of one.  The force list must come out the same, entry for entry, so every force, trajectory and
event log is bitwise the same with the option on and off -- compared here in one build on a melt with the flagship's cell
edge (list skin 0.49: 15 cells of 2.993 per axis = 125 tiles of 27 cells) at 74 088 particles (a 42^3 lattice in a box of
44.9: density 0.8185 against the flagship's 0.8, ~593 home particles per tile).  CPU check of the size (numpy histogram of
the oracle's positions after 200 steps over the 3x3x3-cell blocks): every one of the 125 tiles holds 560..625 particles."""
import ctypes

import numpy as np
import pytest

from chemlab_amd import workloads as W
from helpers import sorted_events

pytestmark = pytest.mark.gpu

N, EDGE, LIST_SKIN, NC = 74088, 44.9, 0.49, 15


def melt(seed=7, **kw):
    return W.reactive_melt(n=N, rho=N / EDGE ** 3, seed=seed, **kw)


def lattice_pairs(rng, p_z=0.5, p_y=0.5, hubs=0.0):
    """Exclusion (= bond) pairs between neighbours of the 42^3 lattice (ids 1..N, z fastest): every particle gets 0..4
    partners (z and y neighbours, drawn); a share `hubs` of the particles is also tied to its x neighbours and two
    diagonal ones (5..8 partners: beyond the four located slots)."""
    k = 42
    i = np.arange(N)
    z, y, x = i % k, (i // k) % k, i // (k * k)
    out = [np.stack([i, i + 1], 1)[(z < k - 1) & (rng.random(N) < p_z)], np.stack([i, i + k], 1)[(y < k - 1) & (rng.random(N) < p_y)]]
    if hubs > 0:
        h = (rng.random(N) < hubs) & (x > 0) & (x < k - 1) & (y < k - 1) & (z < k - 1)
        for d in (k * k, -k * k, k + 1, k * k + 1):
            out.append(np.stack([i, i + d], 1)[h])
    pairs = np.concatenate(out) + 1
    return np.unique(np.sort(pairs, 1), axis=0)


def crowd(spec, rng):
    """Inert particles (a type without any potential) poured into two tiles: 250 more home particles in one (~843: a
    remainder of ~330, too many for the cooperative pass) and 600 in another (~1190: past two full passes)."""
    spec = dict(spec)
    ce = EDGE / NC
    extra = np.concatenate([rng.uniform(0, 3 * ce, (250, 3)) + 3 * ce * np.array([1, 1, 1]), rng.uniform(0, 3 * ce, (600, 3)) + 3 * ce * np.array([3, 2, 1])])
    m = len(extra)
    spec["n"] = N + m
    spec["ids"] = np.arange(1, N + m + 1)
    spec["types"] = np.concatenate([spec["types"], np.full(m, 3, np.int32)])
    spec["pos"] = np.concatenate([spec["pos"], extra])
    spec["vel"] = np.concatenate([spec["vel"], rng.normal(0, 0.5, (m, 3))])
    spec["mass"] = np.ones(N + m)
    spec["state"] = np.ones(N + m, np.int32)
    spec["res_id"] = np.concatenate([spec["res_id"], spec["res_id"].max() + 1 + np.arange(m, dtype=np.int32)])
    return spec


def tile_counts(eng, pos):
    """(tiles in use, home particles of every 3x3x3-cell block from the positions)."""
    out = (ctypes.c_int32 * 6)()
    eng.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert eng.api.lib.chem_debug_tiles(ctypes.c_void_p(eng.ctx), out) == 0
    assert out[1] == NC, "cells per axis: %d" % out[1]
    t = np.minimum((np.mod(pos, EDGE) / (3 * EDGE / NC)).astype(int), NC // 3 - 1)
    return out[0], np.bincount((t[:, 2] * 5 + t[:, 1]) * 5 + t[:, 0], minlength=125)


def overflow_homes(pos, tiles):
    """Tags of the particles in the last two cell rows (y, z) of the given tiles: the home particles behind the 512th."""
    c = np.minimum((np.mod(pos, EDGE) / (EDGE / NC)).astype(int), NC - 1)
    t = c // 3
    tid = (t[:, 2] * 5 + t[:, 1]) * 5 + t[:, 0]
    last = (c[:, 2] % 3 == 2) & (c[:, 1] % 3 >= 1)
    return np.nonzero(last & np.isin(tid, tiles))[0]


def pair_of_engines(make_gpu, spec, prec, options=(), **kw):
    a, b = make_gpu(prec), make_gpu(prec)
    for e, coop in ((a, 0), (b, 1)):
        h = W.apply(spec, e, **kw)
        e.set_option("list_skin", LIST_SKIN)
        for k, v in options:
            e.set_option(k, v)
        e.set_option("coop_overflow", coop)
    return a, b, h


def same_lists(a, b, tags):
    for tg in tags:
        la, lb = a.debug_force_list(int(tg)), b.debug_force_list(int(tg))
        assert np.array_equal(la, lb), "force list of tag %d differs" % tg


def compare(a, b, spec, steps, sample_seed, min_crowded=63, reactions=False):
    """Lists and forces of the start configuration, then a run across at least five list builds: bitwise."""
    n = spec["n"]
    rng = np.random.default_rng(sample_seed)
    a.run(0); b.run(0)
    ntiles, cnt = tile_counts(b, b.get_state("POS"))
    assert ntiles == 125
    assert (cnt > 512).sum() >= min_crowded, "tiles beyond one pass: %d of %d" % ((cnt > 512).sum(), ntiles)
    pos = a.get_state("POS")
    tags = np.unique(np.concatenate([rng.choice(n, n // 10, replace=False), overflow_homes(pos, [0, 31, 62, 93, 124])]))
    same_lists(a, b, tags)
    assert np.array_equal(a.get_state("FORCE"), b.get_state("FORCE"))
    a.run(steps); b.run(steps)
    assert b.timers()["list_rebuilds"] >= 5 and a.timers()["list_rebuilds"] == b.timers()["list_rebuilds"]
    for what in ("POS_UNFOLDED", "VEL", "FORCE"):
        assert np.array_equal(a.get_state(what), b.get_state(what)), what
    same_lists(a, b, tags[::8])
    if reactions:
        ea, eb = sorted_events(a.get_events()), sorted_events(b.get_events())
        assert len(eb) > 100 and ea == eb
    return cnt


@pytest.mark.parametrize("prec", [32, 64])
def test_melt_same_lists_forces_trajectory(make_gpu, prec):
    spec = melt()
    a, b, _ = pair_of_engines(make_gpu, spec, prec, reactions=False)
    cnt = compare(a, b, spec, 100, 1)
    print("home particles per tile: min %d mean %.1f max %d" % (cnt.min(), cnt.mean(), cnt.max()))


@pytest.mark.parametrize("hubs", [0.0, 0.03])
def test_exclusions_located_and_generic(make_gpu, hubs):
    """1..4 exclusions per particle (partners located as slots); with hubs some particles carry 5..8 (generic sweep)."""
    spec = melt(seed=8)
    spec["exclusions"] = lattice_pairs(np.random.default_rng(3), hubs=hubs)
    deg = np.bincount(spec["exclusions"].ravel(), minlength=N + 1)[1:]
    assert (deg[deg > 0] <= 4).all() if hubs == 0 else ((deg >= 5) & (deg <= 8)).sum() > 1000
    a, b, _ = pair_of_engines(make_gpu, spec, 32, reactions=False)
    compare(a, b, spec, 100, 2)


@pytest.mark.parametrize("bond_pass", [0, 1])
def test_inline_bonds(make_gpu, bond_pass):
    """Bonds = exclusions, evaluated by the force kernel from the slots the list build records (bond_pass 0) or ignores
    (bond_pass 1: the force launch behind a rebuild records them)."""
    spec = melt(seed=9)
    bonds = lattice_pairs(np.random.default_rng(4), p_z=0.4, p_y=0.3, hubs=0.02)
    spec["exclusions"] = bonds
    spec["lists"] = [dict(arity=2, kind="HARMONIC", params=[30.0, 1.05], ids=bonds)]
    a, b, _ = pair_of_engines(make_gpu, spec, 32, options=(("bonds_inline", 1), ("bond_pass", bond_pass)), reactions=False)
    compare(a, b, spec, 100, 3)


@pytest.mark.parametrize("excl", [False, True])
def test_slab_path(make_gpu, excl):
    """The standalone list kernel of the decomposed path (one rank, its own z neighbour)."""
    spec = melt(seed=10)
    if excl:
        spec["exclusions"] = lattice_pairs(np.random.default_rng(5), hubs=0.02)
    a, b, _ = pair_of_engines(make_gpu, spec, 32, options=(("dd_self", 1),), reactions=False)
    compare(a, b, spec, 100, 4)


def test_crowded_tiles_fall_back_to_ordinary_passes(make_gpu):
    rng = np.random.default_rng(6)
    spec = crowd(melt(seed=11), rng)
    a, b, _ = pair_of_engines(make_gpu, spec, 32, reactions=False)
    cnt = compare(a, b, spec, 100, 5)
    assert cnt.max() > 1024 and ((cnt > 512 + 113) & (cnt < 1024)).any()


def test_reactive_run_same_events(make_gpu):
    spec = melt(seed=12, interval=10, rate=50.0)
    a, b, _ = pair_of_engines(make_gpu, spec, 32)
    compare(a, b, spec, 100, 6, reactions=True)
