"""The bond pass ("Inline bonds"): the list build ignores the exclusions, the LDS slots of every home
particle's bonded partners are recorded once per list build -- by workgroups of the fused rebuild that have run out of tiles
(dev_bond_slots_tile, single domain) or by k_bond_slots behind the list launch (slabs; single domain with option
bond_slots_kernel = 1) -- and every force launch up to the next build evaluates the bonds from them.

What is checked, per case:
  * the forces of the step of a forced list build (run(0): the host's rebuild_now) and of the step after it (the recorded slots
    read back by a launch that has not built them) against the oracle on the very same configuration, at the tolerance of the
    existing inline-bond tests (test_gpu_parity.TOL; the reactive melt in fp64 only, see there);
  * the same forces and a 200-step trajectory, bit for bit, between the two routes.  A forced build of the single domain is a
    launch of the fused rebuild like any other, so the second route is the stand-alone kernel (bond_slots_kernel = 1); both runs
    hold the device's own builds and builds the host forces through rebuild_now, at the same steps;
  * DevCtl::bond_slot_miss and excl_slot_error stay 0: run() reads the control block at its end and raises on either.

Shapes (star molecules, one per lattice site, the lattice shifted across the periodic boundary; rc + skin = 2.8):
  k = 5  five cells per axis, the smallest box that is given tiles (8 tiles: 3 + 2 cells per axis, every tile an edge tile);
  k = 7  seven cells per axis: not a multiple of the 3-cell tile edge (27 tiles, edge tiles of one cell, partners across the wrap);
  arms 1-4: first quad only; 5-8: second quad; 3, 6 and 10: centres beyond the eight recorded slots stay with the work list
  (the host then keeps the bond pass off and the list build records, as before);
  one reactive melt of 4000 particles (five cells per axis) whose bonds and exclusions grow during the run."""
import ctypes

import numpy as np
import pytest

from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import sorted_events
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                 [1, 1, 1], [-1, -1, 1], [1, -1, -1], [-1, 1, -1]], float)
DIRS /= np.linalg.norm(DIRS, axis=1)[:, None]
SPACING = {5: 3.3, 7: 3.0}      # lattice constant of the molecules: box edges 16.5 and 21.0 = 5 and 7 cells of at least 2.8


def stars(k, arms, seed=17):
    """k^3 star molecules, molecule m with arms[m % len(arms)] arms bonded (= excluded) to its centre."""
    a0 = SPACING[k]
    rng = np.random.default_rng(seed)
    L = k * a0
    sites = (np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3) + 0.5) * a0
    pos, bonds = [], []
    for m, c in enumerate(sites):
        na = arms[m % len(arms)]
        i0 = len(pos) + 1
        pos.append(c)
        for a in range(na):
            pos.append(c + DIRS[a])
            bonds.append((i0, i0 + 1 + a))
    pos = np.array(pos) + rng.uniform(-0.05, 0.05, (len(pos), 3))
    pos = np.mod(pos + 1.6, L)      # molecules astride the periodic boundary
    n = len(pos)
    bonds = np.array(bonds)
    return dict(n=n, box=[L] * 3, rc=2.5, skin=0.3, dt=0.002, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32), pos=pos,
                vel=rng.normal(0, 0.6, (n, 3)), mass=np.ones(n), lj=[(0, 0, 0.5, 0.9, 2.5)], kT=1.0, gamma=0.0, seed=1,
                lists=[dict(arity=2, kind="HARMONIC", params=[40.0, 1.0], ids=bonds)], exclusions=bonds, rebuild_criterion=0)


def cells_per_axis(g):
    out = (ctypes.c_int32 * 6)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    return out[1], out[0]      # cells along x, tiles


def engine(make_gpu, spec, prec, options=(), **kw):
    g = make_gpu(prec)
    for k, v in options:
        if k.startswith("dd_self"):      # (before anything else: it picks the transport)
            g.set_option(k, v)
    h = W.apply(spec, g, **kw)
    for k, v in options:
        if not k.startswith("dd_self"):
            g.set_option(k, v)
    return g, h


def force_error(make_oracle, spec, g, prec, lists=None, exclusions=None):
    """g's forces against the oracle's on the configuration g holds now."""
    spec2 = dict(spec, pos=g.get_state("POS"), vel=g.get_state("VEL"), types=g.get_state("TYPE"))
    if lists is not None:
        spec2["lists"], spec2["exclusions"], spec2["state"] = lists, exclusions, g.get_state("STATE")
    o = make_oracle()
    W.apply(spec2, o, thermostat=False, reactions=False)
    o.run(0)
    fg, fo = g.get_state("FORCE"), o.get_state("FORCE")
    err = rel_err(fg, fo)
    print("fp%d against the oracle: force error %.3e (max |F| %.1f)" % (prec, err, np.abs(fo).max()))
    return fg, err


def forces_at_a_build_and_behind_it(make_oracle, spec, g, prec, **kw):
    g.run(0)      # the host's forced build (rebuild_now) and the force launch behind it
    r0 = g.timers()["list_rebuilds"]
    fa, err = force_error(make_oracle, spec, g, prec, **kw)
    assert err < TOL[prec]
    g.run(1)      # the step after: the slots of that build, read by a launch that has not recorded them
    assert g.timers()["list_rebuilds"] == r0
    fb, err = force_error(make_oracle, spec, g, prec, **kw)
    assert err < TOL[prec]
    return fa, fb


def same_bits(a, b):
    for what in ("FORCE", "POS_UNFOLDED", "VEL"):
        assert np.array_equal(a.get_state(what), b.get_state(what)), what


def routes_agree(a, b, steps=200, forced=(30, 31)):
    """a: the fused rebuild's tail; b: k_bond_slots.  The same steps, the host's forced builds at the same ones."""
    a.run(0); b.run(0)
    same_bits(a, b)
    r0 = a.timers()["list_rebuilds"]
    done = 0
    for stop in list(forced) + [steps]:
        a.run(stop - done); b.run(stop - done)
        done = stop
        same_bits(a, b)
        if stop < steps:
            for e in (a, b):
                e.set_option("bond_pass", 1)      # (marks the lists stale: the next run() starts with rebuild_now)
    ta, tb = a.timers(), b.timers()
    assert ta["list_rebuilds"] == tb["list_rebuilds"]
    assert ta["list_rebuilds"] - r0 >= len(forced) + 1, "list builds in the run: %d" % (ta["list_rebuilds"] - r0)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("k,arms", [(5, (1, 2, 3, 4)), (5, (5, 6, 7, 8)), (7, (1, 2, 3, 4)), (7, (5, 6, 7, 8)), (7, (3, 6, 10))],
                         ids=["smallest-1to4", "smallest-5to8", "edge-1to4", "edge-5to8", "edge-worklist"])
def test_star_molecules_single_domain(make_gpu, make_oracle, k, arms, prec):
    spec = stars(k, arms)
    a, _ = engine(make_gpu, spec, prec, thermostat=False)
    b, _ = engine(make_gpu, spec, prec, options=(("bond_slots_kernel", 1),), thermostat=False)
    fa = forces_at_a_build_and_behind_it(make_oracle, spec, a, prec)
    assert cells_per_axis(a)[0] == k
    b.run(0)
    assert np.array_equal(fa[0], b.get_state("FORCE"))
    b.run(1)
    assert np.array_equal(fa[1], b.get_state("FORCE"))
    routes_agree(a, b)


@pytest.mark.parametrize("prec", [32, 64])
def test_reactive_melt_in_the_smallest_box(make_gpu, make_oracle, prec):
    """Bonds and exclusions that grow at every reaction interval; the forced builds of the reaction steps are rebuild_now's."""
    spec = W.reactive_melt(n=4000, seed=12, interval=10)
    spec["rebuild_criterion"] = 0
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e9
    a, ha = engine(make_gpu, spec, prec)
    b, hb = engine(make_gpu, spec, prec, options=(("bond_slots_kernel", 1),))
    routes_agree(a, b)
    assert cells_per_axis(a)[0] == 5
    assert sorted_events(a.get_events()) == sorted_events(b.get_events()) and len(a.get_events()) > 1000
    bonds = a.get_list(ha["reaction_bonds"])
    assert np.array_equal(bonds, b.get_list(hb["reaction_bonds"])) and len(bonds) > 100
    # the configuration the run has reached, with its bonds: forces at a build and behind it against the oracle
    lists = [dict(arity=2, kind="HARMONIC", params=[30.0, 0.97], ids=bonds)]
    excl = a.get_exclusions()
    spec2 = dict(spec, pos=a.get_state("POS"), vel=a.get_state("VEL"), types=a.get_state("TYPE"), state=a.get_state("STATE"),
                 lists=lists, exclusions=excl)
    c, _ = engine(make_gpu, spec2, prec, thermostat=False, reactions=False)
    # fp64 only.  In fp32 the force kernel takes the bonded partners' pair term out of sums that hold it (bond_mode 2); at rate
    # 1e9 bonds form between overlapping particles whose pair term is several hundred, the largest net force is 70, and the
    # rounding of that cancellation is 2.35e-5 of it -- measured against the oracle and against the fp32 bonded kernel alike,
    # with the slots recorded by the force kernel (the library before this change: bit-identical states) and by the rebuild.
    # The slots are what this file is about: a wrong one is an error of order one, which the fp64 comparison would show, and
    # the fp32 routes are compared bit for bit above; the fp32 forces against the oracle are checked on the star molecules.
    if prec == 64:
        forces_at_a_build_and_behind_it(make_oracle, spec2, c, prec, lists=lists, exclusions=excl)
    else:
        c.run(0); c.run(1)      # (the two flags: run() raises on either)


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("path", ["unfused", "dd_self"])
def test_star_molecules_on_the_other_list_builds(make_gpu, make_oracle, path, prec):
    """The unfused chain (fused_rebuild = 0) and one slab that is its own z-neighbour (k_bond_slots behind the slab's list
    launch, ghost partners through the ghost tag map): forces at a build and behind it, then a trajectory against the oracle."""
    spec = stars(7, (1, 2, 3, 4, 5, 6, 7, 8))
    g, _ = engine(make_gpu, spec, prec, options=((("fused_rebuild", 0),) if path == "unfused" else (("dd_self", 1),)), thermostat=False)
    forces_at_a_build_and_behind_it(make_oracle, spec, g, prec)
    o = make_oracle()
    W.apply(spec, o, thermostat=False)
    o.run(61); g.run(60)
    assert g.timers()["list_rebuilds"] >= 2
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-9 if prec == 64 else 1e-4)
