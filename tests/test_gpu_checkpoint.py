"""Checkpoint and exact restart on the device (include/chem_mi355.h chem_checkpoint_save / chem_checkpoint_load).

The contract: A runs run(a), saves, runs run(b); B repeats A's set-up calls -- with the positions of step 0 and zero velocities,
so that nothing of B's own survives by accident --, loads, runs run(b).  From the load on every getter agrees, floating-point
values bit for bit (np.array_equal, no tolerance: both contexts upload the same host data and build their lists from it).

melt            the smallest boxes of tests/test_gpu_geometry.py's ladder that reach the LDS tiles (5 x 5 x 5 cells), the per-cell
                lists (the same box, tiles = 0) and the brute-force list (2 x 7 x 7), Langevin on, both precisions; the tile box
                also under the accumulated rebuild criterion (the neighbour launch only on steps that can need a rebuild).  a is
                found step by step from chem_get_timers: the list was built at least once after step 0 and is three steps old at
                the save, so the restart cannot lean on a fresh list; b ends behind the second list build that follows.
everything      the reactive melt with fixed distances and the Langevin piston of tests/test_gpu_piston.py's coexistence test, plus
                a hybrid bond list, spawned angles, a resolution ramp on the particles a reaction converts, a typed fix set that
                releases them, and ATRP.  Saved at step 53 (reaction interval 10, ATRP interval 7), three reaction steps
                behind the first bonds, so that chains of three exist and angles have been spawned.
idempotence     save(B) right after the load is the loaded blob; two saves of A with nothing between them are equal.
refusals        a decomposed context, another precision, a context with one list more: by name, and the run that follows is the
                run without the attempt."""
import ctypes

import numpy as np
import pytest
from scipy.spatial import cKDTree

import aged_ref as AR
import helpers as H
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError

pytestmark = pytest.mark.gpu

PER_PARTICLE = ("POS", "IMAGE", "VEL", "FORCE", "TYPE", "STATE", "MOLID", "RESID", "CHARGE", "MASS", "POS_UNFOLDED")


def _path(g):
    """(tile count, cells along x): no tiles on the per-cell and brute-force paths, no cells on the brute-force path"""
    out = (ctypes.c_int32 * 6)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    return int(out[0]), int(out[1])


def _same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], "%s[%s]" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, k))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _compare(ga, gb, lists=(), sets=(), extras=False, what=""):
    assert ga.step == gb.step, what
    for k in PER_PARTICLE:
        _same(ga.get_state(k), gb.get_state(k), what + k)
    _same(ga.observe(), gb.observe(), what + "observe")
    _same(ga.box(), gb.box(), what + "box")
    _same(ga.barostat_state(), gb.barostat_state(), what + "barostat_state")
    _same(ga.get_events(), gb.get_events(), what + "events")
    _same(ga.get_exclusions(), gb.get_exclusions(), what + "exclusions")
    for h in lists:
        _same(ga.get_list(h), gb.get_list(h), what + "list %d" % h)
        _same(ga.list_get_lambda(h), gb.list_get_lambda(h), what + "list lambda %d" % h)
    for h in sets:
        _same(ga.fix_get(h), gb.fix_get(h), what + "fix_get %d" % h)
    if extras:
        _same(ga.get_state("LAMBDA"), gb.get_state("LAMBDA"), what + "LAMBDA")
        _same(ga.fix_log(), gb.fix_log(), what + "fix_log")
        _same(ga.fix_joins(), gb.fix_joins(), what + "fix_joins")
        _same(ga.reaction_removed(), gb.reaction_removed(), what + "reaction_removed")
        _same(ga.atrp_stats(), gb.atrp_stats(), what + "atrp_stats")
        _same(ga.pressure(), gb.pressure(), what + "pressure")


def _cold(spec):
    """the set-up of the loading context: the positions of step 0, zero velocities"""
    return dict(spec, vel=np.zeros_like(np.asarray(spec["vel"], np.float64)))


# ---- 1. the melt on every list path -------------------------------------------------------------------------------------------------
MELT = {"tiles": ((5, 5, 5), {}, True), "tiles_accumulated": ((5, 5, 5), {}, False), "cells": ((5, 5, 5), {"tiles": 0}, True), "brute": ((2, 7, 7), {}, True)}


def _melt_engine(make_gpu, prec, case, cold=False):
    nc, opts, by_displacement = MELT[case]
    spec = dict(H.ladder_spec(nc, 0.5, "uniform"), gamma=2.0)
    if not by_displacement:
        del spec["rebuild_criterion"]
    g = make_gpu(prec)
    for k, v in opts.items():
        g.set_option(k, v)
    W.apply(_cold(spec) if cold else spec, g)
    return g, spec


def _builds(g):
    return g.timers()["list_rebuilds"]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", sorted(MELT))
def test_melt_restart_is_exact_on_every_list_path(make_gpu, case, prec):
    nc, opts, _ = MELT[case]
    ga, spec = _melt_engine(make_gpu, prec, case)
    ga.run(0)
    ntiles, ncx = _path(ga)
    assert (ntiles > 0) == case.startswith("tiles") and (ncx > 0) == (case != "brute"), (case, ntiles, ncx)
    # a: the list has been built behind step 0 and the last three steps did not build it (so none fell on step a)
    first, age, last = _builds(ga), 0, _builds(ga)
    while not (last > first and age >= 3):
        assert ga.step < 200, "no aged list within 200 steps"
        ga.run(1)
        now = _builds(ga)
        age, last = (0, now) if now != last else (age + 1, last)
    a = ga.step
    blob = ga.checkpoint_save()
    assert ga.checkpoint_save() == blob                                        # two saves with nothing between them
    gb, _ = _melt_engine(make_gpu, prec, case, cold=True)
    gb.checkpoint_load(blob)
    assert gb.step == a and gb.checkpoint_save() == blob                        # a save right after the load: the loaded bytes
    _compare(ga, gb, what="at the load: ")
    # b: until each context has built its lists twice more -- once for the restart itself, once because the particles moved
    b, before_a, before_b = 0, _builds(ga), _builds(gb)
    while not (_builds(ga) >= before_a + 2 and b >= 5):
        assert b < 200, "no list build within 200 steps of the restart"
        ga.run(5)
        gb.run(5)
        b += 5
    assert _builds(ga) - before_a == _builds(gb) - before_b >= 2, (case, prec, _builds(ga), before_a, _builds(gb), before_b)
    print("%s fp%d: %d particles, a = %d (%d builds), b = %d (%d builds), blob %d bytes" % (case, prec, spec["n"], a, last, b, _builds(ga) - before_a, len(blob)))
    _compare(ga, gb, what="%d steps behind the load: " % b)
    assert not np.array_equal(ga.get_state("POS"), np.asarray(H.ladder_spec(nc, 0.5, "uniform")["pos"]))


# ---- 2. everything at once ----------------------------------------------------------------------------------------------------------
A_, B_, D_ = 0, 1, 2
INTERVAL, ATRP_INTERVAL, SAVE_AT, AFTER, RATE = 10, 7, 53, 27, 3.0


def _everything_spec():
    spec = W.reactive_melt(n=4000, seed=23, interval=INTERVAL, rate=RATE)
    L0, dfix = np.asarray(spec["box"], np.float64), 1.19
    near = cKDTree(AR.fold(spec["pos"], L0), boxsize=L0).query_pairs(dfix + 0.03, output_type="ndarray")
    d = spec["pos"][near[:, 0]] - spec["pos"][near[:, 1]]
    d -= L0 * np.rint(d / L0)
    near = near[np.abs(np.sqrt((d * d).sum(1)) - dfix) < 0.03]
    used, plain, typed = set(), [], []
    for i, j in near[np.lexsort((near[:, 1], near[:, 0]))]:
        i, j = int(i), int(j)
        if i in used or j in used:
            continue
        if spec["types"][j] != B_ and spec["types"][i] == B_:
            i, j = j, i
        if spec["types"][j] == B_ and len(typed) < 40:                     # the target is a B: a reaction that converts it sets it free
            typed.append((i + 1, j + 1)); used.update((i, j))
        elif len(plain) < 20:
            plain.append((i + 1, j + 1)); used.update((i, j))
    assert len(typed) == 40 and len(plain) == 20
    plain, typed = np.asarray(plain, np.int64), np.asarray(typed, np.int64)
    spec = dict(spec, exclusions=np.concatenate([plain, typed]), resolution=[(D_, D_, 0.0), (B_, D_, 0.0)], res_rates=[(D_, 0.02)],
                lists=[dict(arity=3, kind="ANG_HARMONIC", params=[1.25, np.pi], ids=np.empty((0, 3), np.int64), register=[(A_, A_, A_)])],
                atrp=dict(interval=ATRP_INTERVAL, num_particles=200, ratio_activator=0.8, ratio_deactivator=0.2, delta_catalyst=0.05, k_activate=1.0, k_deactivate=1.0,
                          select_from_all=True, seed=77,
                          centers=[dict(type_id=D_, state=1, is_activator=False, new_type=D_, new_mass=1.0, delta_state=5),
                                   dict(type_id=D_, state=6, is_activator=True, new_type=D_, new_mass=1.0, delta_state=-5)]))
    return spec, plain, typed, dfix


def _everything_engine(make_gpu, prec, spec, plain, typed, dfix, p0):
    g = make_gpu(prec)
    h = W.apply(spec, g)
    g.list_set_hybrid(h["reaction_bonds"], 0.0, 0.02)                       # new bonds switch on over 50 steps
    g.reaction_set_resolution(0, "type_2", 0.0)                             # A + B -> A + D: the D fades in under the rate of its type
    sets = [g.fix_create(-1, -1), g.fix_create(-1, B_)]
    g.fix_add(sets[0], plain, dfix)
    g.fix_add(sets[1], typed, dfix)
    g.fix_postprocess(sets[1], D_, lam=0.25)                                # a released D starts at lambda 0.25
    if p0 is not None:
        g.barostat_langevin(p0, 2000.0, 1.0, spec["kT"], 41)
    return g, h, sets


@pytest.mark.parametrize("prec", [64, 32])
def test_everything_at_once(make_gpu, prec):
    spec, plain, typed, dfix = _everything_spec()
    ga, h, sets = _everything_engine(make_gpu, prec, spec, plain, typed, dfix, None)
    ga.run(0)
    print("fp%d: %d tiles, %d cells along x" % ((prec,) + _path(ga)))      # (the λ words may not leave room for the LDS tiles: whichever path the plan takes)
    p0 = ga.pressure()["pressure"] + 2.0
    ga.barostat_langevin(p0, 2000.0, 1.0, spec["kT"], 41)
    ga.run(SAVE_AT)
    assert SAVE_AT % INTERVAL and SAVE_AT % ATRP_INTERVAL
    # what the save has to carry, each of it present
    ev0, lam_b, lam_p, log0 = ga.get_events(), ga.list_get_lambda(h["reaction_bonds"]), ga.get_state("LAMBDA"), ga.fix_log()
    angles0, stats0, st0 = ga.get_list(h[0]), ga.atrp_stats(), ga.barostat_state()
    print("fp%d at step %d: %d events, %d bonds (%d with 0 < lambda < 1), %d angles, %d particles with 0 < lambda < 1, %d releases, %d ATRP firings (%d flips), pe %.4g, box %.5f -> %.5f" % (
        prec, ga.step, len(ev0), len(lam_b), int(((lam_b > 0) & (lam_b < 1)).sum()), len(angles0), int(((lam_p > 0) & (lam_p < 1)).sum()), len(log0), len(stats0),
        sum(s["activated"] + s["deactivated"] for s in stats0), st0["momentum"], spec["box"][0], ga.box()[0]))
    assert len(ev0) > 0 and ((lam_b > 0) & (lam_b < 1)).any() and ((lam_p > 0) & (lam_p < 1)).any() and len(log0) > 0
    assert len(angles0) > 0 and (ga.get_state("TYPE") != spec["types"]).any()              # spawned angles, a type change
    assert len(stats0) == SAVE_AT // ATRP_INTERVAL and sum(s["activated"] + s["deactivated"] for s in stats0) > 0
    assert st0["kind"] == 2 and st0["momentum"] != 0.0 and ga.box()[0] != spec["box"][0]
    blob = ga.checkpoint_save()
    assert ga.checkpoint_save() == blob
    gb, hb, sets_b = _everything_engine(make_gpu, prec, _cold(spec), plain, typed, dfix, p0)
    assert hb == h and sets_b == sets
    gb.checkpoint_load(blob)
    assert gb.checkpoint_save() == blob
    lists = sorted(set(h.values()))
    _compare(ga, gb, lists, sets, extras=True, what="at the load: ")
    assert len(gb.get_events()) == len(ev0)                                                # the whole log, not the part since the load
    ga.run(AFTER)
    gb.run(AFTER)
    assert ga.step == SAVE_AT + AFTER
    _compare(ga, gb, lists, sets, extras=True, what="%d steps behind the load: " % AFTER)
    ev1 = ga.get_events()
    print("fp%d at step %d: %d events, %d bonds, %d angles, %d releases, blob %d bytes" % (prec, ga.step, len(ev1), len(ga.get_list(h["reaction_bonds"])), len(ga.get_list(h[0])),
                                                                                        len(ga.fix_log()), len(blob)))
    assert len(ev1) > len(ev0) and ev1["step"].max() > SAVE_AT and len(ga.atrp_stats()) == (SAVE_AT + AFTER) // ATRP_INTERVAL      # events on both sides of the save


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_loads_leave_the_context_as_it_was(make_gpu):
    ga, spec = _melt_engine(make_gpu, 64, "tiles")
    ga.run(7)
    blob = ga.checkpoint_save()
    # another precision
    g32, _ = _melt_engine(make_gpu, 32, "tiles")
    g32.run(3)
    with pytest.raises(ChemError, match="precision mismatch: the blob was written by a CHEM_PREC_F64 context, this one is CHEM_PREC_F32") as e:
        g32.checkpoint_load(blob)
    assert e.value.code == _capi.EINVAL
    g32.run(9)
    ref, _ = _melt_engine(make_gpu, 32, "tiles")
    ref.run(3)
    ref.run(9)
    _compare(g32, ref, what="fp32 after the refused load: ")
    # one list more
    gl, _ = _melt_engine(make_gpu, 64, "tiles")
    extra = gl.list_create(2, "HARMONIC", False)
    gl.list_set_params(extra, [30.0, 0.97])
    gl.run(3)
    with pytest.raises(ChemError, match=r"the configuration differs from the one the blob was saved under: list count \(blob 0, context 1\)") as e:
        gl.checkpoint_load(blob)
    assert e.value.code == _capi.EINVAL
    gl.run(9)
    ref, _ = _melt_engine(make_gpu, 64, "tiles")
    extra = ref.list_create(2, "HARMONIC", False)
    ref.list_set_params(extra, [30.0, 0.97])
    ref.run(3)
    ref.run(9)
    _compare(gl, ref, lists=[extra], what="one list more after the refused load: ")
    # a corrupt blob and a cut one
    bad = bytearray(blob)
    bad[len(bad) // 2] ^= 1
    gc, _ = _melt_engine(make_gpu, 64, "tiles")
    gc.run(3)
    for b, word in ((bytes(bad), "checksum mismatch"), (blob[:len(blob) // 2], "truncated"), (b"", "truncated")):
        with pytest.raises(ChemError, match=word) as e:
            gc.checkpoint_load(b)
        assert e.value.code == _capi.EINVAL
    gc.run(9)
    ref, _ = _melt_engine(make_gpu, 64, "tiles")
    ref.run(3)
    ref.run(9)
    _compare(gc, ref, what="after the corrupt blobs: ")
    # ... and the good blob still loads there
    gc.checkpoint_load(blob)
    ga.run(4)
    gc.run(4)
    _compare(ga, gc, what="a load into a context that has run: ")


def test_decomposed_context_refuses_save_and_load(make_gpu):
    ga, _ = _melt_engine(make_gpu, 64, "tiles")
    ga.run(5)
    blob = ga.checkpoint_save()
    spec = H.slab_spec("self_droplet")      # (5 x 5 x 23 cells as one slab that is its own z-neighbour: tests/test_gpu_geometry.py)

    def slab():
        g = make_gpu(64)
        g.set_option("dd_self", 1)
        W.apply(spec, g)
        return g
    gd = slab()
    gd.run(3)
    with pytest.raises(ChemError, match="checkpoint_save on a decomposed context: a gap of the decomposed path") as e:
        gd.checkpoint_save()
    assert e.value.code == _capi.ENOTIMPL
    with pytest.raises(ChemError, match="checkpoint_load on a decomposed context: a gap of the decomposed path") as e:
        gd.checkpoint_load(blob)
    assert e.value.code == _capi.ENOTIMPL
    gd.run(9)
    ref = slab()
    ref.run(3)
    ref.run(9)
    for k in ("POS", "IMAGE", "VEL", "FORCE", "TYPE", "STATE"):
        _same(gd.get_state(k), ref.get_state(k), "slab after the refusals: " + k)
    _same(gd.observe(), ref.observe(), "slab after the refusals: observe")


def test_save_before_the_particles_is_a_state_error(make_gpu):
    g = make_gpu(64)
    g.set_box([10.0, 10.0, 10.0])
    with pytest.raises(ChemError, match="checkpoint_save: set particles first") as e:
        g.checkpoint_save()
    assert e.value.code == _capi.ESTATE
    with pytest.raises(ChemError, match="checkpoint_load: set the context up first") as e:
        g.checkpoint_load(b"\0" * 64)
    assert e.value.code == _capi.ESTATE
