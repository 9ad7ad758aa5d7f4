"""Neighbour launch only on steps that can need a rebuild (options skip_idle, idle_lag, idle_kappa; single domain, fused
rebuild, accumulated criterion) changes no result.

On a step without the launch the force kernel's prologue folds the step's displacement maxima, decides and keeps the books;
if a rebuild falls due there after all, the run stops at that step and the host redoes it with the launch.  Either way the
list is built on the step it is built on with a launch on every step (skip_idle 0), so positions, velocities, forces, events,
bonds and both rebuild counts must be the same bit for bit.  skip_idle 2 leaves out every launch the host did not ask for
itself: every regular rebuild then goes through stop-and-resume.  The system is the one of
test_run_stopped_by_the_device_recovers_and_changes_nothing (tests/test_gpu_round3.py): 8788 particles, the smallest melt on
the fused path that rebuilds a dozen times in 120 steps."""
import ctypes

import numpy as np
import pytest

from chemlab_amd import workloads as W
from helpers import sorted_events
from test_gpu_list_overflow import melt, LIST_SKIN

pytestmark = pytest.mark.gpu

STEPS = 120


def counter(eng, name):
    fn = getattr(eng.api.lib, name)
    fn.restype = ctypes.c_int64
    return int(fn(ctypes.c_void_p(eng.ctx)))


def counters(eng):
    return tuple(counter(eng, "chem_debug_idle_" + k) for k in ("skipped", "wrong_skips", "timeouts"))


def spec_small():
    spec = W.reactive_melt(n=8788, seed=71, interval=40)
    spec["rebuild_criterion"] = 0
    return spec


def engine(make_gpu, spec, prec, skip_idle, options=(), **kw):
    e = make_gpu(prec)
    h = W.apply(spec, e, **kw)
    for k, v in options:
        e.set_option(k, v)
    e.set_option("skip_idle", skip_idle)
    return e, h


def snapshot(e, h):
    t = e.timers()
    return dict(pos=e.get_state("POS_UNFOLDED"), vel=e.get_state("VEL"), force=e.get_state("FORCE"), events=sorted_events(e.get_events()),
                bonds=e.get_list(h["reaction_bonds"]), rebuilds=t["rebuilds"], list_rebuilds=t["list_rebuilds"])


def same(a, b):
    for k in ("pos", "vel", "force", "bonds"):
        assert np.array_equal(a[k], b[k]), k
    assert a["events"] == b["events"]
    assert (a["rebuilds"], a["list_rebuilds"]) == (b["rebuilds"], b["list_rebuilds"])


_reference = {}


def reference(make_gpu, prec):
    """A launch on every step: computed once per precision, shared, never changed."""
    if prec not in _reference:
        e, h = engine(make_gpu, spec_small(), prec, 0)
        e.run(STEPS)
        assert counters(e) == (0, 0, 0)
        _reference[prec] = snapshot(e, h)
        assert len(_reference[prec]["events"]) > 100 and _reference[prec]["list_rebuilds"] >= 8
    return _reference[prec]


@pytest.mark.parametrize("prec", [32, 64])
def test_rule_changes_nothing(make_gpu, prec):
    ref = reference(make_gpu, prec)
    e, h = engine(make_gpu, spec_small(), prec, 1)
    e.run(STEPS)
    same(ref, snapshot(e, h))
    skipped, wrong, timeouts = counters(e)
    print("skip_idle 1, fp%d: %d of %d steps without the launch, %d wrong skips, %d timeouts, %d list builds" % (prec, skipped, STEPS, wrong, timeouts, ref["list_rebuilds"]))
    assert skipped > 0 and wrong == 0 and timeouts == 0


@pytest.mark.parametrize("prec", [32, 64])
def test_every_regular_rebuild_through_stop_and_resume(make_gpu, prec):
    ref = reference(make_gpu, prec)
    e, h = engine(make_gpu, spec_small(), prec, 2)
    e.run(STEPS)
    same(ref, snapshot(e, h))
    skipped, wrong, timeouts = counters(e)
    # List builds the host asks for itself, from the spec: the one before the first step and at most one per reaction step (the
    # rebuild a reaction step requests when it has changed bonds and exclusions; reaction steps at 40, 80 and 120).  Every other
    # build of the run is a decision of the device and went through a stop.
    requested = 1 + STEPS // 40
    print("skip_idle 2, fp%d: %d steps without the launch, %d wrong skips, %d list builds of which at most %d requested by the host"
          % (prec, skipped, wrong, ref["list_rebuilds"], requested))
    assert wrong >= ref["list_rebuilds"] - requested and wrong >= 5 and timeouts == 0
    assert counter(e, "chem_debug_halts") == wrong
    assert skipped <= STEPS - wrong         # (steps enqueued behind a stop left at once and are redone: not counted)


def test_generations_two_runs_and_a_set_up_change(make_gpu):
    """Two runs back to back, then a list-skin change.  What the device published during one call is not used by the next: the
    first step of a call gets the neighbour launch, so the skipped count of a one-step run stays put -- this leg is the one
    that only the hint's generation protects (nothing is rebuilt between the calls, the hint of the first call is one step
    old and well inside the budget).  The step behind the set-up change launches in any case, the host having asked for that
    rebuild itself; the leg pins that the new generation's hints are used again behind it and that the results agree with an
    engine that launches on every step."""
    a, ha = engine(make_gpu, spec_small(), 32, 0)
    b, hb = engine(make_gpu, spec_small(), 32, 1)
    a.run(50); b.run(50)
    s0 = counters(b)[0]
    assert s0 > 0
    a.run(1); b.run(1)                         # back to back
    assert counters(b)[0] == s0
    for e in (a, b):
        e.set_option("list_skin", 0.45)
    a.run(1); b.run(1)                         # behind a geometry change (a rebuild the host asks for, a new generation)
    assert counters(b)[0] == s0
    a.run(30); b.run(30)
    assert counters(b)[0] > s0
    same(snapshot(a, ha), snapshot(b, hb))
    assert counters(b)[1:] == (0, 0)


def test_flagship_cell_edge(make_gpu):
    """The flagship's cell edge and tile fill (tests/test_gpu_list_overflow.py: 74 088 particles, list skin 0.49), 40 steps, fp32."""
    out = []
    for skip in (0, 1):
        e = make_gpu(32)
        W.apply(melt(), e, reactions=False)
        e.set_option("list_skin", LIST_SKIN)
        e.set_option("skip_idle", skip)
        e.run(40)
        out.append((e.get_state("POS_UNFOLDED"), e.get_state("VEL"), e.get_state("FORCE"), e.timers()["list_rebuilds"], e.timers()["rebuilds"], counters(e)))
    a, b = out
    for k in range(3):
        assert np.array_equal(a[k], b[k])
    assert a[3:5] == b[3:5] and a[3] >= 2
    print("flagship cell edge: %d of 40 steps without the launch, %d wrong skips, %d timeouts" % b[5])
    assert b[5][0] > 0 and b[5][1] == 0 and b[5][2] == 0


def acc_words(eng):
    out = (ctypes.c_double * 2)()
    eng.api.lib.chem_debug_acc.restype = ctypes.c_int64
    assert eng.api.lib.chem_debug_acc(ctypes.c_void_p(eng.ctx), out) == 0
    return out[0], out[1]


@pytest.mark.parametrize("prec", [32, 64])
def test_bucket_row_recovery_under_the_rule(make_gpu, prec):
    """The stop of test_run_stopped_by_the_device_recovers_and_changes_nothing (bucket rows one slot wider than the fullest cell
    of the lattice start: the melting system overflows them some dozens of steps in) with the rule on.  The redo needs two
    attempts -- the first runs with the old rows and meets the full row again --, both must read the stopped step's own
    maxima: the reference rule's accumulated distance (DevCtl::acc_ref), the list's (acc_maxdist) and both rebuild counts
    after the run are those of an engine that launches on every step and never stopped, bit for bit, like the trajectory.
    The step behind the recovery must not wait for a hint that never comes: no look-ahead time-out."""
    spec = spec_small()
    a, ha = engine(make_gpu, spec, prec, 0)
    b, hb = engine(make_gpu, spec, prec, 1)
    a.run(0)
    pos = a.get_state("POS")
    L = spec["box"][0]; nc = int(L // 2.8)
    occ = np.bincount(np.ravel_multi_index(np.minimum((pos / (L / nc)).astype(int), nc - 1).T, (nc, nc, nc)), minlength=nc ** 3).max()
    b.set_option("bucket_cap", int(occ) + 1)
    # Several calls (the same for both engines): the words are compared within a few steps of the recovery, before a rebuild
    # the host asks for can level them.  No call ends on a reaction step (40, 80, 120), so that every rebuild of the run is
    # enqueued by the loop -- a rebuild at the start of a call would widen the rows on the spot, without a stop.
    for k, n in enumerate([44] + [7] * 11):
        a.run(n); b.run(n)
        ra, rb, ta, tb = acc_words(a), acc_words(b), a.timers(), b.timers()
        assert ra == rb and (ta["rebuilds"], ta["list_rebuilds"]) == (tb["rebuilds"], tb["list_rebuilds"]), (k, ra, rb)
    assert counter(b, "chem_debug_halts") >= 1      # it did happen
    same(snapshot(a, ha), snapshot(b, hb))
    print("bucket-row recovery, fp%d: %d runs resumed, counters %r" % (prec, counter(b, "chem_debug_halts"), counters(b)))
    skipped, wrong, timeouts = counters(b)
    assert skipped > 0 and timeouts == 0
