"""Forces from a neighbour list that has aged, on the device, in both precisions, against the exact pair sum of
tests/aged_ref.py at the engine's own positions -- no oracle, no second engine.

Every other fp32 check of the pair forces is taken at run(0), one evaluation behind a fresh list; after that fp32 runs are
judged by the trajectory alone, which a pair missing from the list for the last steps before a rebuild does not move enough
to show.  Here the forces are compared at the steps where the list is oldest, on every list path (LDS tiles, the per-cell list,
the brute-force list, a slab that is its own neighbour, two and three slabs), under both rebuild criteria and with a wider
internal list skin; the steps at which the lists are rebuilt are compared with the rule restated from the engine's own
positions; and pairs that enter the cutoff from the very edge of the list radius, 0.002 skin before the rebuild falls due,
must be in the forces.  tests/test_aged_ref.py keeps the reference and the constructions honest on the CPU."""
import numpy as np
import pytest

import aged_ref as AR
import helpers as H
from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import energy_scales, force_error_without_cutoff_flips
from test_gpu_pair_matrix import _energy_ok
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks

pytestmark = pytest.mark.gpu

PATHS = {"tiles": (1, {}), "cells": (1, {"tiles": 0}), "brute": (1, {}), "dd_self": (1, {"dd_self": 1}), "P2": (2, {}), "P3": (3, {})}
SINGLE = ("tiles", "cells", "brute")        # the device alone decides the rebuilds; on slabs the host calls for some of its own


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.compile_geometry_harness(tmp_path_factory.mktemp("host"))


def _on_path(make_gpu, prec, path, opts, body):
    """body(engine) on every rank of `path`, the engine's options set; returns the ranks' results."""
    P, popts = PATHS[path]
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        for k, v in dict(popts, **opts).items():
            g.set_option(k, v)
        if P > 1:
            g.comm_init_local(P, r, hub)
        return body(g)
    return _run_ranks(P, rank) if P > 1 else [rank(0)]


def _snapshot(g):
    t = g.timers()
    return dict(x=g.get_state("POS_UNFOLDED"), xf=g.get_state("POS"), v=g.get_state("VEL"), f=g.get_state("FORCE"), obs=g.observe(),
                reb=t["rebuilds"], lreb=t["list_rebuilds"])


def _compare(spec, snap, prec, what):
    """Forces, epot_lj and virial_nb of a snapshot against exact_pairs at its positions; asserts the guards on the way.
    Returns (force error, flipped pairs, pairs on the cutoff)."""
    ref = AR.exact_pairs(spec, snap["xf"])
    assert AR.guards(ref), ("ill-posed", what, ref["shell_pairs"], ref["fmax"], ref["jump"])
    at = dict(spec, pos=snap["xf"])
    if prec == 64:
        err, flips = rel_err(snap["f"], ref["f"]), 0
        assert err < TOL[64], (what, err)
    else:
        err, flips = force_error_without_cutoff_flips(at, snap["f"], ref["f"], TOL_MELT32, max_flips=ref["shell_pairs"])
        assert err < TOL_MELT32 and 0 <= flips <= ref["shell_pairs"], (what, err, flips, ref["shell_pairs"], ref["jump"] / ref["fmax"])
    sc = energy_scales(at)
    for k in ("epot_lj", "virial_nb"):
        assert _energy_ok(snap["obs"][k], ref[k], prec, sc[k]), (what, k, snap["obs"][k], ref[k], sc[k])
    return err, flips, ref["shell_pairs"]


def _same_on_every_rank(res, keys=("x", "v", "f")):
    for r in res[1:]:
        for a, b in zip(r, res[0]):
            assert all(np.array_equal(a[k], b[k]) for k in keys) and (a["reb"], a["lreb"]) == (b["reb"], b["lreb"])


# ---- (a), (b): thermal melts ------------------------------------------------------------------------------------------------------

# name: (path, melt of aged_ref.MELTS, rebuild criterion, option list_skin)
MELT_CASES = {
    "tiles-8788-crit0": ("tiles", "melt8788", 0, 0.0), "tiles-8788-crit1": ("tiles", "melt8788", 1, 0.0),      # the fused tile path
    "tiles-2197-crit0": ("tiles", "melt2197", 0, 0.0), "tiles-2197-crit1": ("tiles", "melt2197", 1, 0.0),      # 5 x 5 x 5 cells
    "cells-2197-crit0": ("cells", "melt2197", 0, 0.0), "cells-2197-crit1": ("cells", "melt2197", 1, 0.0),
    "brute-343-crit0": ("brute", "small_box", 0, 0.0), "brute-343-crit1": ("brute", "small_box", 1, 0.0),
    "dd_self-slab": ("dd_self", "slab", 0, 0.0), "P2-slab": ("P2", "slab", 0, 0.0), "P3-slab": ("P3", "slab", 0, 0.0),
    "tiles-8788-list_skin": ("tiles", "melt8788", 0, 0.5),       # the 16-bit list built for rc + skin_eff, ageing by list_rebuilds
}


def _melt_case(case):
    path, name, crit, ls = MELT_CASES[case]
    return path, AR.melt_spec(name, crit), ({"list_skin": ls} if ls > 0 else {})


def _run_a(make_gpu, prec, path, spec, opts):
    """Engine A: run(1) after run(1); a snapshot after every step (index 0: after run(0)).  The ranks of a decomposition must
    hold the same."""
    def body(g):
        W.apply(spec, g, thermostat=False)
        g.run(0)
        rec = [_snapshot(g)]
        for _ in range(AR.MELT_STEPS):
            g.run(1)
            rec.append(_snapshot(g))
        return rec
    res = _on_path(make_gpu, prec, path, opts, body)
    _same_on_every_rank(res)
    return res[0]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", list(MELT_CASES))
def test_melt_forces_at_the_oldest_list(make_gpu, case, prec):
    """(a) Forces, epot_lj and virial_nb against exact_pairs at every step whose successor builds a list, at every step that
    builds one, at step 1 and at the last step."""
    path, spec, opts = _melt_case(case)
    rec = _run_a(make_gpu, prec, path, spec, opts)
    steps, oldest = AR.check_steps([r["lreb"] for r in rec])
    assert len(oldest) >= (2 if opts else 7), (case, oldest)         # (the wider list lives about twice as long)
    worst, nflip, nshell = 0.0, 0, 0
    for s in steps:
        err, flips, shell = _compare(spec, rec[s], prec, (case, prec, s, "oldest" if s in oldest else ""))
        worst, nflip, nshell = max(worst, err), nflip + flips, nshell + shell
    print("%s fp%d: %d list builds in %d steps, %d steps compared (%d at the oldest list): worst force error %.2e, %d pairs on "
          "their cutoff, %d decided the other way" % (case, prec, rec[-1]["lreb"] - rec[0]["lreb"], AR.MELT_STEPS, len(steps), len(oldest),
                                                       worst, nshell, nflip))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", list(MELT_CASES))
def test_melt_run_in_pieces_ends_on_the_same_bits(make_gpu, case, prec):
    """(a) Engine B runs the same steps in pieces whose last step is an oldest-list step -- those evaluations are then the tail
    of a long run(k), under whatever look-ahead the idle launches apply.  POS_UNFOLDED, VEL and FORCE at the end of every
    piece equal engine A's bit for bit, and the forces there equal exact_pairs (the first and the last piece are compared)."""
    path, spec, opts = _melt_case(case)
    rec = _run_a(make_gpu, prec, path, spec, opts)
    _, oldest = AR.check_steps([r["lreb"] for r in rec])
    ends = sorted(set(oldest) | {AR.MELT_STEPS})
    assert len(ends) >= 3 and len(set(np.diff([0] + ends))) >= 2, ends          # pieces of more than one length

    def body(g):
        W.apply(spec, g, thermostat=False)
        out, at = [], 0
        for e in ends:
            g.run(e - at)
            at = e
            out.append(_snapshot(g))
        return out
    res = _on_path(make_gpu, prec, path, opts, body)
    _same_on_every_rank(res)
    for e, b in zip(ends, res[0]):
        a = rec[e]
        for k in ("x", "v", "f"):
            assert np.array_equal(a[k], b[k]), (case, prec, e, k, np.abs(a[k] - b[k]).max())
        assert (a["reb"], a["lreb"]) == (b["reb"], b["lreb"]), (case, prec, e)
    errs = [_compare(spec, res[0][k], prec, (case, prec, ends[k], "piece"))[0] for k in (0, -1)]
    print("%s fp%d: pieces ending at %s, bits of run(1) x %d; force error at the first and last end %.2e %.2e" % (case, prec, ends, AR.MELT_STEPS, *errs))


def _rule_check(x, counts, half_skin, crit, what):
    got = AR.increments(counts)
    want, unsure = AR.rule_rebuilds(x, half_skin, crit, follow=set(got))
    assert len(unsure) <= 1, (what, unsure)
    assert got == want, (what, got, want, unsure)
    return len(got), len(unsure)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", [c for c in MELT_CASES if MELT_CASES[c][0] in SINGLE])
def test_lists_are_rebuilt_when_the_rule_says(make_gpu, harness, case, prec):
    """(b) The steps at which `rebuilds` goes up are those of the rule on the workload's skin, restated from the engine's own
    unfolded positions -- not later (the list stays valid) and not earlier (the rebuild rate of the benchmark).  Without a list
    skin the lists are built at those very steps; with one, `list_rebuilds` follows the rule on the effective skin."""
    path, spec, opts = _melt_case(case)
    rec = _run_a(make_gpu, prec, path, spec, opts)
    x, crit = [r["x"] for r in rec], spec["rebuild_criterion"]
    n, u = _rule_check(x, [r["reb"] for r in rec], 0.5 * spec["skin"], crit, (case, prec, "rebuilds"))
    se = AR.effective_skin(harness, spec, opts.get("list_skin", 0.0))
    assert (se > spec["skin"]) == bool(opts)
    nl, ul = _rule_check(x, [r["lreb"] for r in rec], 0.5 * se, crit, (case, prec, "list_rebuilds"))
    print("%s fp%d: %d rebuilds by the rule on skin / 2 = %.3f (%d undecidable), %d list builds by the rule on %.4f (%d undecidable)" %
          (case, prec, n, 0.5 * spec["skin"], u, nl, 0.5 * se, ul))
    assert n >= 8 and nl >= (3 if opts else 8)


# ---- (c): closing pairs at the edge of the list radius ------------------------------------------------------------------------------

# (list_skin is an option of the tile path; "brute" runs the pairs in a box of 32 x 32 x 5, under three cells along z)
_TIGHT_ON = [(v, p) for v in AR.TIGHT_VARIANTS for p in PATHS if not (v == "list_skin" and p in ("cells", "brute"))]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("variant,path", _TIGHT_ON, ids=["%s-%s" % vp for vp in _TIGHT_ON])
def test_pairs_closing_from_the_edge_of_the_list_radius_are_in_the_forces(make_gpu, harness, variant, path, prec):
    """(c) Pairs rc + 0.99 skin_eff apart when the list was built are inside rc ten steps later, each partner 0.498 skin_eff from
    where it was binned: no list build in between, and the forces hold every one of them.  Then two more steps: the rebuild
    falls due on the first, and the forces behind it are compared again.  Six of the pairs lie off-centre across a slab
    boundary, one partner rc + 0.986 skin_eff deep in the cell layer the neighbour sends (aged_ref.tight_closing_pairs)."""
    P = PATHS[path][0]
    spec, opts = AR.tight_variant(variant, harness, dd=int(path not in SINGLE), P=P, flat=path == "brute")
    se, M, cl = spec["skin_eff"], spec["M"], spec["closing"]

    def body(g):
        W.apply(spec, g, thermostat=False)
        g.run(0)
        out = [_snapshot(g)]
        for k in (M, 1, 1):
            g.run(k)
            out.append(_snapshot(g))
        return out
    res = _on_path(make_gpu, prec, path, opts, body)
    _same_on_every_rank(res)
    s0, s1, s2, s3 = res[0]
    assert s1["lreb"] == s0["lreb"], (s0["lreb"], s1["lreb"])                    # no list build between the first evaluation and the M-th step
    if not opts:
        assert s1["reb"] == s0["reb"]
    r0, r1 = AR.pair_separations(spec, s0["xf"]), AR.pair_separations(spec, s1["xf"])
    assert r0[cl].min() > spec["rc"] + 0.98 * se and r1[cl].max() < spec["rc"] - 1e-4, (r0[cl].min(), r1[cl].max())
    moved = np.sqrt(((s1["x"] - s0["x"]) ** 2).sum(1)).max()
    assert 0.497 * se < moved < 0.4995 * se, moved / se
    part = np.repeat(cl, 2)
    errs = []
    for k, s in ((M, s1), (M + 1, s2), (M + 2, s3)):
        errs.append(_compare(spec, s, prec, (variant, path, prec, k))[0])
        ref = AR.exact_pairs(spec, s["xf"])
        assert ref["shell_pairs"] == 0
        assert np.abs(s["f"][part]).max(1).min() > 0.5 and np.abs(ref["f"][part]).max(1).min() > 0.5, (variant, path, prec, k)
    assert s2["lreb"] >= s1["lreb"] + 1 and (path not in SINGLE or s3["lreb"] == s1["lreb"] + 1), (s1["lreb"], s2["lreb"], s3["lreb"])
    print("%s %s fp%d: skin_eff %.4f, closing pairs from %.4f to %.4f, largest travel %.4f skin_eff; force error at steps M, M + 1, M + 2: "
          "%.2e %.2e %.2e" % (variant, path, prec, se, r0[cl].min(), r1[cl].max(), moved / se, *errs))
