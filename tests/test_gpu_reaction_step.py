"""The association reaction step on the device against tests/react_ref.py (plain numpy, no oracle): every zoo member through
every scan path -- LDS tiles, the per-cell list, the brute-force list, one slab that is its own neighbour, two and three slabs --
in both precisions.  The members are frozen (no pair potential; K = 0 reaction bonds, or masses of 2^80 where a member carries
bonded forces for test_forces_through_the_incremental_tables) with coordinates on a 2^-10 grid in
power-of-two boxes, so fp64 and the fp32 build's fixed-point codec hold the same positions and every r2 is compared to the bit;
the closing pairs (member 8) move without forces and are compared at the positions read back from the engine.
tests/test_react_ref.py asserts the members' own conditions (matching rounds, ties, pairs on the cutoffs, candidate counts)."""
import pytest

import react_ref as RR
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from test_gpu_bonded import TOL_E, TOL_F
from test_gpu_parity import _HUB, _run_ranks
from test_react_ref import FORCE_MEMBERS, _run_engine, check_against_reference, check_closing, check_forces, run_with_forces

pytestmark = pytest.mark.gpu

PATHS = {"tiles": (1, {}), "cells": (1, {"tiles": 0}), "dd_self": (1, {"dd_self": 1}), "P2": (2, {}), "P3": (3, {})}


def _on_path(make_gpu, prec, path, body):
    """body(engine) on every rank of `path`; returns the ranks' results."""
    P, opts = PATHS[path]
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        for k, v in opts.items():
            g.set_option(k, v)
        if P > 1:
            g.comm_init_local(P, r, hub)
        return body(g)
    return _run_ranks(P, rank) if P > 1 else [rank(0)]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(RR.ZOO))
def test_reaction_step_matches_reference(make_gpu, name, path, prec):
    """Events (step, id_a, id_b, reaction, r2 bits), pad, bond list, spawned lists, STATE, TYPE, MASS, CHARGE, MOLID, RESID,
    exclusions and ATRP stats rows after every reaction step (after every step where the member runs the ATRP activator) equal
    the reference's; every path and both precisions therefore equal each other."""
    spec, _ = RR.member(name)
    for got in _on_path(make_gpu, prec, path, lambda g: _run_engine(g, spec)):
        check_against_reference(name, got)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name", list(RR.SMALL))
def test_reaction_step_brute_force_list(make_gpu, name, prec):
    """A 4^3 box: 2.2 cells per axis, the brute-force list; the scan is k_react_scan on that list."""
    spec, _ = RR.member(name)
    check_against_reference(name, _run_engine(make_gpu(prec), spec))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", FORCE_MEMBERS)
def test_forces_through_the_incremental_tables(make_gpu, name, path, prec):
    """`spawn` and `nbchange_typed` have bonded parameters and masses of 2^80: after every reaction step FORCE and chem_obs.epot_list
    equal the autograd reference on the reference's own lists and types, within the tolerances of tests/test_gpu_bonded.py, relative
    to the largest force component of the particle's cell.  The tuples and exclusions of a step and the slots re-resolved after a
    retyping reach the device through the incremental table uploads only.  Nothing moves: POS after the last step is the input to
    the bit."""
    spec, ref = RR.member(name)
    for out, pos in _on_path(make_gpu, prec, path, lambda g: run_with_forces(g, spec)):
        check_forces(spec, ref, out, pos, TOL_F[prec], TOL_E[prec], "%s fp%d" % (path, prec))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ["tiles", "cells", "dd_self"])
def test_more_candidates_than_the_buffer_holds_is_refused(make_gpu, path, prec):
    """Sixteen identical reactions on the block: 8640 candidates, capacity max(8 N, 1024) = 1728.  CHEM_ENOSPC, not fewer events.
    One rank only: on slabs the scan's refusal is raised by the rank that overflows, in front of the exchange the other ranks
    wait in, and a test must not set that up."""
    spec = RR.cluster(16)

    def body(g):
        W.apply(spec, g)
        try:
            g.run(spec["reaction"]["interval"])
        except ChemError as e:
            return e.code
        finally:
            g.close()
        return 0
    assert _on_path(make_gpu, prec, path, body) == [-2] * PATHS[path][0]


_CLOSING = [("crit0", dict(rebuild_criterion=0), {}, 32.0 / 17.0), ("crit1", dict(rebuild_criterion=1), {}, 32.0 / 17.0),
            ("list_skin", dict(rebuild_criterion=0), {"list_skin": 0.5}, 2.0)]      # rc + 0.5 = 2: sixteen cells of edge 2 per axis


_CLOSING_ON = [(v, p) for v in _CLOSING for p in PATHS if not (v[2] and p == "cells")]      # (list_skin is an option of the tile path)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("variant,path", _CLOSING_ON, ids=["%s-%s" % (v[0], p) for v, p in _CLOSING_ON])
def test_closing_pairs_react_on_the_tables_of_the_last_rebuild(make_gpu, variant, path, prec):
    """Pairs that were rc + 0.9 skin - 0.02 apart when the tables were built and are rc - 0.02 apart at the reaction step, each
    partner 0.45 skin from where it was binned, in other cells and tiles and across periodic faces; receding pairs end outside.
    No rebuild in between (asserted).  (step, ids, reaction) and r2 to the bit against the reference at the engine's own
    positions: with a power-of-two box no operation of minimgD / dist2_unfused is left unrestated."""
    _, upd, opts, edge = variant
    spec = dict(RR.closing_pairs(edge), **upd)

    def body(g):
        for k, v in opts.items():
            g.set_option(k, v)
        return [e[:4] for e in check_closing(g, spec)]
    res = _on_path(make_gpu, prec, path, body)
    assert all(r == res[0] for r in res)
