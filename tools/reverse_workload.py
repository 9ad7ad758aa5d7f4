#!/usr/bin/env python
"""What a reaction step with bond removals and joins costs: the full cycle of tests/test_gpu_reverse.py (condensation
A + B -> C:E releasing a dummy as a water, hydrolysis C:E + W -> A + B taking the bond out and joining the water again),
scaled up to K^3 lattice sites, four reaction steps, once with the removal / join / release rules and once without them
(then the condensation happens once and nothing follows).  Run with CHEM_TRACE=1 for the phase times of every reaction
step; the last line is the reaction wall time per reaction step.  profiles/reverse_reaction_step.txt holds a run."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from chemlab_amd import workloads as W      # noqa: E402
from chemlab_amd.engine import Engine       # noqa: E402

A, B, C, E, WAT, D = 0, 1, 2, 3, 4, 5
MASS = {t: 1.0 + 0.5 * t for t in range(8)}


def system(k):
    sp = 1.8
    pos, types = [], []
    for c in np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3):
        base = 0.125 + sp * c
        if int(c.sum()) % 2 == 0:
            pos += [base, base + [0.375, 0, 0], base + [0, 0.25, 0]]; types += [A, B, D]
        else:
            pos += [base, base + [0.375, 0, 0]]; types += [A, A]
    types = np.array(types, np.int32)
    n = len(types)
    rx = dict(delta_1=0, delta_2=0, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1, rate=1e9, min_cutoff=0.0, intramolecular=False,
              is_virtual=False, active=True, new_q_1=0.0, new_q_2=0.0)
    cond = dict(rx, type_1=A, type_2=B, cutoff=0.5, new_type_1=C, new_type_2=E, intraresidual=True)
    hydro = dict(rx, type_1=C, type_2=WAT, cutoff=0.5, new_type_1=A, new_type_2=D, intraresidual=False, is_virtual=True)
    spec = dict(box=[sp * k] * 3, rc=1.5, skin=0.3, dt=0.001, ids=np.arange(1, n + 1), types=types, pos=np.array(pos), mass=np.array([MASS[t] for t in types]),
                vel=np.zeros((n, 3)), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32), rebuild_criterion=1, lj=[(A, 6, 1.0, 0.5, 1.0)],
                reaction=dict(bond=("HARMONIC", [0.0, 1.0]), interval=1, nearest=True, max_per_interval=0, seed=77, type_mass=MASS, reactions=[cond, hydro]))
    return W.snap_to_grid(spec), np.nonzero(types == D)[0]


def run(k, prec, rules):
    spec, dummy = system(k)
    g = Engine(device=0, precision=prec)
    h = W.apply(spec, g, thermostat=False)
    if rules:
        hs = g.fix_create(A, D)
        g.fix_add(hs, [(int(d) - 1, int(d) + 1) for d in dummy], 0.25)
        g.fix_postprocess(hs, D, WAT, MASS[WAT], 0.0, -1, 0.0)
        g.reaction_release(0, "type_1", hs, 1)
        g.reaction_neighbour_change(1, "type_1", E, 1, B, MASS[B])
        g.reaction_remove_bond(1, "type_1", C, 1, C, E, True)
        g.reaction_join(1, "type_1", hs, 0.25)
        g.reaction_set_resolution(1, "type_2", 0.5)
    g.run(0)
    for _ in range(4):
        g.run(1)
    t = g.timers()
    nev = len(g.get_events())
    nrem, njoin = (len(g.reaction_removed()), len(g.fix_joins())) if rules else (0, 0)      # (--rules 0 also runs on a build without them)
    print("rules %d: %d particles, %d events, %d bonds left, %d removal records, %d joins; reaction wall %.3f ms per reaction step (%d steps)"
          % (rules, g.n, nev, len(g.get_list(h["reaction_bonds"])), nrem, njoin, 1e3 * t["reaction_wall_s"] / t["reaction_steps"], t["reaction_steps"]), flush=True)
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--precision", type=int, default=32)
    ap.add_argument("--rules", type=int, nargs="+", default=[0, 1], help="0: without the rules, 1: with them")
    a = ap.parse_args()
    for rules in a.rules:
        run(a.k, a.precision, rules)
