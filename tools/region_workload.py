#!/usr/bin/env python3
"""The price of region rules (DESIGN.md "Region rules"; profiles/region_kernels.txt): the C3 set-up of tools/bench_configs.py
-- 128k beads of a tabulated polymer melt with harmonic bonds and angles -- with every 50th bead of a minority type 1, and six
FreezeRegion slabs (chem_region_add, mode prob, every step) at the box faces that turn type 1 into type 2.  All three types
carry the same table, so a frozen bead stays part of the melt and the run stays what it was: what is measured is the rule.

The same binary runs the same system twice, without and with the rules:

    python3 tools/region_workload.py [--steps K] [--warmup W] [--prec 32|64] [--chains N] [--width w] [--prob p] [--every m]

Prints one JSON line: steps per second of both runs, the added wall time per firing (the scan launch plus the two half kicks
launched apart on a firing step), firings, firings that changed something per thousand steps, host synchronisations the
rules caused.  The scan kernel's own time is read from
    rocprofv3 --kernel-trace --stats -- python3 tools/region_workload.py --steps 500
(k_region_scan in the kernel statistics)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W          # noqa: E402
from chemlab_amd.engine import Engine           # noqa: E402


def system(chains, every):
    spec = W.polymer_melt(n_chains=chains, chain_len=32, seed=3)
    spec["types"][::every] = 1
    t = spec["tables"][0]
    spec["tables"] = [(a, b) + tuple(t[2:]) for a in range(3) for b in range(a, 3)]
    return spec


def timed(spec, prec, warmup, steps, rules):
    g = Engine(device=0, precision=prec)
    W.apply(spec, g)
    for r in rules:
        g.region_enable(g.region_add(**r))
    g.run(warmup)
    g.sync()
    f0, s0 = g.region_counters()
    n0 = len(g.region_stats())
    t0 = time.perf_counter()
    g.run(steps)
    g.sync()
    dt = time.perf_counter() - t0
    f1, s1 = g.region_counters()
    st = g.region_stats()[n0:]
    out = dict(wall_s=dt, steps_per_s=steps / dt, firings=f1 - f0, syncs=s1 - s0, changing_steps=len(set(st["step"].tolist())),
               changed=int(st["changed"].sum()), frozen=int((g.get_state("TYPE") == 2).sum()))
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prec", type=int, default=32)
    ap.add_argument("--chains", type=int, default=4000)
    ap.add_argument("--width", type=float, default=0.5)
    ap.add_argument("--prob", type=float, default=0.001)
    ap.add_argument("--every", type=int, default=50)
    a = ap.parse_args()
    spec = system(a.chains, a.every)
    L = float(spec["box"][0])
    rules = []
    for d in range(3):
        for upper in (False, True):
            lo, hi = [0.0] * 3, [L] * 3
            if upper:
                lo[d] = L - a.width
            else:
                hi[d] = a.width
            rules.append(dict(lo=lo, hi=hi, target_type=1, new_type=2, interval=1, mode="prob", value=a.prob, reset_velocity=True,
                              reset_force=True, seed=12345))
    base = timed(spec, a.prec, a.warmup, a.steps, [])
    with_rules = timed(spec, a.prec, a.warmup, a.steps, rules)
    out = dict(particles=int(spec["n"]), minority=int((spec["types"] == 1).sum()), precision=a.prec, steps=a.steps, width=a.width, prob=a.prob,
               steps_per_s_without=base["steps_per_s"], steps_per_s_with=with_rules["steps_per_s"],
               added_us_per_firing=1e6 * (with_rules["wall_s"] - base["wall_s"]) / max(with_rules["firings"], 1),
               firings=with_rules["firings"], host_syncs=with_rules["syncs"], changed=with_rules["changed"],
               changing_firings_per_1000_steps=1000.0 * with_rules["changing_steps"] / a.steps, frozen_at_end=with_rules["frozen"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
