#!/usr/bin/env python3
"""The price of the cap radius in the pair loop ("Capped pairs"; profiles/capped_kernels.txt): the C3
set-up of tools/bench_configs.py -- 128k beads of a tabulated polymer melt with harmonic bonds and angles -- with its one
table uncapped (--caprad 0, the kernels every context launched before) or capped at --caprad (chem_nb_cap: k_pair_tiles_cap).
The default radius 0.65 is the melt's first-neighbour distance rho^(-1/3), so that a good share of the pairs sits inside it.

    python3 tools/capped_workload.py [--caprad C] [--steps K] [--warmup W] [--prec 32|64] [--chains N]

Prints one JSON line: particles, steps, steps per second, the share of listed pairs inside the cap radius at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W          # noqa: E402
from chemlab_amd.engine import Engine           # noqa: E402


def share_inside(g, spec, caprad, sample=2000):
    """fraction of the pairs within the cutoff of `sample` particles that lie inside the cap radius"""
    x, box = g.get_state("POS"), np.asarray(spec["box"])
    rng = np.random.default_rng(1)
    inside = total = 0
    for i in rng.choice(len(x), size=min(sample, len(x)), replace=False):
        d = x - x[i]
        d -= box * np.rint(d / box)
        r2 = (d * d).sum(1)
        r2[i] = np.inf
        total += int((r2 <= spec["rc"] ** 2).sum())
        inside += int((r2 < caprad * caprad).sum())
    return inside / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--caprad", type=float, default=0.65)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prec", type=int, default=32)
    ap.add_argument("--chains", type=int, default=4000)
    a = ap.parse_args()
    spec = W.polymer_melt(n_chains=a.chains, chain_len=32, seed=3)
    if a.caprad > 0:
        spec["caps"] = [(0, 0, a.caprad)]
    g = Engine(device=0, precision=a.prec)
    W.apply(spec, g)
    g.run(a.warmup)
    g.sync()
    t0 = time.perf_counter()
    g.run(a.steps)
    g.sync()
    dt = time.perf_counter() - t0
    out = dict(particles=int(spec["n"]), caprad=a.caprad, steps=a.steps, precision=a.prec, steps_per_s=a.steps / dt,
               rebuilds=int(g.timers()["rebuilds"]), share_inside=share_inside(g, spec, a.caprad) if a.caprad > 0 else 0.0)
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
