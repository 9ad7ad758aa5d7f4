#!/usr/bin/env python3
"""The price of the hybrid kernel family on a workload with angles ("Hybrid pair lists";
profiles/hybrid_tuples_kernels.txt): the C3 set-up of tools/bench_configs.py -- 128k beads of a tabulated polymer melt with
harmonic bonds and angles -- with its angle list plain (--variant plain: k_bonded_work, the kernel every such context launched
before) or hybrid at lambda0 = 1, rate 0 (--variant hybrid: chem_list_set_hybrid_tuples, k_bonded_work_hyb, every triple two
entries wide).  lambda is 1 for every entry, so the physics is the same; the kernels and the entry table differ.

    python3 tools/hybrid_tuples_workload.py [--variant plain|hybrid] [--steps K] [--warmup W] [--prec 32|64] [--chains N]

Prints one JSON line: particles, triples, steps, steps per second, rebuilds."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W          # noqa: E402
from chemlab_amd.engine import Engine           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("plain", "hybrid"), default="hybrid")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prec", type=int, default=32)
    ap.add_argument("--chains", type=int, default=4000)
    a = ap.parse_args()
    spec = W.polymer_melt(n_chains=a.chains, chain_len=32, seed=3)
    angles = spec["lists"].pop(1)
    g = Engine(device=0, precision=a.prec)
    W.apply(spec, g)
    h = g.list_create(3, angles["kind"], False)
    g.list_set_params(h, angles["params"])
    if a.variant == "hybrid":
        g.list_set_hybrid_tuples(h, 1.0, 0.0)      # (while the list is empty)
    g.list_add(h, angles["ids"])
    g.run(a.warmup)
    g.sync()
    t0 = time.perf_counter()
    g.run(a.steps)
    g.sync()
    dt = time.perf_counter() - t0
    lam = g.list_get_lambda(h)
    out = dict(particles=int(spec["n"]), variant=a.variant, triples=int(len(angles["ids"])), steps=a.steps, precision=a.prec, steps_per_s=a.steps / dt,
               rebuilds=int(g.timers()["rebuilds"]), lambda_min=float(lam.min()), lambda_max=float(lam.max()))
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
