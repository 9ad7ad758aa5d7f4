#!/usr/bin/env python3
"""A run with fixed distances at a size a user would run, for a kernel trace (profiles/fix_distances_kernels.txt):
N LJ hosts (default 108000 = 4 * 30^3) at rho = 0.2, three interaction-free dummies per host at 0.3 / 0.4 / 0.35 (total
density 0.8, the melt's).

    rocprofv3 --kernel-trace --stats -d <dir> -o fixd -- python3 tools/fix_distances_workload.py [--hosts N] [--steps K] [--prec 32|64]
    python3 tools/kstats.py <dir>/fixd_kernel_stats.csv 12

Prints one JSON line: particles, entries, steps, wall time per step."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W          # noqa: E402
from chemlab_amd.engine import Engine           # noqa: E402

DIST = (0.30, 0.40, 0.35)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=108000)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--prec", type=int, default=32)
    a = ap.parse_args()
    spec = W.lj_melt(n=a.hosts, rho=0.2, seed=5, jitter=0.05)      # hosts at a quarter of the melt's density: 0.8 with the dummies
    n = spec["n"]
    rng = np.random.default_rng(6)
    u = rng.normal(size=(n, 3, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    dpos = (spec["pos"][:, None, :] + np.array(DIST)[None, :, None] * u).reshape(-1, 3)
    dids = np.arange(n + 1, 4 * n + 1)
    g = Engine(device=0, precision=a.prec)
    W.apply(spec, g, thermostat=False, reactions=False)
    g.add_particles(dids, np.ones(3 * n, np.int32), dpos, np.full(3 * n, 0.25))
    h = g.fix_create()
    for j in range(3):
        g.fix_add(h, np.stack([np.arange(1, n + 1), n + 3 * np.arange(n) + j + 1], 1), DIST[j])
    g.run(a.warmup)
    g.sync()
    t0 = time.time()
    g.run(a.steps)
    g.sync()
    dt = time.time() - t0
    x = g.get_state("POS_UNFOLDED")
    pairs, dist = g.fix_get(h)
    d = x[pairs[:, 1] - 1] - x[pairs[:, 0] - 1]
    L = np.array(spec["box"])
    d -= L * np.rint(d / L)
    err = np.abs(np.linalg.norm(d, axis=1) - dist).max()
    print(json.dumps(dict(hosts=n, particles=4 * n, entries=int(g.fix_count(h)), steps=a.steps, precision=a.prec, ms_per_step=1e3 * dt / a.steps,
                          max_distance_error=float(err), list_rebuilds=int(g.timers()["list_rebuilds"]))))


if __name__ == "__main__":
    main()
