#!/usr/bin/env python3
"""The price of g(r) sampling inside chem_run (DESIGN.md "Radial distribution functions"; profiles/rdf_kernels.txt): the C3
set-up of tools/bench_configs.py -- 128k beads of a tabulated polymer melt with harmonic bonds and angles -- and the C5 melt of
bench.py (a simple-cubic reactive LJ melt, reactions left off here), each run without sampling and with sample_every = 1, 10
and 100, 256 bins, for one selector and for eight selectors with the molecule split, on the same binary.

    python3 tools/rdf_workload.py [--steps K] [--warmup W] [--prec 32|64|0 (both)] [--system c3|c5|both] [--n5 N] [--every 1,10,100]
                                  [--trace]

Prints one JSON line per (system, precision): steps per second without sampling, and per configuration the steps per second,
the added wall time per frame, the frames taken and the pairs counted per frame.  The kernels' own durations are read from
    rocprofv3 --kernel-trace --stats -- python3 tools/rdf_workload.py --trace --steps 200 --system c5 --prec 32 --every 10
(--trace: one run only, eight selectors with the split, reactions on so that k_react_scan_tiles is in the same statistics as
k_rdf_tiles, k_rdf_frame and k_pair_tiles); their register, LDS and scratch figures from
    make -C chemlab_amd/csrc resource-usage."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W          # noqa: E402
from chemlab_amd.engine import Engine           # noqa: E402

SEL8 = [(-1, -1), (0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (-1, 0)]


def timed(spec, prec, warmup, steps, conf, reactions):
    g = Engine(device=0, precision=prec)
    W.apply(spec, g, reactions=reactions)
    if conf:
        g.rdf_init(spec["rc"], 256, conf["sel"], split_molecules=conf["split"])
        g.rdf_sample_every(conf["every"])
    g.run(warmup)
    g.sync()
    if conf:
        g.rdf_reset()
    t0 = time.perf_counter()
    g.run(steps)
    g.sync()
    dt = time.perf_counter() - t0
    out = dict(wall_s=dt, steps_per_s=steps / dt)
    if conf:
        r = g.rdf()
        nz = int((r["counts"] != 0).sum())
        out.update(frames=r["frames"], pairs_per_frame=int(r["counts"][0].sum()) // max(r["frames"], 1), nonzero_words=nz)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prec", type=int, default=0)
    ap.add_argument("--system", default="both")
    ap.add_argument("--n5", type=int, default=1000000)
    ap.add_argument("--every", default="1,10,100")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    systems = []
    if a.system in ("c3", "both"):
        systems.append(("C3", W.polymer_melt(n_chains=4000, chain_len=32, seed=3)))
    if a.system in ("c5", "both"):
        systems.append(("C5", W.reactive_melt(n=a.n5, rho=0.8, interval=500, seed=2, skin=0.3)))
    for name, spec in systems:
        for prec in ((32, 64) if a.prec == 0 else (a.prec,)):
            if a.trace:
                spec = dict(spec)
                if "reaction" in spec:
                    spec["reaction"] = dict(spec["reaction"], interval=50)
                r = timed(spec, prec, a.warmup, a.steps, dict(sel=SEL8, split=True, every=int(a.every.split(",")[0])), True)
                print(json.dumps(dict(system=name, precision=prec, trace=True, **r)), flush=True)
                continue
            base = timed(spec, prec, a.warmup, a.steps, None, False)
            row = dict(system=name, n=int(spec["n"]), precision=prec, steps=a.steps, r_max=spec["rc"], bins=256, base_steps_per_s=round(base["steps_per_s"], 1), runs=[])
            for sel, split, label in (([(-1, -1)], False, "1 selector"), (SEL8, True, "8 selectors, split")):
                for every in [int(v) for v in a.every.split(",")]:
                    r = timed(spec, prec, a.warmup, a.steps, dict(sel=sel, split=split, every=every), False)
                    per_frame_ms = 1e3 * (r["wall_s"] - base["wall_s"]) / max(r["frames"], 1)
                    row["runs"].append(dict(conf=label, every=every, steps_per_s=round(r["steps_per_s"], 1), frames=r["frames"],
                                            added_ms_per_frame=round(per_frame_ms, 4), pairs_per_frame=r["pairs_per_frame"], nonzero_words=r["nonzero_words"]))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
