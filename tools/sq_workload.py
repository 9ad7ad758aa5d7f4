#!/usr/bin/env python3
"""The price of a structure-factor frame (DESIGN.md "Structure factor"; profiles/sq_kernels.txt): the C3 set-up of
tools/bench_configs.py -- 128k beads of a tabulated polymer melt with harmonic bonds and angles -- and the C5 melt of bench.py (a
simple-cubic reactive LJ melt, reactions left off here), a frame for nmax = 4, 8 and 16 with one and with four selectors, on the
same binary.

    python3 tools/sq_workload.py [--steps K] [--warmup W] [--prec 32|64|0 (both)] [--system c3|c5|both] [--n5 N] [--frames F]
                                 [--host-n N] [--out FILE]

A frame is timed on the device: F frames back to back between two HIP events on the context's stream (chem_debug_sq_frame_ms).
Beside it: the same build's wall time per MD step without sampling, and a host evaluation of the same sums -- numpy, fp64,
N x nvec cos and sin -- at --host-n particles of the same system (default 10^4) for one selector, scaled linearly to the system's
particle count.  Prints one JSON line per (system, precision) and, with --out, writes the table as text.  The kernels' register,
LDS and scratch figures come from
    make -C chemlab_amd/csrc resource-usage."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chemlab_amd import workloads as W                  # noqa: E402
from chemlab_amd.engine import Engine, sq_vectors       # noqa: E402

SEL1 = [(-1, -1)]
SEL4 = [(-1, -1), (0, 0), (0, 1), (1, 1)]
NMAX = (4, 8, 16)


def frame_ms(g, frames):
    fn = g.api.lib.chem_debug_sq_frame_ms
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    ms = C.c_double(0.0)
    g._ck(fn(g.ctx, int(frames), C.byref(ms)))
    return ms.value


def host_ms(box, pos, nmax, n_total):
    """The total |rho|^2 on the host in fp64, vectors in blocks so that the phase matrix stays in cache-sized pieces; milliseconds
    scaled linearly from len(pos) to n_total particles."""
    n = sq_vectors(nmax).astype(np.float64)
    f = (pos / box).T.copy()
    t0 = time.perf_counter()
    out = np.empty(len(n))
    for k0 in range(0, len(n), 256):
        th = 2.0 * np.pi * (n[k0:k0 + 256] @ f)
        out[k0:k0 + 256] = np.cos(th).sum(axis=1) ** 2 + np.sin(th).sum(axis=1) ** 2
    return 1e3 * (time.perf_counter() - t0) * n_total / len(pos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--prec", type=int, default=0)
    ap.add_argument("--system", default="both")
    ap.add_argument("--n5", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=10000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    systems = []
    if a.system in ("c3", "both"):
        systems.append(("C3", W.polymer_melt(n_chains=4000, chain_len=32, seed=3)))
    if a.system in ("c5", "both"):
        systems.append(("C5", W.reactive_melt(n=a.n5, rho=0.8, interval=500, seed=2, skin=0.3)))
    rows = []
    for name, spec in systems:
        for prec in ((32, 64) if a.prec == 0 else (a.prec,)):
            g = Engine(device=0, precision=prec)
            W.apply(spec, g, reactions=False)
            g.run(a.warmup)
            g.sync()
            t0 = time.perf_counter()
            g.run(a.steps)
            g.sync()
            step_ms = 1e3 * (time.perf_counter() - t0) / a.steps
            pos, box = g.get_state("POS"), g.box()
            row = dict(system=name, n=int(spec["n"]), precision=prec, steps=a.steps, step_ms=round(step_ms, 4), frames=[])
            for nmax in NMAX:
                hm = host_ms(box, pos[:a.host_n], nmax, int(spec["n"]))
                for sel, label in ((SEL1, "1 selector"), (SEL4, "4 selectors")):
                    g.sq_init(nmax, sel)
                    frame_ms(g, 1)                       # (the first frame allocates the scratch and sets the LDS attribute)
                    ms = frame_ms(g, a.frames)
                    r = g.sq()
                    assert r["frames"] == a.frames + 1 and np.isfinite(r["sums"]).all()
                    row["frames"].append(dict(nmax=nmax, nvec=int(r["nvec"]), conf=label, frame_ms=round(ms, 4), md_steps=round(ms / step_ms, 2),
                                              host_numpy_ms_1sel=round(hm, 1)))
                g.sq_init(1, [])
            g.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("system n prec step_ms | nmax nvec selectors frame_ms md_steps host_numpy_ms(1 selector, scaled from %d particles)\n" % a.host_n)
            for row in rows:
                for fr in row["frames"]:
                    f.write("%s %d fp%d %.4f | %d %d %s %.4f %.2f %.1f\n" % (row["system"], row["n"], row["precision"], row["step_ms"], fr["nmax"], fr["nvec"],
                                                                            fr["conf"].split()[0], fr["frame_ms"], fr["md_steps"], fr["host_numpy_ms_1sel"]))


if __name__ == "__main__":
    main()
