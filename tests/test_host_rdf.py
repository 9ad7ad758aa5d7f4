"""Radial distribution functions, host side: chemlab_amd/csrc/chem_rdf_host.hpp (edges, the bin of a squared distance, selector
masks, the normaliser M, validation, LDS budget and launch plan) against tests/rdf_ref.py.  Nothing here needs a GPU.  The
harness is compiled with g++ from tests/host/, once more with -fsanitize=address,undefined as a stand-alone program."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rdf_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "rdf_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "rdf_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "rdf_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = [x.split() for x in out.stdout.split("\n") if x]
    assert len(res) == len(lines)
    return res


def dbits(x):
    return "%d" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.mark.parametrize("r_max,nbins", [(2.5, 256), (1.5, 1024), (2.0, 32), (0.7, 1), (2.8, 100), (1.0 / 3.0, 7)])
def test_edges_and_bins_against_the_reference(harness, r_max, nbins):
    """e2[k] bit for bit; the bin of random d2 values, of every edge value and of its neighbours one ulp below and above, of 0,
    of values far outside and of e2[nbins] itself."""
    dr = np.float64(r_max) / np.float64(nbins)
    e2 = RR.edges2(r_max, nbins)
    got = drive(harness, ["edge2 %s %d %d" % (dbits(dr), nbins, k) for k in range(nbins + 1)])
    assert [int(g[1]) for g in got] == [int(np.float64(v).view(np.uint64)) for v in e2]
    rng = np.random.default_rng(nbins)
    d2 = list(rng.uniform(0.0, 1.2 * e2[-1], 2000)) + list(rng.uniform(0.0, e2[min(3, nbins)], 200))
    for v in e2:
        d2 += [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)] if v > 0 else [v, np.nextafter(v, np.inf)]
    d2 += [0.0, 5e-324, 1e300, 4.0 * e2[-1], np.inf]
    d2 = np.array(d2, dtype=np.float64)
    got = drive(harness, ["bin %s %d %s" % (dbits(dr), nbins, dbits(v)) for v in d2])
    want = RR.bin_of(d2, e2)
    assert [int(g[1]) for g in got] == [int(k) for k in want]
    assert (want == -1).sum() > 100 and (want == nbins - 1).sum() >= 1 and (want == 0).sum() >= 1


def test_selector_masks_and_normalisers(harness):
    rng = np.random.default_rng(9)
    sels = [[(-1, -1)], [(0, 0), (0, 1), (1, 1), (-1, -1)], [(3, -1), (-1, 3), (15, 0), (0, 15), (7, 7), (-1, -1), (2, 5), (5, 2)]]
    for sel in sels:
        flat = " ".join("%d %d" % s for s in sel)
        pairs = [(a, b) for a in range(16) for b in range(16)]
        got = drive(harness, ["mask %d %s %d %d" % (len(sel), flat, a, b) for a, b in pairs])
        for (a, b), g in zip(pairs, got):
            want = sum(1 << s for s, t in enumerate(sel) if RR.matches(t, np.int64(a), np.int64(b)))
            assert int(g[1]) == want, (sel, a, b)
        for _ in range(6):
            c = rng.integers(0, 2000, 16) * (rng.uniform(size=16) < 0.5)
            types = np.repeat(np.arange(16), c)
            got = drive(harness, ["norm %d %s %s" % (len(sel), flat, " ".join("%d" % v for v in c))])[0]
            assert [int(v) for v in got[1:]] == [RR.norm_pairs(t, types) for t in sel]
    # a million particles of one type: M needs more than 32 bits
    c = [0] * 16
    c[2] = 1 << 20
    got = drive(harness, ["norm 1 -1 -1 " + " ".join("%d" % v for v in c)])[0]
    assert int(got[1]) == (1 << 20) * ((1 << 20) - 1) // 2


def test_validation(harness):
    ok = ["valid %s 256 1 -1 -1" % dbits(2.5), "valid %s 1024 8 %s" % (dbits(1.0), " ".join(["0 15"] * 8)), "valid %s 1 1 0 0" % dbits(1e-3),
          "valid %s 0 0" % dbits(0.0)]                       # (npairs = 0 switches off: nothing else is looked at)
    bad = ["valid %s 256 1 -1 -1" % dbits(v) for v in (0.0, -1.0, np.inf, np.nan)]
    bad += ["valid %s %d 1 -1 -1" % (dbits(2.5), nb) for nb in (0, -3, 1025)]
    bad += ["valid %s 256 %d -1 -1" % (dbits(2.5), k) for k in (-1, 9)]
    bad += ["valid %s 256 1 %d %d" % (dbits(2.5), a, b) for a, b in ((-2, 0), (0, 16), (16, -1))]
    assert [int(g[1]) for g in drive(harness, ok)] == [0] * len(ok)
    assert [int(g[1]) for g in drive(harness, bad)] == [EINVAL] * len(bad)


def test_launch_plan_and_its_refusals(harness):
    budget, ncu = 150 * 1024, 256
    # tiles: the histogram behind the image, a persistent grid of at most two workgroups per compute unit
    g = drive(harness, ["plan 0 256 1 1 40016 %d %d 1000" % (budget, ncu)])[0]
    assert g[:2] == ["plan", "ok"] and [int(v) for v in g[2:]] == [512, 512, 40016, 40016 + 1024]
    g = drive(harness, ["plan 0 256 1 1 40016 %d %d 100" % (budget, ncu)])[0]
    assert int(g[2]) == 100                                             # never more workgroups than tiles
    g = drive(harness, ["plan 0 1024 8 2 40010 %d %d 5000" % (budget, ncu)])[0]
    assert [int(v) for v in g[2:]] == [256, 512, 40016, 40016 + 65536]      # 16-byte aligned; one workgroup per compute unit
    # per-cell and brute-force lists: chunks of 256 staged particles (36 bytes each)
    g = drive(harness, ["plan 1 1024 8 2 0 %d %d 343" % (budget, ncu)])[0]
    assert [int(v) for v in g[2:]] == [2, 256, 9216, 9216 + 65536]
    refused = ["plan 0 1024 8 2 90000 %d %d 1000" % (budget, ncu),      # fp64 image of a full tile + 64 KB
               "plan 0 0 1 1 40016 %d %d 1000" % (budget, ncu), "plan 0 1025 1 1 40016 %d %d 1000" % (budget, ncu),
               "plan 0 256 0 1 40016 %d %d 1000" % (budget, ncu), "plan 0 256 9 1 40016 %d %d 1000" % (budget, ncu),
               "plan 1 256 1 3 0 %d %d 1000" % (budget, ncu), "plan 1 1024 8 2 0 65536 %d 1000" % ncu,
               "plan 1 256 1 1 0 %d %d 65537" % (budget, ncu)]            # the all-pairs pass stops at 65536 particles
    assert [g[1] for g in drive(harness, refused)] == ["refused"] * len(refused)
    assert drive(harness, ["plan 0 512 8 2 90000 %d %d 1000" % (budget, ncu)])[0][1] == "ok"
    assert drive(harness, ["plan 1 256 1 1 0 %d %d 65536" % (budget, ncu)])[0][1] == "ok"
    assert drive(harness, ["plan 0 256 1 1 40016 %d %d 10000000" % (budget, ncu)])[0][1] == "ok"      # (tiles: no such limit)
