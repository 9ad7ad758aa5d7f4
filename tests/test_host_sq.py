"""Static structure factor, host side: chemlab_amd/csrc/chem_sq_host.hpp (the enumeration of the wave vectors and its inverse,
validation, the selector -> class table, the launch plan) against tests/sq_ref.py.  Nothing here needs a GPU.  The harness is
compiled with g++ from tests/host/, once more with -fsanitize=address,undefined as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import sq_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
BUDGET, NCU = 150 * 1024, 256
SCRATCH_MAX = 32 << 20


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "sq_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "sq_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "sq_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    res = [x.split() for x in out.stdout.split("\n") if x]
    assert len(res) == len(lines)
    return res


@pytest.mark.parametrize("nmax", [1, 2, 3, 16])
def test_enumeration_is_a_bijection_onto_the_canonical_half(harness, nmax):
    """Every k maps to a kept vector inside the range, in strictly increasing lexicographic order, and back to k (the harness's
    own sweep); the vectors themselves equal the reference's triple loop; what is not kept has no index."""
    want = SR.vectors(nmax)
    nv = ((2 * nmax + 1) ** 3 - 1) // 2
    assert [int(v) for v in drive(harness, ["nvec %d" % nmax])[0][1:]] == [nv] and len(want) == nv
    assert [int(v) for v in drive(harness, ["enum %d" % nmax])[0][1:]] == [nv, 0]
    ks = list(range(nv)) if nmax <= 3 else sorted(set(np.random.default_rng(1).integers(0, nv, 600).tolist() + [0, 15, 16, 16 + 33 * 16 - 1, 16 + 33 * 16, nv - 1]))
    got = drive(harness, ["vec %d %d" % (nmax, k) for k in ks])
    assert [[int(v) for v in g[1:]] for g in got] == want[ks].tolist()
    got = drive(harness, ["index %d %d %d %d" % ((nmax,) + tuple(want[k])) for k in ks])
    assert [int(g[1]) for g in got] == ks
    outside = [(0, 0, 0), (0, 0, -1), (0, -1, 1), (-1, 0, 0), (-1, 1, 1), (nmax + 1, 0, 0), (1, nmax + 1, 0), (1, 0, -nmax - 1), (0, 0, nmax + 1)]
    assert [int(g[1]) for g in drive(harness, ["index %d %d %d %d" % ((nmax,) + v) for v in outside])] == [-1] * len(outside)


def test_counts_of_the_rule_set(harness):
    assert [int(g[1]) for g in drive(harness, ["nvec %d" % k for k in (1, 3, 8, 16)])] == [13, 171, 2456, 17968]


def test_validation(harness):
    ok = ["valid 1 1 -1 -1", "valid 16 4 0 15 15 0 -1 3 7 7", "valid 8 2 0 0 0 1", "valid 0 0", "valid 99 0 null"]      # (npairs = 0 switches off: nothing else is looked at)
    bad = ["valid %d 1 -1 -1" % k for k in (0, -1, 17, 1000)]
    bad += ["valid 4 %d -1 -1" % k for k in (-1, 5, 9)]
    bad += ["valid 4 1 %d %d" % t for t in ((-2, 0), (0, 16), (16, -1))]
    bad += ["valid 4 1 null", "valid 4 3 null"]
    assert [int(g[1]) for g in drive(harness, ok)] == [0] * len(ok)
    assert [int(g[1]) for g in drive(harness, bad)] == [EINVAL] * len(bad)


def test_class_table_of_overlapping_selectors(harness):
    g = drive(harness, ["classes 4 -1 -1 0 0 0 1 -1 1"])[0]
    a, b, c = " ".join(g[1:]).split("|")
    assert [int(v) for v in a.split()] == [3, -1, 0, 1]                               # three distinct sets: any, {0}, {1}
    assert [int(v) for v in b.split()] == [0, 0, 1, 1, 1, 2, 0, 2]
    assert [int(v) for v in c.split()] == [0b011, 0b101] + [0b001] * 14               # type 0: any and {0}; type 1: any and {1}; the rest: any
    g = drive(harness, ["classes 4 0 1 2 3 4 5 6 7"])[0]                              # the most: eight sets, a particle in one at the most
    a, b, c = " ".join(g[1:]).split("|")
    assert [int(v) for v in a.split()] == [8] + list(range(8)) and [int(v) for v in b.split()] == list(range(8))
    assert [int(v) for v in c.split()] == [1 << t for t in range(8)] + [0] * 8
    g = drive(harness, ["classes 1 5 5"])[0]
    assert " ".join(g[1:]).split("|")[0].split() == ["1", "5"]
    cnt = [0] * 16
    cnt[0], cnt[1], cnt[4] = 700, 300, 24
    g = drive(harness, ["count 4 -1 -1 0 0 0 1 -1 1 " + " ".join(str(v) for v in cnt)])[0]
    assert [int(v) for v in g[1:]] == [1024, 1024, 700, 700, 700, 300, 1024, 300]
    big = [0] * 16
    big[2] = 1 << 33
    assert [int(v) for v in drive(harness, ["count 1 -1 2 " + " ".join(str(v) for v in big)])[0][1:]] == [1 << 33, 1 << 33]


def test_launch_plan_fits_every_configuration(harness):
    """n = 1, 63, 64, 65, 10^6 with every nmax, one and eight classes: nothing refused, the scratch at most 32 MB (what the plan
    uses and what is allocated for any n), the LDS inside the budget, the super-chunks whole 64-particle chunks that cover n
    with none empty."""
    cases = [(n, nmax, ncls) for n in (1, 63, 64, 65, 10 ** 6) for nmax in range(1, 17) for ncls in (1, 2, 8)]
    got = drive(harness, ["plan %d %d %d %d %d" % (n, nmax, ncls, BUDGET, NCU) for n, nmax, ncls in cases])
    for (n, nmax, ncls), g in zip(cases, got):
        assert g[1] == "ok", (n, nmax, ncls)
        nqb, nsuper, per, block, lds, scratch, cap = [int(v) for v in g[2:]]
        nvec = ((2 * nmax + 1) ** 3 - 1) // 2
        assert block == 256 and nqb == -(-nvec // 512)
        assert lds == 3 * 64 * (nmax + 1) * 16 <= BUDGET
        assert scratch == nsuper * ncls * nvec * 16 <= cap <= SCRATCH_MAX
        assert per % 64 == 0 and nsuper >= 1 and (nsuper - 1) * per < n <= nsuper * per
        if n <= 65:
            assert nsuper == -(-n // 64) and per == 64
    # a million particles at nmax = 1 spread over the device; at nmax = 16 with eight classes the scratch bound decides
    g = [int(v) for v in drive(harness, ["plan 1000000 1 1 %d %d" % (BUDGET, NCU)])[0][2:]]
    assert g[0] == 1 and g[1] >= 4 * NCU - 64
    g = [int(v) for v in drive(harness, ["plan 1000000 16 8 %d %d" % (BUDGET, NCU)])[0][2:]]
    assert g[0] == 36 and g[1] <= SCRATCH_MAX // (8 * 17968 * 16) == 14
    refused = ["plan 0 4 1 %d %d" % (BUDGET, NCU), "plan 100 0 1 %d %d" % (BUDGET, NCU), "plan 100 17 1 %d %d" % (BUDGET, NCU),
               "plan 100 4 0 %d %d" % (BUDGET, NCU), "plan 100 4 9 %d %d" % (BUDGET, NCU), "plan 100 16 1 50000 %d" % NCU]
    assert [g[1] for g in drive(harness, refused)] == ["refused"] * len(refused)
