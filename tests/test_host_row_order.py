"""CPU-only tests of the row-order rule of chemlab_amd/csrc/chem_roworder_host.hpp (option row_order): the rows of a tile's
force list are stored ascending by (chunks of eight entries, natural index), except that the R = nh - (ceil(nh / P) - 1) P
shortest fill the last, partly filled pass of P lanes and the others the full passes in ascending order.  The rule is
compared with a brute-force model written here (a Python sort); the harness is compiled with g++ from tests/host/ and
answers both through the host's counting sort and through the pieces the kernels use (ranks per class and wave-pass)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H

P = 512


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "roworder_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "roworder_harness.cpp"), "-o", exe])
    return exe


def model(cnt, p):
    """qnat[position] = home, by the rule's words."""
    nh = len(cnt)
    if nh == 0:
        return []
    asc = sorted(range(nh), key=lambda i: (-(-cnt[i] // 8), i))
    npass = -(-nh // p)
    r = nh - (npass - 1) * p
    return asc[r:] + asc[:r]          # full passes: the remaining rows ascending; last pass: the R shortest


def ask(harness, cases):
    """cases: (P, counts).  Both answers of the harness for every case."""
    lines = []
    for p, cnt in cases:
        tail = " ".join("%d" % c for c in cnt)
        lines += ["order %d %d %s" % (p, len(cnt), tail), "device %d %d %s" % (p, len(cnt), tail)]
    out = H.run_harness(harness, lines)
    return [([int(w) for w in out[2 * k][1:]], [int(w) for w in out[2 * k + 1][1:]]) for k in range(len(cases))]


def check(harness, cases):
    for (p, cnt), (host, dev) in zip(cases, ask(harness, cases)):
        nh = len(cnt)
        assert sorted(host) == list(range(nh)), "not a permutation (nh %d, P %d)" % (nh, p)
        assert host == model(cnt, p), (nh, p)
        assert dev == host, "the kernels' arithmetic disagrees with the host's (nh %d, P %d)" % (nh, p)
        # the placement, said once more without the model: chunks ascend inside the full passes and inside the last pass,
        # and no row of the last pass is longer than a row of a full pass
        k = [-(-cnt[i] // 8) for i in host]
        nfull = (-(-nh // p) - 1) * p if nh else 0
        assert k[:nfull] == sorted(k[:nfull]) and k[nfull:] == sorted(k[nfull:])
        if nfull and nh > nfull:
            assert max(k[nfull:]) <= min(k[:nfull])


SIZES = (0, 1, P, P + 1, P + 66, 2 * P + 3)


@pytest.mark.parametrize("nh", SIZES)
def test_sizes_with_melt_like_rows(harness, nh):
    """Row lengths as the melt has them (mean 47, sigma 8, clipped to 19..78) at every size that changes the pass structure."""
    rng = np.random.default_rng(100 + nh)
    cases = [(P, [int(c) for c in np.clip(rng.normal(46.9, 7.9, nh).round(), 19, 78)]) for _ in range(4)]
    check(harness, cases)


@pytest.mark.parametrize("nh", SIZES)
def test_all_rows_equal(harness, nh):
    """Nothing to sort: the full passes hold homes R .. nh-1, the last pass homes 0 .. R-1 (ties resolve by natural index)."""
    cases = [(P, [c] * nh) for c in (0, 1, 8, 9, 47)]
    check(harness, cases)
    for (p, cnt), (host, _) in zip(cases, ask(harness, cases)):
        r = nh - (-(-nh // P) - 1) * P if nh else 0
        assert host == list(range(r, nh)) + list(range(r))


@pytest.mark.parametrize("nh", (1, 20, 31))
def test_all_rows_distinct(harness, nh):
    """Every row in a chunk class of its own (8 k entries, k = 0 .. nh-1 shuffled): the order is the sort itself."""
    rng = np.random.default_rng(7)
    cases = []
    for p in (4, 8, 64):
        k = rng.permutation(nh)
        cases.append((p, [int(8 * v) for v in k]))
    check(harness, cases)


@pytest.mark.parametrize("nh", SIZES)
def test_rows_of_zero_length(harness, nh):
    """Inert home particles (no entry at all) among ordinary rows, and tiles of nothing else."""
    rng = np.random.default_rng(200 + nh)
    mixed = [int(c) for c in np.where(rng.random(nh) < 0.3, 0, rng.integers(1, 79, nh))]
    check(harness, [(P, mixed), (P, [0] * nh)])


def test_ties_resolve_by_natural_index(harness):
    """Counts 1..8 are one class, 9..16 the next: inside a class the natural index decides, whatever the counts."""
    cnt = [16, 3, 9, 8, 1, 12, 7, 10, 0, 2]
    (host, dev), = ask(harness, [(4, cnt)])
    # classes: 0 -> [8]; 1 -> [1, 3, 4, 6, 9]; 2 -> [0, 2, 5, 7].  nh 10, P 4: three passes, R = 2
    asc = [8, 1, 3, 4, 6, 9, 0, 2, 5, 7]
    assert host == asc[2:] + asc[:2] and dev == host
    check(harness, [(4, cnt), (3, cnt), (10, cnt), (16, cnt)])


def test_other_pass_sizes_and_crowded_tiles(harness):
    """P = 256 and 1024 (the force kernel's other workgroup sizes), tiles past two and three passes, wave-pass edges."""
    rng = np.random.default_rng(3)
    cases = []
    for p in (256, 512, 1024):
        for nh in (63, 64, 65, p - 1, 2 * p, 2 * p + 1, 3 * p + 17, 2047, 2048):
            cases.append((p, [int(c) for c in rng.integers(0, 249, nh)]))
    check(harness, cases)


def test_last_pass_size(harness):
    out = H.run_harness(harness, ["last %d %d" % (P, nh) for nh in (0, 1, P - 1, P, P + 1, P + 66, 2 * P, 2 * P + 3)])
    assert [int(w[1]) for w in out] == [0, 1, P - 1, P, 1, 66, P, 3]


def test_plan_and_switch(harness):
    out = H.run_harness(harness, ["plan 1000000 46656 27 4608", "plan 8000 512 27 1024", "plan 100 729 27 1024", "plan 4000000 1000 27 20000",
                                  "on 1 1 1 0 192", "on 0 1 1 0 192", "on 1 0 1 0 192", "on 1 1 0 0 192", "on 1 1 1 1 192",
                                  "on 1 1 1 0 248", "on 1 1 1 0 256"])
    v = [int(w[1]) for w in out]
    # twice a full tile of 27 cells at the mean occupancy + 64, never beyond the tile's slots or 2048 homes
    assert v[:4] == [2 * 579 + 64, 2 * 422 + 64, 72, 2048]
    assert H.run_harness(harness, ["plan 8000 512 27 800"])[0][1] == "800"
    # single domain, fused, tiles, and a row stride whose chunk counts fit the 32 classes (8 * 31 entries)
    assert v[4:] == [1, 0, 0, 0, 0, 1, 0]
