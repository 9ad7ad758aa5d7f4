"""CPU-only tests of the host rule of chemlab_amd/csrc/chem_idle_host.hpp: does step s get its neighbour launch, given the
state the device published about an earlier step?  (CtxT::run calls it once per step on the single-domain fused path; the
device decides on every step whatever the rule says, so a wrong answer costs time, never a result -- tests/test_gpu_skip_idle.py.)
The rule is compared with a brute-force model written here: the accumulated distance is carried forward one step at a time
with kappa times the published displacement, and one step beyond s.  The harness is compiled with g++ from tests/host/."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H

HALF_SKIN, KAPPA = 0.245, 1.25        # the flagship's list skin 0.49; the default allowance


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "idle_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(root, "tests", "host", "idle_harness.cpp"), "-o", exe])
    return exe


def line(p, acc, d, s, gen=3, host_gen=3, halted=0, requested=0, diagnostics=0, half_skin=HALF_SKIN, kappa=KAPPA):
    return "launch %d %s %s %d %d %d %d %d %d %s %s" % (p, H.dbits(acc), H.dbits(d), gen, halted, host_gen, requested, diagnostics, s,
                                                       H.dbits(half_skin), H.dbits(kappa))


def launches(harness, lines):
    return [int(w[1]) for w in H.run_harness(harness, lines)]


def model_bound(p, acc, d, s, kappa):
    """Steps p + 1 .. s and one more, each adding kappa * d."""
    for _ in range(p + 1, s + 2):
        acc += kappa * d
    return acc


def draws(rng, k):
    """(p, acc, d, s): hints 1..30 steps old, distances around the flagship's (0.019 per step against 0.245)."""
    p = rng.integers(0, 1 << 40, k)
    return [(int(p[i]), float(rng.uniform(0, 0.3)), float(rng.uniform(0, 0.04)), int(p[i] + rng.integers(1, 31))) for i in range(k)]


def test_skips_exactly_where_the_model_stays_inside_the_budget(harness):
    rng = np.random.default_rng(1)
    cases = draws(rng, 4000)
    got = launches(harness, [line(p, acc, d, s) for p, acc, d, s in cases])
    nskip = 0
    for (p, acc, d, s), launch in zip(cases, got):
        b = model_bound(p, acc, d, s, KAPPA)
        if abs(b - HALF_SKIN) < 1e-12:       # (the model adds, the rule multiplies: equal up to rounding)
            continue
        assert launch == (1 if b > HALF_SKIN else 0), (p, acc, d, s, b)
        nskip += 1 - launch
    assert 100 < nskip < 3900       # both answers are exercised


def test_never_skips_beyond_the_budget_whatever_the_skin_and_allowance(harness):
    rng = np.random.default_rng(2)
    cases = draws(rng, 3000)
    hs = rng.uniform(0.05, 0.4, len(cases)); ka = rng.uniform(1.0, 1.6, len(cases))
    got = launches(harness, [line(p, acc, d, s, half_skin=float(h), kappa=float(k)) for (p, acc, d, s), h, k in zip(cases, hs, ka)])
    for (p, acc, d, s), h, k, launch in zip(cases, hs, ka, got):
        if model_bound(p, acc, d, s, float(k)) > float(h) * (1 + 1e-12):
            assert launch == 1, (p, acc, d, s, h, k)
        # ... and the bound is never below what the plain criterion would have accumulated with the published displacement
        assert model_bound(p, acc, d, s, float(k)) >= acc + (s - p) * d


def test_never_skips_without_a_valid_older_hint_of_this_generation(harness):
    p, acc, d = 1000, 0.01, 0.001            # comfortably inside: skipped when everything is in order
    ok = line(p, acc, d, p + 1)
    bad = [line(p, acc, d, p + 1, gen=2),                    # another generation (stale)
           line(p, acc, d, p + 1, host_gen=4),
           line(-1, acc, d, p + 1),                          # nothing published
           line(p, acc, d, p),                               # not older than s
           line(p, acc, d, p - 5),                           # from the future
           line(p, float("nan"), d, p + 1), line(p, acc, float("nan"), p + 1),
           line(p, float("inf"), d, p + 1), line(p, acc, float("inf"), p + 1),
           line(p, -0.5, d, p + 1), line(p, acc, -1e-3, p + 1),
           line(p, acc, d, p + 1, requested=1),              # the host asked for a rebuild itself
           line(p, acc, d, p + 1, diagnostics=1),            # want32 / debug_stamps
           line(p, acc, d, p + 1, kappa=0.5), line(p, acc, d, p + 1, kappa=float("nan")),
           line(p, acc, d, p + 1, half_skin=0.0), line(p, acc, d, p + 1, half_skin=float("nan"))]
    got = launches(harness, [ok] + bad)
    assert got[0] == 0
    assert got[1:] == [1] * len(bad)


def test_monotone_in_step_distance_and_displacement(harness):
    """Once the rule asks for the launch it keeps asking for it at every later step, larger accumulated distance and larger
    displacement."""
    rng = np.random.default_rng(3)
    lines, groups = [], []
    for p, acc, d, s in draws(rng, 300):
        ladder = ([(p, acc, d, s + k) for k in range(0, 24, 2)], [(p, acc + 0.02 * k, d, s) for k in range(12)],
                  [(p, acc, d * (1 + 0.25 * k), s) for k in range(12)])
        for lad in ladder:
            groups.append((len(lines), len(lad)))
            lines += [line(*c) for c in lad]
    got = launches(harness, lines)
    for at, k in groups:
        g = got[at:at + k]
        assert g == sorted(g), (lines[at], g)


def test_skips_comfortably_inside_the_budget(harness):
    """The flagship's figures: 0.019 per step against 0.245 -- the steps right behind a rebuild are skipped with a hint two
    or three steps old, the last ones of a list's life are not."""
    d = 0.019
    got = launches(harness, [line(100, k * d, d, 100 + lag) for k in range(13) for lag in (1, 2, 3)])
    for k in range(13):
        for j, lag in enumerate((1, 2, 3)):
            want = 1 if k * d + (lag + 1) * KAPPA * d > HALF_SKIN else 0
            assert got[3 * k + j] == want, (k, lag)
    assert got[:3 * 6] == [0] * 18 and got[-3:] == [1, 1, 1]


def test_look_ahead_freshness(harness):
    out = H.run_harness(harness, ["fresh 98 3 3 100 2", "fresh 97 3 3 100 2", "fresh 99 2 3 100 2", "fresh -1 3 3 1 2", "fresh 120 3 3 100 2"])
    assert [int(w[1]) for w in out] == [1, 0, 0, 0, 1]
