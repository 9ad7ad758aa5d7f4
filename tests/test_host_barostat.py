"""CPU-only tests of the barostat rules of chemlab_amd/csrc/chem_baro_host.hpp -- what k_baro_mu and CtxT::baro_step
(chem_api.hip) call: the pressure, mu against the formula, the refusal at mu^3 <= 0, the displacement charge of a scaling, and
the re-plan decision against cell_grid on boxes just either side of a cell-count threshold.  The harness is compiled with g++
from tests/host/."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "barostat_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "barostat_harness.cpp"), "-o", exe])
    return exe


def dval(word):
    return struct.unpack("<d", struct.pack("<Q", int(word)))[0]


def line(cmd, *xs):
    return cmd + " " + " ".join(H.dbits(x) if isinstance(x, float) else "%d" % x for x in xs)


def test_pressure_and_mu_against_the_formula(harness):
    rng = np.random.default_rng(11)
    cases = [(float(rng.uniform(1e-3, 1e-2)), float(rng.uniform(0.05, 5.0)), float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))) for _ in range(200)]
    out = H.run_harness(harness, [line("mu", *c) for c in cases])
    for (dt, tau, p0, p), o in zip(cases, out):
        m3 = 1.0 - (dt / tau) * (p0 - p)
        assert o[0] == "mu" and dval(o[1]) == m3 and o[2] == "1"
        # the cube root to one unit in the last place of either library
        assert abs(dval(o[3]) - m3 ** (1.0 / 3.0)) <= 2.3e-16 * dval(o[3])
        # cubed again: three times a cube root good to two units (2 x 2.3e-16) plus the two roundings of the products
        assert abs(dval(o[3]) ** 3 - m3) <= (3 * 2 + 1) * 2.3e-16 * m3
    pc = [(float(rng.uniform(0, 1e4)), float(rng.uniform(-1e4, 1e4)), float(rng.uniform(1, 1e5))) for _ in range(50)]
    for (k, w, v), o in zip(pc, H.run_harness(harness, [line("pressure", *c) for c in pc])):
        assert dval(o[1]) == (k + w) / (3.0 * v)
    # P == P0: the box stays exactly
    o = H.run_harness(harness, [line("mu", 0.004, 1.0, 0.75, 0.75)])[0]
    assert dval(o[1]) == 1.0 and dval(o[3]) == 1.0


def test_refusal_at_mu3_not_positive(harness):
    tau, dt = 1.0, 0.5
    cases = [(dt, tau, 2.0, 0.0),            # mu^3 == 0 exactly: 1 - 0.5 * 2
             (dt, tau, 2.0 + 1e-9, 0.0), (dt, tau, 1e6, 0.0), (dt, tau, float("nan"), 0.0), (dt, tau, 0.0, float("-inf")),
             (dt, tau, 2.0 - 1e-9, 0.0)]     # just positive: accepted, no clamp
    out = H.run_harness(harness, [line("mu", *c) for c in cases])
    assert dval(out[0][1]) == 0.0
    assert [o[2] for o in out] == ["0", "0", "0", "0", "0", "1"]
    assert 0.0 < dval(out[5][3]) < 1e-3


def test_displacement_charge(harness):
    rng = np.random.default_rng(12)
    cases = [(float(1.0 + rng.uniform(-2e-3, 2e-3)), float(rng.uniform(1.0, 3.0)), float(rng.uniform(0.1, 0.6))) for _ in range(100)] + [(1.0, 2.5, 0.3)]
    out = H.run_harness(harness, [line("charge", *c) for c in cases])
    for (mu, rc, se), o in zip(cases, out):
        c = dval(o[1])
        assert c == 0.5 * abs(mu - 1.0) * (rc + se)
        # two particles of a listed pair, each charged c: together they cover the change of the largest listed separation
        assert 2.0 * c >= abs(mu - 1.0) * (rc + se) * (1 - 1e-15)
    assert dval(out[-1][1]) == 0.0


@pytest.mark.parametrize("nc", [(5, 5, 5), (4, 4, 4), (3, 3, 3), (5, 4, 6)])
def test_replan_either_side_of_a_threshold(harness, nc):
    rl = 2.8
    for axis in range(3):
        for eps, expect_nc in ((+1e-9, nc[axis]), (-1e-9, nc[axis] - 1)):
            L = [n * rl * 1.3 for n in nc]
            L[axis] = nc[axis] * rl * (1.0 + eps)
            L = [float(x) for x in L]
            grid = [int(math.floor(x / rl)) for x in L]
            assert grid[axis] == expect_nc
            if min(grid) < 3:
                grid = [0, 0, 0]            # fewer than 3 cells on any axis: no cells at all
            o = H.run_harness(harness, [line("replan", *L, rl, *nc), line("replan", *L, rl, *grid)])
            assert [int(w) for w in o[0][2:]] == grid and [int(w) for w in o[1][2:]] == grid
            assert o[0][1] == ("0" if list(nc) == grid else "1")            # against the grid in force before the scaling
            assert o[1][1] == "0"                                           # against the grid a fresh context plans: nothing to do
