"""CPU-only tests of the Langevin-piston rules of chemlab_amd/csrc/chem_baro_host.hpp -- what k_baro_piston and
CtxT::baro_measure (chem_api.hip) call -- against tests/piston_ref.py on a table of inputs: momenta of both signs, gammaP = 0,
kT = 0, a huge momentum, NaN.  Finite results agree to a relative 1e-15 (exp and sqrt of either library are good to one unit in
the last place, the products add a few roundings of 1.1e-16 each -- measured against the sum of the absolute terms of G, so that
terms that cancel do not hide an error); piston_ok is false exactly where the momentum or a factor is not finite (or mu is 0:
1 / sqrt(mu) is not finite then).  The harness is compiled with g++ from tests/host/."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import piston_ref as PS

REL = 1e-15


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path_factory.mktemp("host")), "piston_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "piston_harness.cpp"), "-o", exe])
    return exe


def dval(word):
    return struct.unpack("<d", struct.pack("<Q", int(word)))[0]


def line(cmd, *xs):
    return cmd + " " + " ".join(H.dbits(x) for x in xs)


def test_factors_against_the_reference(harness):
    rng = np.random.default_rng(21)
    cases = [(float(rng.uniform(-500, 500)), float(10 ** rng.uniform(0, 4)), float(3 * rng.integers(1, 5000)), float(rng.uniform(5e-4, 8e-3))) for _ in range(200)]
    cases += [(0.0, 50.0, 6591.0, 0.004), (-0.0, 50.0, 3.0, 0.004)]
    out = H.run_harness(harness, [line("factors", *c) for c in cases])
    for (pe, w, nf, dt), o in zip(cases, out):
        sv, mu = dval(o[1]), dval(o[2])
        assert o[0] == "factors" and o[3] == "1"
        assert abs(sv - PS.piston_sv(pe, w, nf, dt)) <= REL * sv and abs(mu - PS.piston_mu(pe, w, dt)) <= REL * mu
        assert (sv < 1.0) == (pe > 0) or pe == 0                   # a growing box cools
        # sv^2 mu^c = 1: the two factors belong together
        assert abs(sv * sv * mu ** (1.0 + 3.0 / nf) - 1.0) <= 1e-13
    assert dval(out[-2][1]) == 1.0 and dval(out[-2][2]) == 1.0      # pe = 0: the plain velocity-Verlet step
    assert dval(out[-1][1]) == 1.0 and dval(out[-1][2]) == 1.0


def test_stop_exactly_where_something_is_not_finite(harness):
    nan, inf = float("nan"), float("inf")
    cases = [(1e3, 1e-12, 6591.0, 0.004),       # eps_dot dt = 4e12: mu overflows, sv underflows to 0
             (-1e3, 1e-12, 6591.0, 0.004),      # mu underflows to 0, sv overflows
             (-2e5, 1.0, 6591.0, 0.004),        # eps_dot dt = -800: mu = 0 while sv = exp(400) is still finite -- 1 / sqrt(mu) is not
             (nan, 50.0, 6591.0, 0.004), (inf, 50.0, 6591.0, 0.004), (-inf, 50.0, 6591.0, 0.004), (1.0, 50.0, 6591.0, nan),
             (1.7e5, 1.0, 6591.0, 0.004),       # eps_dot dt = 680: large and finite, accepted -- there is no clamp
             (-1.7e5, 1.0, 6591.0, 0.004), (1e300, 1e300, 3.0, 0.004)]
    out = H.run_harness(harness, [line("factors", *c) for c in cases])
    want = []
    for pe, w, nf, dt in cases:
        with np.errstate(all="ignore"):
            want.append("1" if PS.piston_ok(pe, PS.piston_mu(pe, w, dt), PS.piston_sv(pe, w, nf, dt)) else "0")
    assert want == ["0"] * 7 + ["1"] * 3
    assert [o[3] for o in out] == want
    for (pe, w, nf, dt), o in zip(cases, out):
        if o[3] == "1":
            assert math.isfinite(dval(o[1])) and math.isfinite(dval(o[2])) and dval(o[2]) > 0


def test_force_against_the_reference(harness):
    rng = np.random.default_rng(22)
    cases = []
    for k in range(200):
        gp = 0.0 if k % 4 == 0 else float(rng.uniform(0.1, 5.0))
        kT = 0.0 if k % 5 == 0 else float(rng.uniform(0.1, 3.0))
        cases.append((float(rng.uniform(1e2, 1e4)), float(rng.uniform(-10, 10)), float(rng.uniform(-10, 10)), float(3 * rng.integers(1, 5000)),
                      float(rng.uniform(0, 1e4)), gp, float(rng.uniform(-500, 500)), float(10 ** rng.uniform(0, 4)), kT,
                      float(rng.uniform(5e-4, 8e-3)), PS.u01(int(rng.integers(0, 2 ** 32)))))
    out = H.run_harness(harness, [line("force", *c) for c in cases])
    for c, o in zip(cases, out):
        vol, p, p0, nf, mv2, gp, pe, w, kT, dt, u = c
        g = PS.piston_force(*c)
        scale = 3.0 * vol * (abs(p) + abs(p0)) + (3.0 / nf) * mv2 + gp * abs(pe) + math.sqrt(24.0 * gp * w * kT / dt) * 0.5
        assert abs(dval(o[1]) - g) <= REL * scale
        assert abs(dval(o[2]) - (pe + dt * g)) <= REL * (abs(pe) + dt * scale)
        if gp == 0.0:           # no friction, no noise whatever kT and u are
            assert dval(o[1]) == 3.0 * vol * (p - p0) + (3.0 / nf) * mv2
    # kT = 0 with friction: the noise term vanishes, the friction stays
    c = (1000.0, 1.0, 1.0, 300.0, 0.0, 2.0, 7.0, 50.0, 0.0, 0.004, 0.9)
    assert dval(H.run_harness(harness, [line("force", *c)])[0][1]) == -14.0
    # NaN goes through (the stop is piston_ok's, on the momentum it produces)
    c = (1000.0, float("nan"), 1.0, 300.0, 0.0, 2.0, 7.0, 50.0, 0.0, 0.004, 0.9)
    assert math.isnan(dval(H.run_harness(harness, [line("force", *c)])[0][2]))


def test_draw_against_the_python_restatement(harness):
    cases = [(0, 0), (0, 1), (0x1234567887654321, 7), (2 ** 64 - 1, 2 ** 33 + 5), (12345, 10 ** 6)]
    out = H.run_harness(harness, ["draw %d %d" % c for c in cases])
    for (seed, step), o in zip(cases, out):
        assert tuple(int(x) for x in o[1:]) == PS.barostat_draw(seed, step)
