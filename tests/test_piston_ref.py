"""CPU checks of the Langevin piston's reference stepper (tests/piston_ref.py), numpy alone:

order        the conserved quantity H of a melt without thermostat and piston friction deviates by O(dt^2): the maximum
             deviation over the same stretch of time shrinks by a factor of about 4 per halving of dt, for three piston masses
             (a first-order discretisation -- scaling behind the kick, friction as a force -- gives 2);
first step   with pe = 0 the first step is the plain velocity-Verlet step, bit for bit;
guards       the cold lattice of tests/test_gpu_piston.py's list test crosses its cell-count threshold between steps 60 and 150
             with |mu - 1| < 2e-3: lists are still in use when the plan changes;
draw         barostat_draw in Python is chem_philox::barostat_draw of include/chem_philox.h."""
import os
import subprocess

import numpy as np
import pytest

import aged_ref as AR
import piston_ref as PS
import pressure_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLD_W = 16000.0           # piston mass of the cold-lattice runs (P0 = P_start +- pressure_ref.COLD_DP, gammaP = 0)
CELL = PR.COLD_RC + PR.COLD_SKIN


def _melt():
    spec = AR.melt_spec("melt2197", 0)
    return spec, PR.pressure(spec, spec["pos"], spec["vel"])["pressure"]


def run_h(spec, fn, p0, W, dt, nsteps):
    """(max |H - H_first|, |H|, relative box change) over nsteps steps from the spec's start."""
    x, v, L, pe = spec["pos"].copy(), spec["vel"].copy(), np.asarray(spec["box"], np.float64).copy(), 0.0
    f = fn(x, L)[0]
    hs = []
    for s in range(nsteps):
        o = PS.piston_step(spec, x, v, f, L, pe, fn, dt, p0, W, 0.0, 0.0, 0, s + 1)
        hs.append(PS.conserved(o, pe, dt, p0, W))
        x, v, f, L, pe = o["x"], o["v"], o["f"], o["L"], o["pe"]
    hs = np.asarray(hs)
    return float(np.abs(hs - hs[0]).max()), float(abs(hs[0])), float(L[0] / spec["box"][0] - 1.0)


@pytest.mark.parametrize("W", [50.0, 500.0, 5000.0])
def test_conserved_quantity_is_second_order(W):
    spec, p_start = _melt()
    fn = PS.energy_force_fn(spec)
    p0, dt = 0.5 * p_start, 0.004
    dev = [run_h(spec, fn, p0, W, dt / k, 30 * k) for k in (1, 2, 4)]
    print("W = %g: deviations %.3g / %.3g / %.3g on |H| = %.4g, factors %.2f and %.2f, box moved by %.2f %%" % (
        W, dev[0][0], dev[1][0], dev[2][0], dev[0][1], dev[0][0] / dev[1][0], dev[1][0] / dev[2][0], 100 * dev[0][2]))
    for a, b in ((dev[0], dev[1]), (dev[1], dev[2])):
        assert 3.0 <= a[0] / b[0] <= 5.0, (W, a[0], b[0])
    assert abs(dev[0][2]) > 1e-2                                             # the box really moves ...
    assert int(np.floor(spec["box"][0] * (1 + dev[0][2]) / (spec["rc"] + spec["skin"]))) == 5      # ... and stays on 5 cells per axis


def test_first_step_is_plain_velocity_verlet():
    spec, p_start = _melt()
    fn = PR.exact_force_fn(spec)
    x, v, L = spec["pos"].copy(), spec["vel"].copy(), np.asarray(spec["box"], np.float64).copy()
    f, _ = fn(x, L)
    o = PS.piston_step(spec, x, v, f, L, 0.0, fn, spec["dt"], 0.5 * p_start, 50.0, 1.0, 1.5, 7, 1)
    m = np.asarray(spec["mass"], np.float64)[:, None]
    dt = spec["dt"]
    vh = v + 0.5 * dt * f / m
    xn = x + dt * vh
    fnew, _ = fn(xn, L)
    vn = vh + 0.5 * dt * fnew / m
    assert o["sv"] == 1.0 and o["mu"] == 1.0
    assert np.array_equal(o["x"], xn) and np.array_equal(o["v"], vn) and np.array_equal(o["L"], L) and np.array_equal(o["f"], fnew)
    assert o["pe"] != 0.0                                                    # the piston has been kicked: the second step differs


def cold_crossing(direction, extra=0):
    """(step at which floor(L / 2.6) first changes, max |mu - 1| up to there, cells before, cells after)."""
    spec = PR.cold_lattice(direction)
    p_start = PR.pressure(spec, spec["pos"], spec["vel"])["pressure"]
    p0 = p_start + (PR.COLD_DP if direction == "shrink" else -PR.COLD_DP)
    fn = PR.exact_force_fn(spec)
    x, v, L, pe = spec["pos"].copy(), spec["vel"].copy(), spec["box"].copy(), 0.0
    f, _ = fn(x, L)
    n0 = int(np.floor(L[0] / CELL))
    worst = 0.0
    for s in range(1, 201):
        o = PS.piston_step(spec, x, v, f, L, pe, fn, spec["dt"], p0, COLD_W, 0.0, 0.0, 0, s)
        worst = max(worst, abs(o["mu"] - 1.0))
        x, v, f, L, pe = o["x"], o["v"], o["f"], o["L"], o["pe"]
        if int(np.floor(L[0] / CELL)) != n0:
            return s, worst, n0, int(np.floor(L[0] / CELL))
    return None, worst, n0, n0


@pytest.mark.parametrize("direction", ["shrink", "grow"])
def test_guard_of_the_lists_follow_the_box_test(direction):
    s, worst, n0, n1 = cold_crossing(direction)
    print("%s: cell count %d -> %d at step %s, max |mu - 1| = %.3g" % (direction, n0, n1, s, worst))
    assert (n0, n1) == ((5, 4) if direction == "shrink" else (4, 5))
    assert s is not None and 60 <= s <= 150
    assert worst < 2e-3


def test_barostat_draw_matches_the_header(tmp_path):
    cases = [(0, 0), (0, 1), (0x1234567887654321, 7), (2 ** 64 - 1, 2 ** 33 + 5)]
    src = tmp_path / "draw.cpp"
    src.write_text('#include <cstdio>\n#include "chem_philox.h"\nint main() {\n  uint32_t o[4];\n' +
                   "".join("  chem_philox::barostat_draw(%dull, %dull, o); printf(\"%%u %%u %%u %%u\\n\", o[0], o[1], o[2], o[3]);\n" % c for c in cases) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "draw")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for (seed, step), line in zip(cases, out):
        assert tuple(int(x) for x in line.split()) == PS.barostat_draw(seed, step)
    # a domain of its own: not the ATRP draw of tag 0, not the Langevin draw of tag 0
    import react_ref as RR
    assert PS.barostat_draw(5, 9) != tuple(RR.atrp_draw(5, 9, 0))
