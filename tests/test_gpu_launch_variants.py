"""Every pair-force instantiation that options can select, on the device: k_pair_tiles MODE 0..3 at lanes per particle
{1, 2, 4, 8} x pair_block {256, 512, 1024}, forces and (MODE 0 and 3) the ENERGY launch of observe(), and k_pair_force at
{1, 16, 64} lanes in its plain and its CUBIC build.  The host picks the instantiation from chem_launch_host.hpp
(tests/test_host_launch_plan.py checks that rule on the CPU); here each pick is launched once and compared with the oracle.
MODE 4..7 and the bonded kernels are one instantiation each and have their own files (test_gpu_coulomb, test_gpu_resolution,
test_gpu_capped, test_gpu_coulomb14, test_gpu_hybrid_bonds, test_gpu_bonded).

System: 2048 particles (fcc 8^3 x 4, jitter 0.08) at rho = 0.7 with rc = 2.5, skin = 0.3: a box of 5.1 cells per axis, the
smallest the LDS tiles take (125 tiles, chem_debug_tiles is asserted), and about 64 neighbours per particle: eight 8-slot
chunks per row, so that all eight lanes of tpp = 8 carry pairs into the reduction (at rc = 1.5 two lanes would).  One
potential set per MODE: one LJ type (2), two LJ types with their own parameters (1), a linear table on the 1-1 pair (0), a
table of itype 3 on it (3) -- with columns linear in r, which the natural spline reproduces, so that the oracle's linear
interpolation is its reference (test_gpu_spline_tables.test_linear_data_matches_the_oracle).  A context is built once per
(precision, MODE, family); a case changes the two options and evaluates once.  Tolerances are test_gpu_parity's: forces TOL,
in fp32 TOL_MELT32 with the cutoff decisions set apart; epot_lj 1e-11 / 2e-6, epot_tab 1e-11 / 1e-4 relative."""
import ctypes

import numpy as np
import pytest

from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_parity import TOL, TOL_MELT32

pytestmark = pytest.mark.gpu

RC, SKIN = 2.5, 0.3
LJ2 = [(0, 0, 1.0, 1.0, RC), (0, 1, 0.8, 0.9, RC)]


def _spec(mode):
    spec = W.lj_melt(n=2048, rho=0.7, rc=RC, skin=SKIN, seed=40 + mode, jitter=0.08)
    spec["rebuild_criterion"] = 1
    if mode != 2:
        spec["types"] = np.random.default_rng(50 + mode).integers(0, 2, spec["n"]).astype(np.int32)
        spec["lj"] = LJ2 + ([(1, 1, 1.2, 0.95, RC)] if mode == 1 else [])
    if mode == 0:
        spec["tables"] = [(1, 1) + W.synthetic_table(nrow=1250, dr=0.002, rc=RC, eps=2.0, sigma=0.9) + (RC,)]
    if mode == 3:
        r = 0.05 * np.arange(1, 51)                          # rows to r = 2.5; both columns linear in r and zero at rc
        spec["tables"] = [(1, 1, 0.05, 0.05, 2.5 - r, 5.0 - 2.0 * r, RC)]
    return W.snap_to_grid(spec)                              # positions both builds and the oracle hold exactly


_SPEC, _REF, _ENG = {}, {}, {}


def _reference(oracle_mod, mode):
    """The oracle's forces and observables of the MODE's system, computed once."""
    if mode not in _REF:
        _SPEC[mode] = _spec(mode)
        o = oracle_mod.OracleEngine()
        W.apply(_SPEC[mode], o, thermostat=False)
        o.run(0)
        _REF[mode] = (o.get_state("FORCE"), o.observe())
        o.close()
        assert abs(_REF[mode][1]["epot_lj"]) > 1.0 and (mode in (1, 2) or abs(_REF[mode][1]["epot_tab"]) > 1.0)      # relative bounds mean something
    return _SPEC[mode], _REF[mode]


def _ntiles(g):
    out = (ctypes.c_int32 * 6)()
    g.api.lib.chem_debug_tiles.restype = ctypes.c_int64
    assert g.api.lib.chem_debug_tiles(ctypes.c_void_p(g.ctx), out) == 0
    return int(out[0])


@pytest.fixture(scope="module")
def engines():
    yield _ENG
    for g in _ENG.values():
        g.close()
    _ENG.clear()


def _engine(engines, spec, prec, mode, tiles):
    """The context of (precision, MODE, family), set up on first use."""
    key = (prec, mode, tiles)
    if key not in engines:
        from chemlab_amd.engine import Engine
        g = engines[key] = Engine(device=0, precision=prec)
        if not tiles:
            g.set_option("tiles", 0)
        W.apply(dict(spec, tables=[t + (3,) for t in spec["tables"]]) if mode == 3 else spec, g, thermostat=False)
        g.run(0)
        assert (_ntiles(g) > 0) == bool(tiles), _ntiles(g)
    return engines[key]


def _check(g, spec, ref, prec, mode, what):
    fo, oo = ref
    g.run(0)
    fg = g.get_state("FORCE")
    if prec == 64:
        err, flips = rel_err(fg, fo), 0
        assert err < TOL[64], (what, err)
    else:
        err, flips = force_error_without_cutoff_flips(spec, fg, fo, TOL_MELT32, max_flips=8)
        assert err < TOL_MELT32 and 0 <= flips <= 8, (what, err, flips)
    line = "%s fp%d: force %.2e, %d flips" % (what, prec, err, flips)
    if mode in (0, 3):
        og = g.observe()
        line += ", epot_lj %.2e, epot_tab %.2e" % (abs(og["epot_lj"] / oo["epot_lj"] - 1), abs(og["epot_tab"] / oo["epot_tab"] - 1))
        print(line)
        assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=1e-11 if prec == 64 else 2e-6), what
        assert og["epot_tab"] == pytest.approx(oo["epot_tab"], rel=1e-11 if prec == 64 else 1e-4), what
    else:
        print(line)


@pytest.mark.parametrize("tpp", [1, 2, 4, 8])
@pytest.mark.parametrize("pair_block", [256, 512, 1024])
@pytest.mark.parametrize("mode", [2, 1, 0, 3])
@pytest.mark.parametrize("prec", [64, 32])
def test_tile_kernel_variants_against_the_oracle(engines, oracle_mod, prec, mode, pair_block, tpp):
    spec, ref = _reference(oracle_mod, mode)
    g = _engine(engines, spec, prec, mode, tiles=1)
    g.set_option("pair_block", pair_block)
    g.set_option("tpp", tpp)
    _check(g, spec, ref, prec, mode, ("tiles", mode, pair_block, tpp))


@pytest.mark.parametrize("tpp", [1, 16, 64])
@pytest.mark.parametrize("mode", [0, 3], ids=["plain", "cubic"])
@pytest.mark.parametrize("prec", [64, 32])
def test_row_kernel_variants_against_the_oracle(engines, oracle_mod, prec, mode, tpp):
    """Option tiles = 0: one neighbour row per particle, k_pair_force and its CUBIC build."""
    spec, ref = _reference(oracle_mod, mode)
    g = _engine(engines, spec, prec, mode, tiles=0)
    g.set_option("tpp", tpp)
    _check(g, spec, ref, prec, mode, ("rows", mode, tpp))
