"""CPU-side checks of the Langevin piston's entry points (include/chem_mi355.h chem_barostat_langevin,
chem_barostat_state_get): the symbols are exported and bound with the header's signatures, the state struct has the C compiler's
layout, the CPU checker refuses by name, and the shim class espp.integrator.LangevinBarostat pushes its attributes to the
engine (a stub that records calls)."""
import ctypes as C
import os
import subprocess

import pytest

from chemlab_amd import _capi, espp
from test_host_coulomb import StubEngine, shim_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("barostat_langevin", "barostat_state_get")


def test_symbols_exported_and_bound():
    api = _capi.load()
    for name in NAMES:
        assert hasattr(api.lib, "chem_" + name), name
        assert name in api.exported() and name not in _capi.SIGNATURES          # the CPU oracle has a fixed box: product only
    assert api.barostat_langevin.argtypes == [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_uint64]
    assert api.barostat_state_get.argtypes == [C.c_void_p, C.POINTER(_capi.BarostatState)]
    assert api.abi_version() == 1
    assert {"chem_" + n for n in NAMES} <= set(_capi.header_symbols())


def test_state_layout_matches_the_header(tmp_path):
    assert C.sizeof(_capi.BarostatState) == 48                    # LP64: int32 + padding, 5 x double
    fields = [n for n, _ in _capi.BarostatState._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(chem_barostat_state));\n' +
                   "".join('  printf("%%zu\\n", offsetof(chem_barostat_state, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 48
    assert out[1:] == [getattr(_capi.BarostatState, f).offset for f in fields]


def test_cpu_checker_refuses_by_name(oracle_mod):
    o = oracle_mod.OracleEngine()
    with pytest.raises(NotImplementedError, match=r"LangevinBarostat: the CPU checker has no barostat \(its box is fixed\)"):
        o.barostat_langevin(1.0, 50.0, 1.0, 1.5, 7)
    with pytest.raises(NotImplementedError, match=r"LangevinBarostat: the CPU checker has no barostat \(its box is fixed\)"):
        o.barostat_state()


def test_shim_class_pushes_to_the_engine():
    eng = StubEngine()
    system = shim_system(eng)
    system.rng = espp.esutil.RNG(4711)
    b = espp.integrator.LangevinBarostat(system, system.rng, 1.25)
    b.gammaP, b.mass, b.pressure = 1.0, 50.0, 0.06                        # before addExtension: nothing reaches the engine
    assert (b.gammaP, b.mass, b.pressure) == (1.0, 50.0, 0.06)
    assert not [c for c in eng.calls if c[0] == "barostat_langevin"]
    integrator = espp.integrator.VelocityVerlet(system)
    integrator.addExtension(b)
    assert [c for c in eng.calls if c[0] == "barostat_langevin"] == [("barostat_langevin", (0.06, 50.0, 1.0, 1.25, 4711), {})]
    b.pressure = 0.12                                                       # afterwards: at once, (pressure, mass, gammaP, kT, seed)
    assert eng.calls[-1] == ("barostat_langevin", (0.12, 50.0, 1.0, 1.25, 4711), {})
    b.mass = 500.0
    assert eng.calls[-1] == ("barostat_langevin", (0.12, 500.0, 1.0, 1.25, 4711), {})
    b.gammaP = 0.5
    assert eng.calls[-1] == ("barostat_langevin", (0.12, 500.0, 0.5, 1.25, 4711), {})
    b.disconnect()
    assert eng.calls[-1][0] == "barostat_langevin" and eng.calls[-1][1][1] == 0.0      # mass = 0: off
    n = len(eng.calls)
    b.pressure = 0.2                                                        # disconnected: kept, not pushed
    assert len(eng.calls) == n and b.pressure == 0.2


def test_none_system_is_refused():
    with pytest.raises(NotImplementedError, match="integrator.LangevinBarostat needs a system and its rng"):
        espp.integrator.LangevinBarostat(None, None, 1.0)
    with pytest.raises(NotImplementedError, match="integrator.LangevinBarostat needs a system and its rng"):
        espp.integrator.LangevinBarostat(shim_system(StubEngine()), None, 1.0)
