"""CPU-side checks of the pressure-tensor entry point (include/chem_mi355.h chem_get_pressure_tensor): the symbol is exported
and bound, the ABI version stays 1, the result struct has the C compiler's layout while chem_obs and chem_pressure keep
theirs, the CPU checker's refusal names the feature, and the shim's analysis.PressureTensor reaches the engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chemlab_amd import _capi
from chemlab_amd import espp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound():
    hdr = set(_capi.header_symbols())
    lib = C.CDLL(_capi.LIB_PATH)
    api = _capi.load()
    assert "chem_get_pressure_tensor" in hdr
    assert hasattr(lib, "chem_get_pressure_tensor")
    assert "get_pressure_tensor" in api.exported()
    assert "get_pressure_tensor" in _capi.PRODUCT_ONLY and "get_pressure_tensor" not in _capi.SIGNATURES      # the CPU oracle has none
    assert api.get_pressure_tensor.argtypes == [C.c_void_p, C.POINTER(_capi.PressureTensor)]
    assert api.abi_version() == 1


def _layout(tmp_path, ctype, struct, fields):
    src = tmp_path / ("layout_%s.c" % ctype)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) {\n'
                   '  printf("%%zu\\n", sizeof(%s));\n' % ctype +
                   "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (ctype, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / ("layout_" + ctype))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(struct)
    assert out[1:] == [getattr(struct, f).offset for f in fields]


def test_result_layout_matches_the_header(tmp_path):
    nl = _capi.CHEM_MAX_LISTS
    assert C.sizeof(_capi.PressureTensor) == 8 * (1 + 6 * (4 + nl))
    assert [n for n, _ in _capi.PressureTensor._fields_] == ["volume", "kinetic", "virial_nb", "virial_list", "virial", "tensor"]
    _layout(tmp_path, "chem_pressure_tensor", _capi.PressureTensor, [n for n, _ in _capi.PressureTensor._fields_])
    # virial_list is [list][component]
    p = _capi.PressureTensor()
    p.virial_list[2][4] = 7.0
    flat = (C.c_double * (C.sizeof(p) // 8)).from_buffer(p)
    assert flat[1 + 12 + 6 * 2 + 4] == 7.0


def test_the_older_structs_keep_their_layout(tmp_path):
    nl = _capi.CHEM_MAX_LISTS
    assert C.sizeof(_capi.Pressure) == 8 * (5 + nl)
    _layout(tmp_path, "chem_pressure", _capi.Pressure, [n for n, _ in _capi.Pressure._fields_])
    _layout(tmp_path, "chem_obs", _capi.Obs, [n for n, _ in _capi.Obs._fields_])


def test_cpu_checker_refusal_names_the_feature(make_oracle):
    o = make_oracle()
    with pytest.raises(NotImplementedError, match="PressureTensor: the CPU checker has no virial tensor"):
        o.pressure_tensor()


def test_the_shim_class_reaches_the_engine():
    calls = []

    class FakeEngine(object):
        def pressure_tensor(self):
            calls.append("pressure_tensor")
            return dict(volume=2.0, tensor=np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))

    class FakeSystem(object):
        engine = FakeEngine()

    obs = espp.analysis.PressureTensor(FakeSystem())
    out = obs.compute()
    assert calls == ["pressure_tensor"]
    assert out == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0] and all(type(c) is float for c in out)      # xx, yy, zz, xy, xz, yz
