"""CPU-side checks of the pressure / barostat entry points (include/chem_mi355.h chem_get_pressure, chem_barostat_berendsen,
chem_get_box): the symbols are exported and bound, the ABI version stays 1, the result struct has the C compiler's layout,
and the CPU checker's refusals name the feature."""
import ctypes as C
import os
import subprocess

import pytest

from chemlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("get_pressure", "barostat_berendsen", "get_box")


def test_symbols_are_exported_and_bound():
    hdr = set(_capi.header_symbols())
    lib = C.CDLL(_capi.LIB_PATH)
    api = _capi.load()
    for n in NAMES:
        assert "chem_" + n in hdr
        assert hasattr(lib, "chem_" + n)
        assert n in api.exported()
        assert n in _capi.PRODUCT_ONLY and n not in _capi.SIGNATURES          # the CPU oracle has none of them
    assert api.get_pressure.argtypes == [C.c_void_p, C.POINTER(_capi.Pressure)]
    assert api.barostat_berendsen.argtypes == [C.c_void_p, C.c_double, C.c_double]
    assert api.abi_version() == 1


def test_result_layout_matches_the_header(tmp_path):
    assert C.sizeof(_capi.Pressure) == 8 * (5 + _capi.CHEM_MAX_LISTS)
    fields = [n for n, _ in _capi.Pressure._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(chem_pressure));\n' +
                   "".join('  printf("%%zu\\n", offsetof(chem_pressure, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_capi.Pressure)
    assert out[1:] == [getattr(_capi.Pressure, f).offset for f in fields]


def test_cpu_checker_refusals_name_the_feature(make_oracle):
    o = make_oracle()
    with pytest.raises(NotImplementedError, match="Pressure: the CPU checker has no virial of the bonded lists"):
        o.pressure()
    with pytest.raises(NotImplementedError, match="BerendsenBarostat: the CPU checker has no barostat"):
        o.barostat_berendsen(1.0, 1.0)
    with pytest.raises(NotImplementedError, match="box: the CPU checker has no read-back of the box"):
        o.box()
