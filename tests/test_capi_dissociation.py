"""CPU-side checks of the dissociation entry point (include/chem_mi355.h chem_dissociation_add): the symbol is exported
and bound, the descriptor's layout is the C compiler's, and dissociation_draw (include/chem_philox.h) has the counter
layout of reaction_draw under its own key."""
import ctypes as C
import os
import subprocess

from chemlab_amd import _capi
from test_philox import philox_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound():
    assert "chem_dissociation_add" in _capi.header_symbols()
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "chem_dissociation_add")
    api = _capi.load()
    assert "dissociation_add" in api.exported()
    assert api.dissociation_add.argtypes == [C.c_void_p, C.POINTER(_capi.DissociationDesc)]
    assert "dissociation_add" not in _capi.SIGNATURES          # the CPU oracle has no bond removal: product only
    assert api.abi_version() == 1


def test_descriptor_layout_matches_the_header(tmp_path):
    assert C.sizeof(_capi.DissociationDesc) == 104             # LP64: 8 x int32, 2 x double, 6 x int32, 4 x double
    fields = [n for n, _ in _capi.DissociationDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(chem_dissociation_desc));\n' +
                   "".join('  printf("%%zu\\n", offsetof(chem_dissociation_desc, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(_capi.DissociationDesc)
    assert out[1:] == [getattr(_capi.DissociationDesc, f).offset for f in fields]


def test_dissociation_draw_matches_the_python_restatement(tmp_path):
    cases = [(0, 1, 0, 1, 0), (0x1234567887654321, 7, 11, 4000, 3), (2 ** 64 - 1, 2 ** 33 + 5, 123456, 123457, 15)]
    src = tmp_path / "draw.cpp"
    src.write_text('#include <cstdio>\n#include "chem_philox.h"\nint main() {\n  uint32_t o[4];\n' +
                   "".join("  chem_philox::dissociation_draw(%dull, %dull, %du, %du, %du, o); printf(\"%%u %%u %%u %%u\\n\", o[0], o[1], o[2], o[3]);\n" % c
                           for c in cases) + "  return 0;\n}\n")
    exe = str(tmp_path / "draw")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for (seed, step, lo, hi, r), line in zip(cases, out):
        want = philox_py((lo, hi, step & 0xffffffff, ((r << 24) ^ (step >> 32)) & 0xffffffff), ((seed & 0xffffffff) ^ 0x44495353, seed >> 32))
        assert tuple(int(x) for x in line.split()) == want
