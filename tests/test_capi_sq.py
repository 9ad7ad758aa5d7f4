"""chem_sq_* at the boundary, on the CPU: the symbols and their binding, the struct as the C compiler lays it out, the CPU
checker's refusal, and the shim class and the text writer against a stub engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from chemlab_amd import _capi
from chemlab_amd import engine as E
from chemlab_amd import espp
from chemlab_amd.chemlab import outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sq_init", "sq_sample", "sq_sample_every", "sq_get", "sq_reset")


def test_symbols_are_declared_exported_and_bound():
    lib = C.CDLL(_capi.LIB_PATH)
    for n in NAMES:
        assert "chem_" + n in _capi.header_symbols() and hasattr(lib, "chem_" + n) and n in _capi.PRODUCT_ONLY
    assert set(NAMES) <= set(_capi.load().exported())
    assert (_capi.CHEM_SQ_MAX_N, _capi.CHEM_SQ_MAX_PAIRS) == (16, 4)


def test_struct_layout_is_the_c_compilers(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chem_mi355.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(chem_sq_result), offsetof(chem_sq_result, npairs), offsetof(chem_sq_result, nvec), offsetof(chem_sq_result, frames), '
                   'offsetof(chem_sq_result, na), offsetof(chem_sq_result, nb), offsetof(chem_sq_result, box_sum), sizeof(((chem_sq_result*)0)->na), '
                   'CHEM_SQ_MAX_N, CHEM_SQ_MAX_PAIRS); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = _capi.SqResult
    assert got == [C.sizeof(R), R.npairs.offset, R.nvec.offset, R.frames.offset, R.na.offset, R.nb.offset, R.box_sum.offset, R.na.size,
                   _capi.CHEM_SQ_MAX_N, _capi.CHEM_SQ_MAX_PAIRS]
    assert C.sizeof(R) == 8 + 16 + 8 * (4 + 4 + 3) == 112


def test_the_cpu_checker_refuses(make_oracle):
    o = make_oracle()
    assert not o.supports("sq")
    for call in (lambda: o.sq_init(4), o.sq_sample, lambda: o.sq_sample_every(1), o.sq_reset, o.sq):
        with pytest.raises(NotImplementedError) as ei:
            call()
        assert str(ei.value) == "sq: the CPU checker has no structure factor"


class StubEngine:
    """What the shim and the writer need of an Engine: the sq_* methods, recording their calls; sq() answers from sums it makes
    up through engine.sq_result, the function Engine.sq() itself ends in."""

    def __init__(self, has=True):
        self.calls, self.has, self.conf = [], has, None

    def supports(self, name):
        return self.has and name == "sq"

    def sq_init(self, nmax, type_pairs=((-1, -1),)):
        self.calls.append(("init", nmax, list(type_pairs)))
        self.conf = (nmax, len(type_pairs))

    def sq_sample(self):
        self.calls.append(("sample",))

    def sq_sample_every(self, every):
        self.calls.append(("every", every))

    def sq(self):
        nmax, nsel = self.conf
        nvec = E.sq_nvec(nmax)
        sums = (np.arange(nsel * nvec, dtype=np.float64) + 1.0).reshape(nsel, nvec)
        return E.sq_result(nmax, sums, 3, np.full(nsel, 300.0), np.full(nsel, 75.0), [15.0, 18.0, 30.0])


class StubSystem:
    def __init__(self, eng):
        self.engine = eng


def test_shim_class():
    eng = StubEngine()
    obs = espp.analysis.StaticStructF(StubSystem(eng))
    s = obs.compute(2)
    assert eng.calls == [("init", 2, [(-1, -1)]), ("sample",)] and len(s) == len(eng.sq()["shell_q"]) > 2 and all(isinstance(v, float) for v in s)
    eng.calls.clear()
    obs.start(3, types=[(0, 1), (1, 1)], every=10)
    assert eng.calls == [("init", 3, [(0, 1), (1, 1)]), ("every", 10)]
    r = obs.result()
    assert r["S"].shape == (2, 171) and r["n"].shape == (171, 3) and np.allclose(r["S"], r["sums"] / 150.0, rtol=1e-15)
    with pytest.raises(NotImplementedError) as ei:
        espp.analysis.StaticStructF(StubSystem(StubEngine(has=False))).compute(4)
    assert str(ei.value) == "sq: the CPU checker has no structure factor"


def test_writer_columns(tmp_path):
    eng = StubEngine()
    eng.sq_init(2, [(0, 0), (0, 1)])
    want = eng.sq()
    path = tmp_path / "out" / "sq.dat"
    outputs.write_sq(str(path), want, labels=["AA", "AB"])
    lines = path.read_text().split("\n")
    nshell = len(want["shell_q"])
    assert lines[-1] == "" and len(lines) == nshell + 2
    assert lines[0].startswith("# q count S_AA S_AB") and "frames 3" in lines[0] and "nmax 2" in lines[0]
    rows = np.array([[float(v) for v in l.split()] for l in lines[1:-1]])
    assert rows.shape == (nshell, 4) and rows[:, 1].sum() == want["nvec"] == 62
    assert np.allclose(rows[:, 0], want["shell_q"], atol=1e-6) and np.allclose(rows[:, 2:], want["shell_S"].T, rtol=1e-8)
    assert (np.diff(rows[:, 0]) > 0).all()                                          # shells in increasing |q|
    # the shells are those of the mean box (5, 6, 10): width 2 pi / 10, a vector in the shell nearest to |q| / width
    q = 2 * np.pi * np.sqrt(((want["n"] / np.array([5.0, 6.0, 10.0])) ** 2).sum(axis=1))
    sh = np.floor(q / (2 * np.pi / 10.0) + 0.5).astype(int)
    assert np.array_equal(rows[:, 1].astype(int), [int((sh == i).sum()) for i in np.unique(sh)])
    outputs.write_sq(str(path), E.sq_result(1, np.ones((1, 13)), 1, [1.0], [1.0], [4.0, 4.0, 4.0]))
    assert path.read_text().split("\n")[0].startswith("# q count S_sel0 ")
