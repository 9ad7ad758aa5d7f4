"""CPU-side checks of the checkpoint entry points (include/chem_mi355.h chem_checkpoint_save, chem_checkpoint_load): the symbols
are exported and bound with the header's signatures, the ABI version stays 1, the CPU checker refuses by name, and
Engine.checkpoint_save / checkpoint_load move the bytes they are given (an api stub that records calls): the size query first,
a file written under a temporary name and renamed, a load from bytes or from a path."""
import ctypes as C
import os

import pytest

from chemlab_amd import _capi
from chemlab_amd.engine import ChemError, Engine

NAMES = ("checkpoint_save", "checkpoint_load")


def test_symbols_exported_and_bound():
    api = _capi.load()
    for name in NAMES:
        assert hasattr(api.lib, "chem_" + name), name
        assert name in api.exported() and name not in _capi.SIGNATURES          # the CPU oracle has no checkpoint: product only
    assert api.checkpoint_save.argtypes == [C.c_void_p, C.c_void_p, C.c_int64] and api.checkpoint_save.restype == C.c_int64
    assert api.checkpoint_load.argtypes == [C.c_void_p, C.c_void_p, C.c_int64] and api.checkpoint_load.restype == C.c_int
    assert api.abi_version() == 1
    assert {"chem_" + n for n in NAMES} <= set(_capi.header_symbols())


def test_cpu_checker_refuses_by_name(oracle_mod):
    o = oracle_mod.OracleEngine()
    assert not o.supports("checkpoint")
    with pytest.raises(NotImplementedError, match=r"^checkpoint: the CPU checker has no checkpoint$"):
        o.checkpoint_save()
    with pytest.raises(NotImplementedError, match=r"^checkpoint: the CPU checker has no checkpoint$"):
        o.checkpoint_load(b"")
    o.close()


class StubApi:
    """checkpoint_save hands out `blob`, checkpoint_load keeps what it was given; both record their arguments"""

    def __init__(self, blob):
        self.blob, self.calls, self.loaded = blob, [], None

    def destroy(self, ctx):
        pass

    def last_error(self, ctx):
        return b"stub refusal"

    def checkpoint_save(self, ctx, buf, cap):
        self.calls.append(("save", buf is None, cap))
        if buf is None:
            return len(self.blob)
        if cap < len(self.blob):
            return _capi.ENOSPC
        C.memmove(buf, self.blob, len(self.blob))
        return len(self.blob)

    def checkpoint_load(self, ctx, buf, n):
        self.calls.append(("load", n))
        self.loaded = C.string_at(buf, n)
        return _capi.EINVAL if self.loaded.startswith(b"bad") else 0


def test_engine_moves_the_bytes(tmp_path):
    blob = bytes(range(256)) * 3 + b"\0tail\0"
    api = StubApi(blob)
    e = Engine(api=api, ctx=1)
    assert e.supports("checkpoint") and e.supports("checkpoint_load") and not e.supports("get_box")
    assert e.checkpoint_save() == blob
    assert api.calls == [("save", True, 0), ("save", False, len(blob))]             # the size first, then one call with room for it
    path = tmp_path / "run.ckpt"
    path.write_bytes(b"the last complete checkpoint")
    assert e.checkpoint_save(path) == len(blob)
    assert path.read_bytes() == blob and os.listdir(tmp_path) == ["run.ckpt"]       # written beside it, renamed over it: nothing else is left
    e.checkpoint_load(blob)
    assert api.loaded == blob and api.calls[-1] == ("load", len(blob))
    e.checkpoint_load(str(path))
    assert api.loaded == blob
    e.checkpoint_load(bytearray(b""))
    assert api.loaded == b"" and api.calls[-1] == ("load", 0)
    with pytest.raises(ChemError, match="stub refusal") as err:
        e.checkpoint_load(b"bad blob")
    assert err.value.code == _capi.EINVAL
    e.ctx = None
