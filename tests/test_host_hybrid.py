"""Hybrid pair lists (include/chem_mi355.h, chem_list_set_hybrid), host side: the birth steps of chem_host.hpp through every
path that adds, removes or compacts entries, lambda = min(1, lambda0 + rate (step - birth)), the refusals of set_hybrid, the
entry / slot encoding the device consumes; the espressopp-shaped shim objects on a recording engine; the driver's
--t_hybrid_bond switch; the new C symbols.  Nothing here needs a GPU.  The harness is compiled with g++ from tests/host/,
once more with -fsanitize=address,undefined."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from chemlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EINVAL, ESTATE = -1, -4


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "hybrid_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(tmp_path_factory.mktemp("host"), "hybrid_harness", ["-O1"])


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return build(tmp_path_factory.mktemp("host_san"), "hybrid_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def lam_ref(l0, rate, step, birth):
    return min(1.0, l0 + rate * float(step - birth))


class Model:
    """the lists as plain python: [(a, b, birth)] per list, (lambda0, rate) or None"""

    def __init__(self, nlists):
        self.ent = [[] for _ in range(nlists)]
        self.hyb = [None] * nlists
        self.step = 0

    @staticmethod
    def key(a, b):
        return (min(a, b), max(a, b))

    def add(self, li, a, b):
        if self.key(a, b) in {self.key(x, y) for x, y, _ in self.ent[li]}:
            return False
        self.ent[li].append((a, b, self.step))
        return True

    def remove(self, batch):
        for li, a, b, _ in batch:
            self.ent[li] = [e for e in self.ent[li] if self.key(e[0], e[1]) != self.key(a, b)]

    def lam(self, li, s):
        h = self.hyb[li]
        return [(a, b, birth if h else -1, lam_ref(h[0], h[1], s, birth) if h else 1.0) for a, b, birth in self.ent[li]]


def drive(exe, n, lists, script):
    """lists: arities; script: ('hybrid', li, l0, rate) | ('step', s) | ('bond'|'push', li, a, b) | ('remove', [(li, a, b, unexclude)])
    | ('lam', li, s) | ('slots',) | ('entries',).  Returns what the harness printed, parsed, after comparing every 'lam'
    and 'ins' with the model."""
    m = Model(len(lists))
    lines = ["n %d" % n] + ["list %d" % a for a in lists]
    want = []
    for c in script:
        if c[0] == "hybrid":
            lines.append("hybrid %d %r %r" % c[1:]); m.hyb[c[1]] = (c[2], c[3]); want.append(("hyb", 0))
        elif c[0] == "step":
            lines.append("step %d" % c[1]); m.step = c[1]
        elif c[0] == "bond":
            lines.append("bond %d %d %d" % c[1:]); want.append(("ins", int(m.add(*c[1:]))))
        elif c[0] == "push":
            lines.append("push %d %d %d" % c[1:]); assert m.add(*c[1:])
        elif c[0] == "remove":
            lines.append("remove %d " % len(c[1]) + " ".join("%d %d %d %d" % b for b in c[1])); m.remove(c[1])
        elif c[0] == "lam":
            lines.append("lam %d %d" % c[1:]); want.append(("lam", m.lam(*c[1:])))
        else:
            lines.append(c[0]); want.append((c[0], None))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    it = iter(out.stdout.splitlines())
    got = []
    for line in it:
        w = line.split()
        if w[0] in ("hyb", "ins"):
            got.append((w[0], int(w[1])))
        elif w[0] == "lam":
            rows = [next(it).split() for _ in range(int(w[1]))]
            got.append(("lam", [(int(r[0]), int(r[1]), int(r[2]), float(r[3])) for r in rows]))
        else:
            got.append((w[0], [[float(x) for x in next(it).split()] for _ in range(int(w[1]))]))
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0]
        if w[1] is not None:
            assert g[1] == w[1], (k, g, w)          # lambda exactly: the same double expression on both sides
    return got


SCRIPT = [("hybrid", 0, 0.0, 0.25), ("step", 3), ("bond", 0, 0, 1), ("bond", 0, 2, 3), ("step", 5), ("bond", 0, 4, 5), ("push", 0, 6, 7),
          ("bond", 0, 1, 0),                                      # the reversed duplicate: rejected, no birth step either
          ("step", 6), ("bond", 0, 8, 9), ("bond", 1, 10, 11),   # list 1 is a plain list
          ("lam", 0, 6), ("lam", 1, 6),
          ("remove", [(0, 1, 0, 1), (0, 4, 5, 1), (0, 9, 8, 1)]),  # first, a middle and the last entry
          ("lam", 0, 7),
          ("step", 9), ("bond", 0, 0, 1),                          # bonds again: a new birth step
          ("lam", 0, 9), ("lam", 0, 100)]


def test_birth_steps_follow_the_entries(harness):
    got = drive(harness, 12, [2, 2, 3], SCRIPT)
    lams = [g[1] for g in got if g[0] == "lam"]
    assert [r[3] for r in lams[0]] == [0.75, 0.75, 0.25, 0.25, 0.0]
    assert lams[1] == [(10, 11, -1, 1.0)]
    assert [(r[0], r[1], r[2]) for r in lams[2]] == [(2, 3, 3), (6, 7, 5)]            # the survivors kept theirs
    assert lams[3][-1] == (0, 1, 9, 0.0) and [r[3] for r in lams[3][:2]] == [1.0, 1.0]   # 0.25 * 6 = 1.5 clamps at 1
    assert [r[3] for r in lams[4]] == [1.0, 1.0, 1.0]


def test_the_same_script_under_the_sanitizers(harness_san):
    drive(harness_san, 12, [2, 2, 3], SCRIPT)
    rng = np.random.default_rng(3)
    script, have = [("hybrid", 0, 0.125, 0.03125), ("hybrid", 1, 1.0, 0.0)], []
    for rnd in range(8):
        script.append(("step", 10 * rnd))
        for _ in range(20):
            a, b = (int(x) for x in rng.choice(60, 2, replace=False))
            li = int(rng.integers(0, 2))
            script.append(("bond", li, a, b)); have.append((li, a, b))
        pick = set(rng.permutation(len(have))[:9].tolist())
        script.append(("remove", [have[i] + (1,) for i in sorted(pick)]))
        have = [h for i, h in enumerate(have) if i not in pick]
        script += [("lam", 0, 10 * rnd + 7), ("lam", 1, 10 * rnd + 7), ("entries",), ("slots",)]
    drive(harness_san, 60, [2, 2], script)


def test_rate_zero_keeps_lambda0_and_lambda0_one_is_a_plain_list(harness):
    got = drive(harness, 6, [2, 2, 2], [("hybrid", 0, 0.375, 0.0), ("hybrid", 1, 1.0, 0.5), ("bond", 0, 0, 1), ("bond", 1, 0, 1), ("bond", 2, 0, 1),
                                        ("lam", 0, 0), ("lam", 0, 10 ** 9), ("lam", 1, 0), ("lam", 1, 77), ("lam", 2, 77)])
    lams = [g[1][0][3] for g in got if g[0] == "lam"]
    assert lams == [0.375, 0.375, 1.0, 1.0, 1.0]


def test_set_hybrid_refusals(harness):
    def rc(lines):
        out = subprocess.run([harness], input="\n".join(["n 4", "list 2", "list 3"] + lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        return [int(x) for x in out[1::2]]
    assert rc(["hybrid 1 0.0 0.1"]) == [EINVAL]                                          # arity 3
    assert rc(["hybrid 0 -0.01 0.1", "hybrid 0 1.01 0.1", "hybrid 0 0.5 -1e-9"]) == [EINVAL] * 3
    assert rc(["hybrid 0 nan 0.1", "hybrid 0 0.5 nan", "hybrid 0 0.5 inf", "hybrid 0 inf 0"]) == [EINVAL] * 4
    assert rc(["hybrid 0 0.0 0.0", "hybrid 0 0.0 0.02", "hybrid 0 1.0 0.0"]) == [0, 0, 0]   # again on an empty list: allowed
    out = subprocess.run([harness], input="n 4\nlist 2\nbond 0 0 1\nhybrid 0 0.0 0.1\nlam 0 5\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[:2] == ["ins 1", "hyb %d" % ESTATE] and out[3] == "0 1 -1 1"              # refused: still a plain list


def test_device_encoding_of_birth_steps_and_slots(harness):
    got = drive(harness, 8, [2, 3, 2], [("hybrid", 2, 0.25, 0.125), ("bond", 0, 0, 1), ("step", 0), ("bond", 2, 2, 3), ("step", 41), ("bond", 2, 3, 4),
                                        ("slots",), ("entries",)])
    slots, entries = got[-2][1], got[-1][1]
    # (list, pad of the slot, pad of its key, lambda0, rate); a slot that is not hybrid reads lambda = 1 whatever the step
    assert slots == [[0, 0, 0, 1.0, 0.0], [1, 0, 0, 1.0, 0.0], [2, 1, 1, 0.25, 0.125]]
    by_pair = {}
    for t0, t1, t2, slot, pos in entries:
        by_pair.setdefault((int(t0), int(t1), int(slot)), set()).add((int(t2), int(pos)))
    # the third tag of a hybrid pair is ~birth, always negative (birth 0 -> -1, 41 -> -42); 0 for a plain pair
    assert by_pair == {(0, 1, 0): {(0, 0), (0, 1)}, (2, 3, 2): {(-1, 0), (-1, 1)}, (3, 4, 2): {(-42, 0), (-42, 1)}}


# ---- the shim ------------------------------------------------------------------------------------------------------------------

class StubEngine:
    """records the calls the shim makes; lists are numbered in creation order"""

    def __init__(self):
        self.calls = []
        self.n, self.step = 0, 0
        self.nlists = 0
        self.lam = {}

    def list_create(self, *a):
        self.calls.append(("list_create", a, {}))
        self.nlists += 1
        return self.nlists - 1

    def list_get_lambda(self, h):
        return np.asarray(self.lam.get(h, []), dtype=np.float64)

    def __getattr__(self, name):
        def rec(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return rec


def shim_system(engine):
    from chemlab_amd import espp
    old = espp._factory[0]
    espp.set_engine_factory(lambda: engine)
    try:
        s = espp.System()
    finally:
        espp.set_engine_factory(old)
    s.storage = type("S", (), {"system": s})()
    return s


@pytest.mark.parametrize("cls, pot, kind", [
    ("FixedPairListLambdaHarmonic", lambda e: e.interaction.Harmonic(K=30.0, r0=0.5), "HARMONIC"),
    ("FixedPairListLambdaFENE", lambda e: e.interaction.FENE(K=30.0, r0=0.0, rMax=1.5), "FENE"),
    ("FixedPairListLambdaFENELennardJones", lambda e: e.interaction.FENELennardJones(K=30.0, r0=0.0, rMax=1.5, sigma=1.0, epsilon=1.0), "FENE_LJ"),
    ("FixedPairListLambdaTabulated", lambda e: e.interaction.Tabulated.__new__(e.interaction.Tabulated), "TABULATED")])
def test_shim_lists_reach_set_hybrid(cls, pot, kind):
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    fpl = espp.FixedPairListLambda(system.storage, 0.125)
    fpl.addBonds([(1, 2)])                                         # before the interaction exists: pending
    p = pot(espp)
    if kind == "TABULATED":
        p.r0, p.dr, p.e, p.f, p.itype = 0.0, 0.1, [1.0, 0.0], [0.0, 0.0], 1
    inter = getattr(espp.interaction, cls)(system, fpl, p)
    names = [c[0] for c in eng.calls if c[0] in ("list_create", "list_set_hybrid", "list_add")]
    assert names == ["list_create", "list_set_hybrid", "list_add"]            # hybrid while the list is still empty
    assert [c for c in eng.calls if c[0] == "list_create"][0][1] == (2, kind, False)
    assert [c for c in eng.calls if c[0] == "list_set_hybrid"] == [("list_set_hybrid", (0, 0.125, 0.0), {})]
    assert inter.getFixedPairList() is fpl
    with pytest.raises(TypeError):
        getattr(espp.interaction, cls)(system, espp.FixedPairList(system.storage), p)


def test_shim_register_pair_list_and_resolution():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    integ = espp.integrator.VelocityVerlet(system)
    fpl = espp.FixedPairListLambda(system.storage)                 # init_lambda defaults to 0.0
    ext = espp.integrator.FixedListDynamicResolution(system)
    ext.register_pair_list(fpl, 0.01)                              # before the list is bound: kept, sent with the bind
    assert not [c for c in eng.calls if c[0] == "list_set_hybrid"]
    espp.interaction.FixedPairListLambdaHarmonic(system, fpl, espp.interaction.Harmonic(K=1.0, r0=1.0))
    assert [c[1] for c in eng.calls if c[0] == "list_set_hybrid"] == [(0, 0.0, 0.01)]
    ext.register_pair_list(fpl, 0.02)                              # the driver's order: bound first, rate later
    assert [c[1] for c in eng.calls if c[0] == "list_set_hybrid"][-1] == (0, 0.0, 0.02)
    integ.addExtension(ext)
    assert integ.getNumberOfExtensions() == 1
    with pytest.raises(TypeError):
        ext.register_pair_list(espp.FixedPairList(system.storage), 0.02)
    res = espp.analysis.ResolutionFixedPairList(system, fpl)
    assert res.compute() == 0.0                                    # empty list
    eng.lam[0] = [0.25, 0.5, 1.0, 1.0]
    assert res.compute() == 0.6875
    mon = espp.analysis.SystemMonitor(system, integ, None)
    mon.add_observable("res_fpl_0", res)
    mon.perform_action()
    assert mon.last == (["step", "time", "res_fpl_0"], [0, 0.0, 0.6875])


def test_cpu_checker_refuses_hybrid_lists(make_oracle):
    from chemlab_amd import espp
    o = make_oracle()
    h = o.list_create(2, "HARMONIC")
    with pytest.raises(NotImplementedError, match="hybrid bonds"):
        o.list_set_hybrid(h, 0.0, 0.1)
    with pytest.raises(NotImplementedError, match="hybrid bonds"):
        o.list_get_lambda(h)
    system = type("Sys", (), {"engine": o})()
    fpl = espp.FixedPairListLambda(type("S", (), {"system": system})(), 0.0)
    with pytest.raises(NotImplementedError, match="hybrid bonds"):
        espp.interaction.FixedPairListLambdaHarmonic(system, fpl, espp.interaction.Harmonic(K=1.0, r0=1.0))


# ---- the driver ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def recording_driver(oracle_mod):
    """the CPU checker, which has no hybrid lists, with the two hybrid entry points recorded: enough for the driver's wiring"""
    from chemlab_amd import espp
    calls = []

    class Recorder(oracle_mod.OracleEngine):
        def list_set_hybrid(self, h, lambda0, rate):
            calls.append((h, lambda0, rate))

        def list_get_lambda(self, h):
            return np.ones(len(self.get_list(h)))

    espp.set_engine_factory(lambda: Recorder())
    yield calls
    from chemlab_amd.engine import Engine
    espp.set_engine_factory(lambda: Engine(device=0, precision=32))


@pytest.mark.parametrize("t_hybrid", [50, 0])
def test_driver_t_hybrid_bond(tmp_path, recording_driver, monkeypatch, t_hybrid):
    from chemlab_amd import espp, start_simulation
    d = tmp_path / "chain_growth_catalytic"
    shutil.copytree(os.path.join(GOLD, "chain_growth_catalytic"), str(d))
    monkeypatch.chdir(d)
    res = start_simulation.main(["@params", "--run=1000", "--start_ar=500", "--t_hybrid_bond=%d" % t_hybrid], quiet=True)
    header = open("sim0_energy_12345.csv").readline().strip().split(",")
    fpl = res["chem_fpls"][0][1]
    assert "count_0" in header
    if t_hybrid:
        assert isinstance(fpl, espp.FixedPairListLambda)
        assert recording_driver[-1] == (fpl.handle, 0.0, 0.02) and {c[0] for c in recording_driver} == {fpl.handle}
        assert header[header.index("count_0") + 1] == "res_fpl_0"
        assert any(isinstance(x, espp.integrator.FixedListDynamicResolution) for x in res["integrator"]._ext)
    else:
        assert type(fpl) is espp.FixedPairList and recording_driver == []
        assert not [h for h in header if h.startswith("res_fpl")]
        assert not any(isinstance(x, espp.integrator.FixedListDynamicResolution) for x in res["integrator"]._ext)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_new_symbols():
    names = {"chem_list_set_hybrid", "chem_list_get_lambda"}
    assert names <= set(_capi.header_symbols())
    assert "list_set_hybrid" in _capi.PRODUCT_ONLY and "list_get_lambda" in _capi.PRODUCT_ONLY
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in names:
        assert getattr(lib, name) is not None
    assert _capi.load().abi_version() == 1
