"""Fixed distances / by-product release (include/chem_mi355.h, chem_fix_create ff.), host side: the pure routines of
chemlab_amd/csrc/chem_fix_host.hpp -- add with validation, release by reaction and by type, compaction, the log, the device
order -- against the plain-Python restatement of tests/fixdist_ref.py on seeded random cases; the numpy constraint against
its own definition; the bindings and the CPU checker's refusals.  Nothing here needs a GPU.  The harness is compiled with g++
from tests/host/, once more with -fsanitize=address,undefined as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import fixdist_ref as FX
from chemlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "fix_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "fix_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "fix_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    return [x for x in out.stdout.split("\n") if x]


def parse(out):
    """the harness's answers as a list of (head, payload): records and entries become tuples"""
    res, k = [], 0
    while k < len(out):
        w = out[k].split()
        if w[0] in ("rel", "log", "get"):
            n = int(w[1])
            rows = [out[k + 1 + j].split() for j in range(n)]
            if w[0] == "get":
                res.append(("get", [(int(r[0]), int(r[1]), float(r[2]), int(r[3])) for r in rows]))
            else:
                res.append((w[0], [tuple(int(v) for v in r) for r in rows]))
            k += 1 + n
        else:
            res.append((w[0], w[1:])); k += 1
    return res


class Script:
    """the same operations sent to the harness and applied to the model"""

    def __init__(self, n):
        self.m = FX.Sets(n)
        self.lines, self.want = ["ntags %d" % n], []
        self.types = [0] * n

    def create(self, at=-1, tt=-1):
        h = self.m.create(at, tt)
        self.lines.append("create %d %d" % (at, tt)); self.want.append(("set", [str(ENOSPC if h is None else h)]))
        return h

    def add(self, h, pairs, dist):
        ok = self.m.add(h, pairs, dist)
        self.lines.append("add %d %r %d %s" % (h, dist, len(pairs), " ".join("%d %d" % p for p in pairs)))
        self.want.append(("add", [str(0 if ok else EINVAL)]))
        return ok

    def rule(self, reaction, role, h, count):
        self.m.rules.append((reaction, role, h, count)); self.lines.append("rule %d %d %d %d" % (reaction, role, h, count))

    def set_types(self, types):
        self.types = list(types); self.lines.append("types " + " ".join(str(t) for t in types))

    def settype(self, i, t):
        self.types[i] = t; self.lines.append("settype %d %d" % (i, t))

    def react(self, step, reactants):
        self.lines.append("react %d %d %s" % (step, len(reactants), " ".join("%d %d %d" % r for r in reactants)))
        self.want.append(("rel", self.m.release_by_reaction(reactants, step)))
        return self.want[-1][1]

    def bytype(self, step):
        self.lines.append("bytype %d" % step); self.want.append(("rel", self.m.release_by_type(self.types, step)))
        return self.want[-1][1]

    def get(self, h):
        self.lines.append("get %d" % h); self.want.append(("get", self.m.entries(h)))

    def log(self):
        self.lines.append("log"); self.want.append(("log", self.m.records()))

    def count(self):
        ent = [e for s in self.m.sets for e in s["ent"]]
        self.lines.append("count"); self.want.append(("count", [str(len(ent)), str(len({e[1] for e in ent})), str(len({e[0] for e in ent}))]))

    def check(self, exe):
        got = parse(drive(exe, self.lines))
        assert got == self.want
        return got


def test_validation_refusals(harness):
    s = Script(20)
    h = s.create(); g = s.create(0, 1)
    assert s.add(h, [(0, 10), (0, 11), (1, 12)], 0.5)             # an anchor may carry any number of entries
    assert not s.add(h, [(2, 10)], 0.5)                            # a second live entry for one target
    assert not s.add(g, [(2, 11)], 0.5)                            # ... over all sets
    assert not s.add(h, [(10, 13)], 0.5)                           # an anchor that is a target
    assert not s.add(h, [(3, 0)], 0.5)                             # a target that is an anchor
    assert not s.add(h, [(3, 3)], 0.5)                             # anchor == target
    assert not s.add(h, [(3, -1)], 0.5) and not s.add(h, [(20, 4)], 0.5)      # unknown ids
    assert not s.add(h, [(3, 13)], 0.0) and not s.add(h, [(3, 13)], -1.0)
    assert not s.add(h, [(3, 13)], float("inf")) and not s.add(h, [(3, 13)], float("nan"))
    assert not s.add(7, [(3, 13)], 0.5)                            # unknown set
    assert not s.add(h, [(3, 13), (4, 13)], 0.5)                   # the same target twice in one call
    assert not s.add(h, [(3, 13), (13, 14)], 0.5)                  # a target of the call used as an anchor of the call
    assert not s.add(h, [(3, 13), (5, 3)], 0.5)                    # an anchor of the call used as a target of the call
    s.get(h); s.count()                                            # nothing of the refused calls was added
    assert s.add(g, [(3, 13)], 0.25)
    s.get(g); s.count()
    for _ in range(FX.MAX_SETS - 2):
        assert s.create() is not None
    assert s.create() is None                                      # CHEM_ENOSPC beyond the constant
    s.check(harness)


def test_release_by_reaction_order_count_and_roles(harness):
    s = Script(40)
    h = s.create(); g = s.create()
    s.add(h, [(0, 20), (1, 21), (0, 22), (1, 23), (0, 24), (2, 25)], 0.4)
    s.add(g, [(0, 30), (3, 31), (3, 32)], 0.3)
    s.rule(0, 1, h, 1)          # reaction 0: role 1 loses one entry of h
    s.rule(0, 2, h, 2)          # ... role 2 two
    s.rule(1, 1, g, 5)          # reaction 1: role 1 loses up to five of g (fewer are there)
    s.rule(0, 1, g, 1)          # a second rule on (0, 1), another set
    # event (0, 1): role 1 = particle 0 loses its lowest entry of h (target 20) and its entry of g; role 2 = particle 1 both of h
    r = s.react(5, [(0, 1, 0), (0, 2, 1)])
    assert sorted(x[3] for x in r) == [20, 21, 23, 30]
    s.get(h); s.get(g)
    # the next event on particle 0 takes the next lowest (22); a reactant without entries releases nothing; a reaction without a rule nothing
    r = s.react(6, [(0, 1, 0), (0, 1, 5), (2, 1, 0), (0, 2, 7)])
    assert [x[3] for x in r] == [22]
    # fewer left than asked: role 2 wants two, particle 0 has one left
    r = s.react(7, [(0, 2, 0)])
    assert [x[3] for x in r] == [24]
    r = s.react(7, [(1, 1, 3), (1, 2, 3)])
    assert [x[3] for x in r] == [31, 32]
    assert s.react(8, [(0, 2, 0), (1, 1, 3)]) == []
    s.get(h); s.get(g); s.count(); s.log()
    s.check(harness)
    # two events of one step on the same anchor, role order: the first event's role-1 release comes first
    t = Script(12)
    k = t.create()
    t.add(k, [(0, 5), (0, 6), (0, 7), (1, 8)], 1.0)
    t.rule(0, 1, k, 1); t.rule(0, 2, k, 1)
    r = t.react(3, [(0, 1, 1), (0, 2, 0), (0, 1, 0), (0, 2, 4)])
    assert [x[3] for x in r] == [5, 6, 8]                          # (reported in log order: insertion index)
    t.get(k); t.log()
    t.check(harness)


def test_release_by_type(harness):
    s = Script(30)
    a = s.create(0, 1); b = s.create(-1, 2); c = s.create()
    s.set_types([0] * 10 + [1] * 10 + [2] * 10)
    s.add(a, [(0, 10), (0, 11), (1, 12)], 0.4)
    s.add(b, [(2, 20), (3, 21)], 0.4)
    s.add(c, [(4, 22), (4, 13)], 0.4)
    assert s.bytype(0) == []
    s.settype(0, 3)                                               # the anchor's type: both of its entries in a leave, nothing else
    assert [x[3] for x in s.bytype(4)] == [10, 11]
    s.settype(12, 2)                                              # a target's type
    s.settype(2, 5)                                               # an anchor of a set without an anchor condition: stays
    s.settype(21, 0)
    s.settype(4, 9); s.settype(22, 9)                             # the set without types never releases by type
    r = s.bytype(9)
    assert [(x[1], x[3], x[4]) for x in r] == [(a, 12, FX.CAUSE_TYPE), (b, 21, FX.CAUSE_TYPE)]
    s.get(a); s.get(b); s.get(c); s.log(); s.count()
    assert s.add(a, [(0, 10)], 0.4)                               # a released target may be fixed again
    s.get(a)
    s.check(harness)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_scripts_against_the_model(harness, seed):
    """adds (valid and invalid), both kinds of release, reads of every set and of the log, interleaved at random"""
    rng = np.random.default_rng(seed)
    n = 60
    s = Script(n)
    nset = 4
    conds = [(-1, -1), (0, 1), (-1, 1), (0, -1)]
    for k in range(nset):
        s.create(*conds[k])
    types = [0] * 30 + [1] * 30
    s.set_types(types)
    for reaction in range(3):
        for role in (1, 2):
            if rng.random() < 0.8:
                s.rule(reaction, role, int(rng.integers(0, nset)), int(rng.integers(1, 4)))
    released = accepted = refused = 0
    for step in range(1, 60):
        op = rng.random()
        if op < 0.45:
            k = int(rng.integers(1, 5))
            pairs = [(int(rng.integers(0, 30)), int(rng.integers(25, n))) for _ in range(k)]
            ok = s.add(int(rng.integers(0, nset)), pairs, float(rng.uniform(0.1, 1.0)))
            accepted += ok; refused += not ok
        elif op < 0.75:
            reactants = []
            for _ in range(int(rng.integers(1, 4))):
                r, pa, pb = int(rng.integers(0, 3)), int(rng.integers(0, 30)), int(rng.integers(0, 30))
                reactants += [(r, 1, pa), (r, 2, pb)]
            released += len(s.react(step, reactants))
        else:
            s.settype(int(rng.integers(0, n)), int(rng.integers(0, 3)))
            released += len(s.bytype(step))
        if step % 7 == 0:
            for h in range(nset):
                s.get(h)
            s.log(); s.count()
    for h in range(nset):
        s.get(h)
    s.log(); s.count()
    s.check(harness)
    assert released > 5 and accepted > 5 and refused > 2
    rec = s.m.records()
    keys = [(r[0], r[1]) for r in rec]
    assert keys == sorted(keys)                                    # the log: by step, then set (then insertion index: the model's sort)
    for h in range(nset):                                          # compaction kept the insertion order
        seq = [e[3] for e in s.m.entries(h)]
        assert seq == sorted(seq)


def test_device_order_keeps_the_entries_of_an_anchor_together(harness):
    lines = ["ntags 30", "create -1 -1", "create -1 -1", "add 0 0.5 4 3 10 1 11 3 12 2 13", "add 1 0.5 3 1 14 3 15 0 16", "order"]
    out = drive(harness, lines)
    assert out[-1] == "order 0:16 1:11 1:14 2:13 3:10 3:12 3:15"


def test_the_numpy_constraint():
    rng = np.random.default_rng(5)
    box = np.array([5.4, 6.0, 7.5])
    xa = rng.uniform(-10, 20, (200, 3))
    d = rng.uniform(0.1, 1.0, 200)
    xt = xa + rng.normal(0, 0.6, (200, 3)) + box * rng.integers(-2, 3, (200, 3))
    xt[0] = xa[0]                                                  # |u| = 0
    new = FX.constrain(xa, xt, d, box)
    r = FX.min_image(new - xa, box)
    assert np.abs(np.sqrt((r * r).sum(-1)) - d).max() < 1e-13
    assert np.allclose(r[0], [d[0], 0, 0], atol=1e-13)
    old = FX.min_image(xt - xa, box)
    cosang = (r[1:] * old[1:]).sum(-1) / d[1:] / np.sqrt((old[1:] ** 2).sum(-1))
    assert np.abs(cosang - 1).max() < 1e-12                        # the direction is kept
    assert np.abs(np.rint((new - xt) / box)).max() == 0            # ... and the periodic image
    # one model step: the target ends on the sphere, with the anchor's half-step velocity
    x = rng.uniform(0, 5, (6, 3)); v = rng.normal(0, 1, (6, 3)); f = rng.normal(0, 1, (6, 3)); m = rng.uniform(0.5, 2, 6)
    xn, vh = FX.step_model(x, v, f, m, 0.01, [(0, 3, 0.4), (0, 4, 0.5), (1, 5, 0.3)], box)
    assert np.allclose(FX.distances(xn, [(0, 3, 0.4), (0, 4, 0.5), (1, 5, 0.3)], box), [0.4, 0.5, 0.3], atol=1e-14)
    assert np.array_equal(vh[3], vh[0]) and np.array_equal(vh[4], vh[0]) and np.array_equal(vh[5], vh[1])
    assert np.array_equal(xn[:3], x[:3] + 0.01 * (v[:3] + 0.005 * f[:3] / m[:3, None]))


def test_bindings_and_struct_size():
    import ctypes as C
    assert C.sizeof(_capi.FixRecord) == 32
    names = {"add_particles", "fix_create", "fix_add", "fix_postprocess", "reaction_release", "fix_count", "fix_get", "fix_log"}
    assert names <= set(_capi.PRODUCT_ONLY)
    assert {"chem_" + n for n in names} <= set(_capi.header_symbols())
    lib = C.CDLL(_capi.LIB_PATH)
    assert all(hasattr(lib, "chem_" + n) for n in names)


def test_the_cpu_checker_refuses(make_oracle):
    o = make_oracle()
    for call in (lambda: o.fix_create(), lambda: o.fix_add(0, [(1, 2)], 0.5), lambda: o.fix_postprocess(0, 1), lambda: o.reaction_release(0, 1, 0),
                 lambda: o.fix_count(0), lambda: o.fix_get(0), lambda: o.fix_log(), lambda: o.add_particles([9], [0], [[0, 0, 0]], 1.0)):
        with pytest.raises(NotImplementedError):
            call()
