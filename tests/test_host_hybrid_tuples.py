"""Hybrid triple and quadruple lists (include/chem_mi355.h, chem_list_set_hybrid_tuples), host side: the birth steps of
chem_host.hpp through every path that adds, spawns, removes or compacts tuples, lambda = min(1, lambda0 + rate (step - birth)), the
refusals of set_hybrid_tuples, the entry encoding the device consumes, the birth arrays of a checkpoint; the espressopp-shaped
shim objects on a recording engine; the driver's --t_hybrid_angle / --t_hybrid_dihedral switches; the new C symbol.  Nothing here
needs a GPU.  The harness is compiled with g++ from tests/host/, once more with -fsanitize=address,undefined as a stand-alone
program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hybrid_tuples_ref as T
from chemlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EINVAL, ESTATE = -1, -4


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "hybrid_tuples_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "hybrid_tuples_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "hybrid_tuples_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, lines):
    """what the harness printed: [(word, value or rows)] -- 'lam', 'excl', 'entries' carry rows of numbers"""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    it = iter(out.stdout.splitlines())
    got = []
    for line in it:
        w = line.split()
        if w[0] in ("hyb", "hybt", "ins"):
            got.append((w[0], int(w[1])))
        elif w[0] == "hex":
            got.append((w[0], bytes.fromhex(w[1])))
        elif w[0] == "ckpt":
            got.append((w[0], (int(w[1]), int(w[2]), " ".join(w[3:]))))
        else:
            got.append((w[0], [[float(x) for x in next(it).split()] for _ in range(int(w[1]))]))
    return got


def lam_ref(l0, rate, step, birth):
    return min(1.0, l0 + rate * float(step - birth))


def canon(t):
    t = tuple(int(x) for x in t)
    return min(t, t[::-1])


class Model:
    """the topology in plain python, tags 0-based: per list [(tags, birth)], the bond set, hybrid = (lambda0, rate) or None.
    What a batch of bonds spawns is hybrid_tuples_ref.spawned (ids = tags + 1)."""

    def __init__(self, n, types, arities, reg, hybrid):
        self.n, self.types, self.arities, self.reg, self.hybrid = n, np.asarray(types), arities, reg, hybrid
        self.ent = [[] for _ in arities]
        self.bonds = []
        self.step = 0

    def where(self, t):
        """the first list of that arity with a registered type tuple that matches (forwards or backwards)"""
        tt = tuple(int(self.types[x]) for x in t)
        for li, ar in enumerate(self.arities):
            if ar == len(t) and any(tuple(k) in (tt, tt[::-1]) for k in self.reg.get(li, [])):
                return li
        return None

    def add(self, li, t):
        if canon(t) in {canon(e[0]) for e in self.ent[li]}:
            return False
        self.ent[li].append((tuple(t), self.step))
        return True

    def bond_batch(self, li, pairs):
        new = [p for p in pairs if self.add(li, p)]
        reg3 = [k for l, ks in self.reg.items() if self.arities[l] == 3 for k in ks]
        reg4 = [k for l, ks in self.reg.items() if self.arities[l] == 4 for k in ks]
        t3, _, t4, _ = T.spawned(np.asarray(self.bonds, np.int64).reshape(-1, 2) + 1, [(self.step, a + 1, b + 1) for a, b in new], self.types, reg3, reg4)
        self.bonds += new
        for t in (t3 - 1).tolist() + (t4 - 1).tolist():
            li_t = self.where(t)
            tt = tuple(int(self.types[x]) for x in t)
            fwd = any(tuple(k) == tt for k in self.reg[li_t])       # (spawned() has oriented it: forwards matches)
            assert fwd or any(tuple(k) == tt[::-1] for k in self.reg[li_t])
            self.add(li_t, t)

    def remove(self, batch):
        gone = {canon((a, b)) for _, a, b, _ in batch}
        for li, a, b, _ in batch:
            self.ent[li] = [e for e in self.ent[li] if canon(e[0]) != canon((a, b))]
        self.bonds = [p for p in self.bonds if canon(p) not in gone]
        for li, ar in enumerate(self.arities):
            if ar > 2:
                self.ent[li] = [e for e in self.ent[li] if not any(canon(e[0][k:k + 2]) in gone for k in range(ar - 1))]

    def lam(self, li, s):
        h = self.hybrid.get(li)
        return [list(t) + [birth if h else -1, lam_ref(h[0], h[1], s, birth) if h else 1.0] for t, birth in self.ent[li]]

    def entries(self):
        """the per-tag CSR: a pair or a plain triple is one entry (t0, t1, t2 | 0 | ~birth of a hybrid pair, slot, member), a plain
        quadruple two, the second (t3, 0, 0, 0, 0) -- the encoding of every list that is not hybrid, unchanged -- and a hybrid
        triple or quadruple two as well, the second (t3 | 0, 0, ~birth, 0, 0).  Rows in list order, entries in list order."""
        rows = [[] for _ in range(self.n)]
        for li, ar in enumerate(self.arities):
            h = self.hybrid.get(li)
            for t, birth in self.ent[li]:
                for k in range(ar):
                    rows[t[k]].append([t[0], t[1], t[2] if ar > 2 else (~birth if h else 0), li, k])
                    if ar > 2 and h:
                        rows[t[k]].append([t[3] if ar == 4 else 0, 0, ~birth, 0, 0])
                    elif ar == 4:
                        rows[t[k]].append([t[3], 0, 0, 0, 0])
        return [[o] + e for o in range(self.n) for e in rows[o]]


# chains 0-1-2-3 | 4-5-6-7 (| = the gap a reaction closes), 8-9 | 10-11, 12 .. 19 loose; all of type 0 but 3, 4 (type 1)
TYPES = [0, 0, 0, 1, 1, 0, 0, 0] + [0] * 12
ARITIES = [2, 3, 3, 4, 4, 2]                  # bonds, plain triples, HYBRID triples, plain quadruples, HYBRID quadruples, reaction bonds
REG = {2: [(0, 0, 1), (0, 1, 1), (0, 0, 0)], 4: [(0, 0, 1, 1), (0, 1, 1, 0), (0, 0, 0, 0)]}
HYB = {2: (0.0, 0.125), 4: (0.25, 0.0625)}


def setup_lines():
    lines = ["n 20"] + ["type %d %d" % (i, t) for i, t in enumerate(TYPES) if t] + ["list %d" % a for a in ARITIES]
    for li, keys in REG.items():
        lines += ["reg %d %s" % (li, " ".join(str(x) for x in k)) for k in keys]
    lines += ["hybt %d %r %r" % (li, l0, r) for li, (l0, r) in HYB.items()]
    return lines


def drive(exe, script):
    """script: ('step', s) | ('add', li, tags) | ('bonds', li, [(a, b)...]) | ('remove', [(li, a, b, unexclude)]) | ('lam', li, s) |
    ('entries',).  Every answer of the harness is compared with the model; returns (model, answers)."""
    m = Model(20, TYPES, ARITIES, REG, HYB)
    lines, want = setup_lines(), [("hybt", 0)] * len(HYB)
    for c in script:
        if c[0] == "step":
            lines.append("step %d" % c[1]); m.step = c[1]
        elif c[0] == "add":
            lines.append("add %d %s" % (c[1], " ".join(str(x) for x in c[2]))); want.append(("ins", int(m.add(c[1], c[2]))))
        elif c[0] == "bonds":
            lines.append("bonds %d %d %s" % (c[1], len(c[2]), " ".join("%d %d" % p for p in c[2]))); m.bond_batch(c[1], c[2])
        elif c[0] == "remove":
            lines.append("remove %d " % len(c[1]) + " ".join("%d %d %d %d" % b for b in c[1])); m.remove(c[1])
        elif c[0] == "lam":
            lines.append("lam %d %d" % c[1:]); want.append(("lam", m.lam(*c[1:])))
        elif c[0] == "entries":
            lines.append("entries"); want.append(("entries", m.entries()))
    got = run(exe, lines)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1], (k, g, w)      # lambda exactly: the same double expression on both sides
    return m, got


PRE = [("bonds", 0, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7), (8, 9), (10, 11)]),          # step 0: the chains (their own tuples are spawned: birth 0) ...
       ("add", 1, (0, 1, 2)), ("add", 3, (0, 1, 2, 3)), ("add", 1, (2, 1, 0))]                    # ... plain tuples by list_add; the reversed duplicate is refused
SCRIPT = PRE + [
    ("step", 3), ("bonds", 5, [(3, 4)]),                        # one bond: triples (2 3 4), (3 4 5), quadruples (1 2 3 4), (2 3 4 5), (3 4 5 6)
    ("add", 2, (12, 13, 14)), ("add", 4, (12, 13, 14, 15)),     # list_add on a hybrid list: born at step 3 too
    ("lam", 2, 3), ("lam", 4, 3), ("lam", 2, 7), ("lam", 1, 7), ("entries",),
    ("step", 8), ("bonds", 5, [(9, 16), (16, 10)]),             # two adjacent bonds of ONE step: one angle (9 16 10), spawned once
    ("lam", 2, 9), ("lam", 4, 9),
    ("remove", [(5, 3, 4, 1)]),                                 # takes every tuple across 3-4 and its birth; the rest is compacted
    ("lam", 2, 9), ("lam", 4, 9), ("entries",),
    ("step", 20), ("bonds", 5, [(4, 3)]),                       # bonds again: the tuples start at lambda0
    ("lam", 2, 20), ("lam", 4, 20), ("lam", 2, 1000), ("lam", 4, 1000), ("entries",)]


def test_birth_steps_follow_the_tuples(harness):
    m, got = drive(harness, SCRIPT)                              # (every answer already equals the model's)
    lams = [g[1] for g in got if g[0] == "lam"]
    tri = lambda rows: {canon(r[:3]): (int(r[3]), r[4]) for r in rows}
    quad = lambda rows: {canon(r[:4]): (int(r[4]), r[5]) for r in rows}
    old3 = {(0, 1, 2): 0, (1, 2, 3): 0, (4, 5, 6): 0, (5, 6, 7): 0}      # the chains' own bonds, all of step 0: their tuples were spawned then
    old4 = {}                                                            # ((0 1 2 3) reads 0 0 0 1: not registered)
    new = lambda d, old: {k: v for k, v in d.items() if k not in old}
    assert {k: v[0] for k, v in tri(lams[0]).items() if k in old3} == old3 and {k: v[0] for k, v in quad(lams[1]).items() if k in old4} == old4
    assert new(tri(lams[0]), old3) == {(2, 3, 4): (3, 0.0), (3, 4, 5): (3, 0.0), (12, 13, 14): (3, 0.0)}
    assert new(quad(lams[1]), old4) == {(1, 2, 3, 4): (3, 0.25), (2, 3, 4, 5): (3, 0.25), (3, 4, 5, 6): (3, 0.25), (12, 13, 14, 15): (3, 0.25)}
    assert {v for v in new(tri(lams[2]), old3).values()} == {(3, 0.5)} and lams[3] == [[0, 1, 2, -1, 1.0]]       # the plain list keeps no births
    # two adjacent bonds of one step: (8 9 16), (9 16 10), (16 10 11), each once, born at step 8
    assert {k: v for k, v in tri(lams[4]).items() if 16 in k} == {(8, 9, 16): (8, 0.125), (9, 16, 10): (8, 0.125), (11, 10, 16): (8, 0.125)}
    assert {k: v for k, v in quad(lams[5]).items() if 16 in k} == {(8, 9, 16, 10): (8, 0.3125), (9, 16, 10, 11): (8, 0.3125)}
    # the removal of 3 - 4: every tuple across it is gone with its birth, the survivors keep theirs through the compaction
    assert new(tri(lams[6]), old3) == {(12, 13, 14): (3, 0.75), (8, 9, 16): (8, 0.125), (9, 16, 10): (8, 0.125), (11, 10, 16): (8, 0.125)}
    assert new(quad(lams[7]), old4) == {(12, 13, 14, 15): (3, 0.625), (8, 9, 16, 10): (8, 0.3125), (9, 16, 10, 11): (8, 0.3125)}
    assert {k: v[0] for k, v in tri(lams[6]).items() if k in old3} == old3
    # bonded again at step 20: spawned again, at lambda0
    again3, again4 = tri(lams[8]), quad(lams[9])
    assert again3[(2, 3, 4)] == (20, 0.0) and again3[(3, 4, 5)] == (20, 0.0) and again3[(12, 13, 14)] == (3, 1.0)
    assert again4[(1, 2, 3, 4)] == (20, 0.25) and again4[(12, 13, 14, 15)] == (3, 1.0) and again4[(8, 9, 16, 10)] == (8, 1.0)
    assert {r[4] for r in lams[10]} == {1.0} and {r[5] for r in lams[11]} == {1.0}                    # clamps at exactly 1


def test_entry_encoding(harness):
    m, got = drive(harness, PRE + [("step", 41), ("bonds", 5, [(3, 4)]), ("entries",)])
    ent = got[-1][1]
    # the row of tag 2, in list order: bonds (1 2), (2 3) | plain triple (0 1 2) | hybrid triples (0 1 2), (1 2 3) of step 0 and (2 3 4) of
    # step 41 | plain quadruple (0 1 2 3) | hybrid quadruples (1 2 3 4), (2 3 4 5): widths 1 1 | 1 | 2 2 2 | 2 | 2 2 interleaved
    row = [[int(x) for x in e[1:]] for e in ent if e[0] == 2]
    assert [e[3] for e in row] == [0, 0, 1, 2, 0, 2, 0, 2, 0, 3, 0, 4, 0, 4, 0]
    assert row[2] == [0, 1, 2, 1, 2]                                          # a plain triple: one entry, its third tag in t2
    assert row[3] == [0, 1, 2, 2, 2] and row[4] == [0, 0, ~0, 0, 0]           # a hybrid triple: a second entry with ~birth in t2 (birth 0 -> -1),
    assert row[7] == [2, 3, 4, 2, 0] and row[8] == [0, 0, ~41, 0, 0]          # always negative, where a hybrid pair keeps its own
    assert row[9] == [0, 1, 2, 3, 2] and row[10] == [3, 0, 0, 0, 0]           # a plain quadruple's second entry: (t3, 0, 0, 0), as ever
    assert row[11] == [1, 2, 3, 4, 1] and row[12] == [4, 0, ~41, 0, 0]        # a hybrid quadruple's: (t3, 0, ~birth, 0)
    assert ~0 == -1 and ~41 == -42
    # a topology without a hybrid list: the model's rule for plain lists is the encoding as it was before hybrid tuples existed
    plain = Model(20, TYPES, ARITIES, REG, {})
    lines = [l for l in setup_lines() if not l.startswith("hybt")] + ["bonds 0 3 0 1 1 2 2 3", "add 1 0 1 2", "add 3 0 1 2 3", "step 5", "bonds 5 1 3 4", "entries"]
    plain.bond_batch(0, [(0, 1), (1, 2), (2, 3)]); plain.add(1, (0, 1, 2)); plain.add(3, (0, 1, 2, 3)); plain.step = 5; plain.bond_batch(5, [(3, 4)])
    out = run(harness, lines)
    assert out[-1] == ("entries", plain.entries()) and all(e[3] >= 0 for e in out[-1][1])
    # three triples spawned into list 2 and one quadruple into list 4, plain this time: widths 1 and 2
    assert sum(1 for e in out[-1][1] if e[4] == 2) == 3 * 3 and sum(1 for e in out[-1][1] if e[4] == 4) == 4 and sum(1 for e in out[-1][1] if e[1:] == [4, 0, 0, 0, 0]) == 4


def test_refusals(harness):
    def rc(lines):
        return [v for _, v in run(harness, ["n 4", "list 2", "list 3", "list 4"] + lines)]
    assert rc(["hybt 0 0.0 0.1"]) == [EINVAL]                                          # arity 2: chem_list_set_hybrid's
    assert rc(["hybrid 1 0.0 0.1", "hybrid 2 0.0 0.1"]) == [EINVAL, EINVAL]            # and set_hybrid still refuses arity 3 and 4
    assert rc(["hybt 1 -0.01 0.1", "hybt 1 1.01 0.1", "hybt 2 0.5 -1e-9"]) == [EINVAL] * 3
    assert rc(["hybt 1 nan 0.1", "hybt 2 0.5 nan", "hybt 1 0.5 inf", "hybt 2 inf 0"]) == [EINVAL] * 4
    assert rc(["hybt 1 0.0 0.0", "hybt 1 0.0 0.02", "hybt 2 1.0 0.0"]) == [0, 0, 0]   # again on an empty list: allowed
    out = run(harness, ["n 4", "list 3", "add 0 0 1 2", "hybt 0 0.0 0.1", "lam 0 5"])
    assert out == [("ins", 1), ("hybt", ESTATE), ("lam", [[0, 1, 2, -1, 1.0]])]        # refused: still a plain list


def test_checkpoint_carries_the_birth_steps(harness):
    pre = setup_lines() + ["bonds 0 6 0 1 1 2 2 3 4 5 5 6 6 7", "step 3", "bonds 5 1 3 4", "step 9", "add 2 12 13 14", "add 4 12 13 14 15", "step 11"]
    out = run(harness, pre + ["ckpt ok 0", "ckpt short 2", "ckpt short 4", "ckpt late 2", "ckpt late 4", "ckpt early 4"])
    res = [v for k, v in out if k == "ckpt"]
    assert res[0] == (0, 1, "")
    for r in res[1:3]:
        assert r[0] == EINVAL and "birth steps do not match the entries" in r[2]
    for r in res[3:]:
        assert r[0] == EINVAL and "birth step outside [0, step]" in r[2]
    # a triple list that is NOT hybrid and carries birth steps all the same is refused (none are expected), a hybrid one passes
    out = run(harness, ["n 6", "list 3", "list 3", "hybt 1 0 0.5", "add 0 0 1 2", "add 1 3 4 5", "ckpt ok 0", "ckpt stray 0"])
    assert out[-2][1] == (0, 1, "") and out[-1][1][0] == EINVAL and "birth steps do not match the entries" in out[-1][1][2]


def test_checkpoint_bytes_of_a_context_without_hybrid_tuples(harness):
    """The lists section, taken apart by the layout chem_ckpt_host.hpp documents (u64 list count; per list u64 count + int32 tags,
    u64 count + int64 birth steps): a context whose triple and quadruple lists are plain writes empty birth arrays for them, as
    before -- only the hybrid pair list has births -- and with hybrid tuple lists the same section grows by their births alone."""
    import struct
    from test_host_checkpoint import walk

    def lists_section(hybrid_tuples):
        lines = ["n 8", "list 2", "list 3", "list 4", "hybrid 0 0.25 0.5"] + (["hybt 1 0 0.5", "hybt 2 0 0.5"] if hybrid_tuples else [])
        lines += ["step 2", "bonds 0 2 0 1 1 2", "step 6", "add 1 0 1 2", "add 1 4 5 6", "add 2 0 1 2 3", "step 9", "ckpt hex 0"]
        blob = [v for k, v in run(harness, lines) if k == "hex"][0]
        sec = [s for s in walk(blob) if s[0] == "lists"][0]
        return blob[sec[2]:sec[2] + sec[3]]

    def packed(births):
        ents = [[0, 1, 1, 2], [0, 1, 2, 4, 5, 6], [0, 1, 2, 3]]
        out = struct.pack("<Q", 3)
        for e, b in zip(ents, births):
            out += struct.pack("<Q%di" % len(e), len(e), *e) + struct.pack("<Q%dq" % len(b), len(b), *b)
        return out
    assert lists_section(False) == packed([[2, 2], [], []])
    assert lists_section(True) == packed([[2, 2], [6, 6], [6]])


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


def _tab(e, cls):
    p = cls.__new__(cls)
    p.r0, p.dr, p.e, p.f, p.itype = 0.0, 0.1, [1.0, 0.0], [0.0, 0.0], 1
    return p


SHIM = [
    ("FixedTripleList", "AngularHarmonic", lambda e: e.interaction.AngularHarmonic(K=5.0, theta0=2.0), "ANG_HARMONIC"),
    ("FixedTripleList", "Cosine", lambda e: e.interaction.Cosine(K=5.0, theta0=2.0), "ANG_COSINE"),
    ("FixedTripleList", "TabulatedAngular", lambda e: _tab(e, e.interaction.TabulatedAngular), "ANG_TABULATED"),
    ("FixedQuadrupleList", "DihedralHarmonicNCos", lambda e: e.interaction.DihedralHarmonicNCos(K=2.0, phi0=0.3, multiplicity=3), "DIH_NCOS"),
    ("FixedQuadrupleList", "DihedralRB", lambda e: e.interaction.DihedralRB(0.5, -0.3, 0.2, 0.1, -0.1, 0.05), "DIH_RB"),
    ("FixedQuadrupleList", "DihedralHarmonic", lambda e: e.interaction.DihedralHarmonic(K=2.0, phi0=0.3), "DIH_HARMONIC"),
    ("FixedQuadrupleList", "TabulatedDihedral", lambda e: _tab(e, e.interaction.TabulatedDihedral), "DIH_TABULATED"),
]


@pytest.mark.parametrize("typed", [False, True], ids=["plain", "types"])
@pytest.mark.parametrize("base, pot_name, pot, kind", SHIM, ids=[s[1] for s in SHIM])
def test_shim_lists_reach_set_hybrid_tuples(base, pot_name, pot, kind, typed):
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    arity = 3 if base == "FixedTripleList" else 4
    lst = getattr(espp, base + "Lambda")(system.storage, 0.125)
    entry = tuple(range(1, arity + 1))
    (lst.addTriples if arity == 3 else lst.addQuadruples)([entry])       # before the interaction exists: pending
    assert lst.getAllLambda() == [0.125]
    cls = getattr(espp.interaction, "%s%sLambda%s" % (base, "Types" if typed else "", pot_name))
    p = pot(espp)
    if typed:
        inter = cls(system, lst)
        inter.setPotential(*(tuple(range(arity)) + (p,)))
    else:
        inter = cls(system, lst, p)
    names = [c[0] for c in eng.calls if c[0] in ("list_create", "list_set_hybrid_tuples", "list_set_hybrid", "list_add")]
    assert names == ["list_create", "list_set_hybrid_tuples", "list_add"]      # hybrid while the list is still empty
    assert [c for c in eng.calls if c[0] == "list_create"][0][1] == (arity, kind, typed)
    assert [c for c in eng.calls if c[0] == "list_set_hybrid_tuples"] == [("list_set_hybrid_tuples", (0, 0.125, 0.0), {})]
    assert (inter.getFixedTripleList() if arity == 3 else inter.getFixedQuadrupleList()) is lst
    plain = getattr(espp, base)(system.storage)
    with pytest.raises(TypeError):
        cls(system, plain) if typed else cls(system, plain, p)
    with pytest.raises(TypeError):                                         # nor the Lambda list of the other arity
        other = espp.FixedQuadrupleListLambda(system.storage) if arity == 3 else espp.FixedTripleListLambda(system.storage)
        cls(system, other) if typed else cls(system, other, p)


def test_shim_register_lists_and_resolution():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    integ = espp.integrator.VelocityVerlet(system)
    ftl, fql = espp.FixedTripleListLambda(system.storage), espp.FixedQuadrupleListLambda(system.storage, 0.5)      # init_lambda defaults to 0.0
    ext = espp.integrator.FixedListDynamicResolution(system)
    ext.register_triple_list(ftl, 0.01)                             # before the list is bound: kept, sent with the bind
    assert not [c for c in eng.calls if c[0] == "list_set_hybrid_tuples"]
    espp.interaction.FixedTripleListLambdaCosine(system, ftl, espp.interaction.Cosine(K=1.0, theta0=2.0))
    espp.interaction.FixedQuadrupleListTypesLambdaDihedralRB(system, fql).setPotential(0, 0, 0, 0, espp.interaction.DihedralRB(1, 0, 0, 0, 0, 0))
    assert [c[1] for c in eng.calls if c[0] == "list_set_hybrid_tuples"] == [(0, 0.0, 0.01), (1, 0.5, 0.0)]
    ext.register_quadruple_list(fql, 0.125)                        # the driver's order: bound first, rate later
    assert [c[1] for c in eng.calls if c[0] == "list_set_hybrid_tuples"][-1] == (1, 0.5, 0.125)
    integ.addExtension(ext)
    assert ext.triple_lists == [(ftl, 0.01)] and ext.quadruple_lists == [(fql, 0.125)] and ext.pair_lists == []
    for bad in (espp.FixedTripleList(system.storage), fql, espp.FixedPairListLambda(system.storage)):
        with pytest.raises(TypeError):
            ext.register_triple_list(bad, 0.02)
    for bad in (espp.FixedQuadrupleList(system.storage), ftl):
        with pytest.raises(TypeError):
            ext.register_quadruple_list(bad, 0.02)
    with pytest.raises(TypeError):
        ext.register_pair_list(ftl, 0.02)
    r3, r4 = espp.analysis.ResolutionFixedTripleList(system, ftl), espp.analysis.ResolutionFixedQuadrupleList(system, fql)
    assert r3.compute() == 0.0 and r4.compute() == 0.0               # empty lists
    eng.lam[0], eng.lam[1] = [0.25, 0.5, 1.0, 1.0], [0.5, 1.0]
    assert r3.compute() == 0.6875 and r4.compute() == 0.75 and fql.getAllLambda() == [0.5, 1.0]
    mon = espp.analysis.SystemMonitor(system, integ, None)
    mon.add_observable("res_ftl_0", r3)
    mon.add_observable("res_fql_0", r4)
    mon.perform_action()
    assert mon.last == (["step", "time", "res_ftl_0", "res_fql_0"], [0, 0.0, 0.6875, 0.75])


def test_cpu_checker_refuses_hybrid_tuple_lists(make_oracle):
    from chemlab_amd import espp
    o = make_oracle()
    h = o.list_create(3, "ANG_HARMONIC")
    with pytest.raises(NotImplementedError, match="hybrid angles and dihedrals: the CPU checker has no FixedTripleListLambda / FixedQuadrupleListLambda"):
        o.list_set_hybrid_tuples(h, 0.0, 0.1)
    system = type("Sys", (), {"engine": o})()
    ftl = espp.FixedTripleListLambda(type("S", (), {"system": system})(), 0.0)
    with pytest.raises(NotImplementedError, match="hybrid angles and dihedrals"):
        espp.interaction.FixedTripleListLambdaAngularHarmonic(system, ftl, espp.interaction.AngularHarmonic(K=1.0, theta0=2.0))


# ---- the driver ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def recording_driver(oracle_mod):
    """the CPU checker, which has no hybrid lists, with the hybrid entry points recorded: enough for the driver's wiring"""
    from chemlab_amd import espp
    calls, registered = [], []

    class Recorder(oracle_mod.OracleEngine):
        def list_set_hybrid(self, h, lambda0, rate):
            calls.append(("pairs", h, lambda0, rate))

        def list_set_hybrid_tuples(self, h, lambda0, rate):
            calls.append(("tuples", h, lambda0, rate))

        def list_get_lambda(self, h):
            return np.ones(len(self.get_list(h)))

        def topology_register(self, h, types):
            registered.append((h, tuple(int(t) for t in types)))
            return oracle_mod.OracleEngine.topology_register(self, h, types)

    espp.set_engine_factory(lambda: Recorder())
    yield calls, registered
    from chemlab_amd.engine import Engine
    espp.set_engine_factory(lambda: Engine(device=0, precision=32))


def stage(tmp_path):
    d = tmp_path / "chain_growth_catalytic"
    shutil.copytree(os.path.join(GOLD, "chain_growth_catalytic"), str(d))
    top = open(str(d / "topol.top")).read()
    types = open(os.path.join(GOLD, "hybrid_tuples", "bonded_types.top")).read()
    assert top.count("[ nonbond_params ]") == 1
    open(str(d / "topol.top"), "w").write(top.replace("[ nonbond_params ]", types + "[ nonbond_params ]"))
    return d


@pytest.mark.parametrize("t_angle, t_dihedral", [(0, 0), (50, 0), (0, 25), (50, 25)])
def test_driver_t_hybrid_angle_and_dihedral(tmp_path, recording_driver, monkeypatch, t_angle, t_dihedral):
    from chemlab_amd import espp, start_simulation
    calls, registered = recording_driver
    monkeypatch.chdir(stage(tmp_path))
    res = start_simulation.main(["@params", "--run=1000", "--start_ar=500", "--t_hybrid_angle=%d" % t_angle, "--t_hybrid_dihedral=%d" % t_dihedral], quiet=True)
    header = open("sim0_energy_12345.csv").readline().strip().split(",")
    echo = open("sim0params.out").read()
    assert "t_hybrid_angle=%d" % t_angle in echo.replace(" ", "") and "t_hybrid_dihedral=%d" % t_dihedral in echo.replace(" ", "")      # the params echo
    angles, dihedrals = res["angles"], res["dihedrals"]
    assert "angle_dynamic" in angles and "dihedral_dynamic" in dihedrals
    names = [res["system"].getNameOfInteraction(k) for k in range(res["system"].getNumberOfInteractions())]
    exts = [x for x in res["integrator"]._ext if isinstance(x, espp.integrator.FixedListDynamicResolution)]
    for on, lists, kind, col, list_cls, t in ((t_angle > 0, angles, "angle", "res_ftl_0", espp.FixedTripleListLambda, t_angle),
                                                (t_dihedral > 0, dihedrals, "dihedral", "res_fql_0", espp.FixedQuadrupleListLambda, t_dihedral)):
        dyn = lists[kind + "_dynamic"]
        assert not isinstance(dyn[0], list_cls)                        # the topology's own tuples: a plain list, full strength
        reg = [r for r in registered if len(r[1]) == (3 if kind == "angle" else 4)]
        assert reg and {r[1] for r in reg} == {tuple(k) for k in dyn[1]._typed}
        if on:
            hyb, inter = lists[kind + "_hybrid"]
            assert isinstance(hyb, list_cls)
            assert sorted(inter._typed) == sorted(dyn[1]._typed) and inter._typed is not dyn[1]._typed      # the same registered potentials
            assert {r[0] for r in reg} == {hyb.handle}                 # the topology manager spawns into the hybrid list
            assert [c for c in calls if c[0] == "tuples" and c[1] == hyb.handle][-1] == ("tuples", hyb.handle, 0.0, 1.0 / t)
            assert kind + "_hybrid" in names and kind + "_hybrid" in header and col in header
            assert any(l is hyb for x in exts for l, _ in (x.triple_lists if kind == "angle" else x.quadruple_lists))
        else:
            assert kind + "_hybrid" not in lists and kind + "_hybrid" not in names and kind + "_hybrid" not in header and col not in header
            assert {r[0] for r in reg} == {dyn[0].handle}
    if not (t_angle or t_dihedral):
        assert calls == [] and exts == []
        assert not [h for h in header if h.startswith("res_")]
    assert not [c for c in calls if c[0] == "pairs"]                  # --t_hybrid_bond stays off


def test_driver_refuses_a_switch_that_has_nothing_to_ramp(tmp_path, recording_driver, monkeypatch):
    """the fixture as it is has no angletypes and no dihedraltypes, hence no dynamic lists: a switch is not dropped silently"""
    from chemlab_amd import start_simulation
    d = tmp_path / "chain_growth_catalytic"
    shutil.copytree(os.path.join(GOLD, "chain_growth_catalytic"), str(d))
    monkeypatch.chdir(d)
    for switch, kind in (("--t_hybrid_angle=8", "angle"), ("--t_hybrid_dihedral=8", "dihedral")):
        with pytest.raises(RuntimeError, match="%s 8: the topology has no %s_dynamic list" % (switch.split("=")[0], kind)):
            start_simulation.main(["@params", "--run=1000", "--start_ar=500", switch], quiet=True)
    assert recording_driver[0] == []


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_new_symbol():
    assert "chem_list_set_hybrid_tuples" in set(_capi.header_symbols())
    assert "list_set_hybrid_tuples" in _capi.PRODUCT_ONLY
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert lib.chem_list_set_hybrid_tuples is not None
    assert _capi.load().abi_version() == 1
