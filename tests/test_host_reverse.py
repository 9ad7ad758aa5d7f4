"""Reverse reactions (include/chem_mi355.h, chem_reaction_remove_bond / chem_reaction_join), host side: the selection routines
of chemlab_amd/csrc/chem_react_host.hpp (select_removals, removals_by_list, with HostTopology::remove_bonds behind them) and
chem_fix_host.hpp (FixState::join_by_reaction) against the plain-Python restatement of tests/reverse_ref.py: breadth-first
levels 1 - 3 on chains, rings and stars, snapshot types against current types, a bond reachable from two events, a pair
held by two lists, join refusals, insertion order, seeded random scripts; the bindings and the CPU checker's refusals.
Nothing here needs a GPU.  The harness is compiled with g++ from tests/host/, once more with -fsanitize=address,undefined
as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import fixdist_ref as FX
import reverse_ref as RV
from chemlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, E, W = 0, 1, 2, 3


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include")] + flags +
                          [os.path.join(ROOT, "tests", "host", "reverse_harness.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if request.param == "plain":
        return build(tmp_path_factory.mktemp("host"), "reverse_harness", ["-O1"])
    return build(tmp_path_factory.mktemp("host_san"), "reverse_harness_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


class Script:
    """the same operations sent to the harness and applied to the model; the answers are compared line by line"""

    def __init__(self, n, types):
        self.n = n
        self.types = list(types)
        self.type0 = list(types)
        self.graph = [set() for _ in range(n)]
        self.lists, self.excl, self.mol = [], set(), list(range(n))
        self.rx, self.rules, self.jrules = [], [], []
        self.sets = FX.Sets(n)
        self.jlog = []
        self.lines = ["n %d" % n] + ["type %d %d" % (k, t) for k, t in enumerate(types)] + ["snap"]
        self.want = []

    def new_list(self):
        self.lists.append([]); self.lines.append("list")
        return len(self.lists) - 1

    def bond(self, li, a, b):
        ins = not any({a, b} == set(e) for e in self.lists[li])
        if ins:
            self.lists[li].append((a, b))
        self.graph[a].add(b); self.graph[b].add(a); self.excl.add((min(a, b), max(a, b)))
        comp = sorted(RV.levels(self.graph, a, self.n))
        for x in comp:
            self.mol[x] = comp[0]
        self.lines.append("bond %d %d %d" % (li, a, b)); self.want.append("ins %d" % ins)

    def retype(self, tag, t, snap=False):
        self.types[tag] = t; self.lines.append("type %d %d" % (tag, t))
        if snap:
            self.type0 = list(self.types); self.lines.append("snap")

    def reaction(self, t1, t2):
        self.rx.append((t1, t2)); self.lines.append("rx %d %d" % (t1, t2))
        return len(self.rx) - 1

    def rule(self, reaction, invoke_on, anchor_type, nb_level, t1, t2, unexclude):
        self.rules.append(dict(reaction=reaction, invoke_on=invoke_on, anchor_type=anchor_type, nb_level=nb_level, type_1=t1, type_2=t2, unexclude=unexclude))
        self.lines.append("rule %d %d %d %d %d %d %d" % (reaction, invoke_on, anchor_type, nb_level, t1, t2, unexclude))

    def create(self, at=-1, tt=-1):
        h = self.sets.create(at, tt)
        self.lines.append("create %d %d" % (at, tt)); self.want.append("set %d" % h)
        return h

    def add(self, h, a, t, d):
        ok = self.sets.add(h, [(a, t)], d)
        self.lines.append("add %d %r %d %d" % (h, d, a, t)); self.want.append("add %d" % (0 if ok else -1))

    def jrule(self, reaction, role, h, d):
        self.jrules.append((reaction, role, h, d)); self.lines.append("jrule %d %d %d %r" % (reaction, role, h, d))

    def events(self, step, evs):
        """evs: (a, b, reaction); put into canonical order here"""
        evs = sorted(evs, key=lambda e: (min(e[:2]), max(e[:2])))
        rem = RV.select_removals(self.graph, self.type0, self.rx, self.rules, evs)
        unex = {(min(p, q), max(p, q)): u for p, q, r, u in rem}
        recs = RV.apply_removals(self.graph, self.lists, self.excl, self.mol, rem)
        log, added = RV.apply_joins(self.sets, self.jrules, evs, step)
        self.jlog += log
        self.lines.append("events %d %d %s" % (step, len(evs), " ".join("%d %d %d" % e for e in evs)))
        self.want.append("rem %d" % len(recs))
        self.want += ["%d %d %d %d %d" % (p, q, li, r, unex[(min(p, q), max(p, q))]) for p, q, li, r in recs]
        self.want.append("join %d" % len(added))
        seqs = {(e[0], e[1]): e[3] for s in self.sets.sets for e in s["ent"]}
        self.want += ["%d %d %.17g %d" % (a, t, d, seqs[(a, t)]) for a, t, d in added]
        return recs, added

    def dump(self):
        self.lines.append("dump")
        for li, l in enumerate(self.lists):
            self.want.append("list %d %d" % (li, len(l)))
            self.want += ["%d %d" % e for e in l]
        self.want.append("graph")
        self.want += [("%d: " % i + " ".join(str(x) for x in sorted(self.graph[i]))).rstrip() if self.graph[i] else "%d:" % i for i in range(self.n)]
        self.want.append("excl %d" % len(self.excl))
        rows = [sorted([b for a, b in self.excl if a == i] + [a for a, b in self.excl if b == i]) for i in range(self.n)]
        self.want += [("%d: " % i + " ".join(str(x) for x in r)) if r else "%d:" % i for i, r in enumerate(rows)]
        self.want.append("mol")
        self.want += [str(m) for m in self.mol]
        for si, s in enumerate(self.sets.sets):
            self.want.append("fixset %d %d" % (si, len(s["ent"])))
            self.want += ["%d %d %.17g %d" % tuple(e) for e in s["ent"]]
        self.want.append("jlog %d" % len(self.jlog))
        self.want += ["%d %d %d %d %d" % r for r in self.jlog]
        self.want.append("end")

    def check(self, exe):
        out = subprocess.run([exe], input="\n".join(self.lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr + out.stdout
        got = [x.rstrip() for x in out.stdout.split("\n") if x]
        assert got == self.want


def shape(kind, m):
    if kind == "chain":
        return [(k, k + 1) for k in range(m - 1)]
    if kind == "ring":
        return [(k, (k + 1) % m) for k in range(m)]
    return [(0, k) for k in range(1, m)]


@pytest.mark.parametrize("kind", ["chain", "ring", "star"])
@pytest.mark.parametrize("level", [1, 2, 3])
def test_levels(harness, kind, level):
    """alternating C / E on 7 particles + one W; an event on every second C, rules on both roles"""
    m = 7
    s = Script(m + 3, [C if k % 2 == 0 else E for k in range(m)] + [W, W, W])
    li = s.new_list()
    for a, b in shape(kind, m):
        s.bond(li, a, b)
    r = s.reaction(C, W)
    s.rule(r, 3, C, level, C, E, 1)
    recs, _ = s.events(4, [(0, m, r), (4, m + 1, r)])
    assert len(recs) >= 1 or (kind, level) == ("star", 3)              # (a star has nothing three bonds away)
    s.dump()
    s.check(harness)


def test_snapshot_types(harness):
    """E -> A in the same step still matches C:E; a C that was an A at the snapshot does not"""
    s = Script(6, [C, E, A, E, W, W])
    li = s.new_list()
    s.bond(li, 0, 1); s.bond(li, 2, 3)
    r = s.reaction(C, W)
    s.rule(r, 1, C, 1, C, E, 1)
    s.retype(1, A)                  # what the step's own events and neighbour rules did: not in the snapshot
    s.retype(2, C)
    recs, _ = s.events(1, [(0, 4, r), (2, 5, r)])
    assert [x[:2] for x in recs] == [(0, 1)]
    s.dump()
    s.check(harness)


def test_bond_of_two_events_and_pair_in_two_lists(harness):
    s = Script(6, [C, C, E, W, W, W])
    l0, l1 = s.new_list(), s.new_list()
    s.bond(l0, 0, 1); s.bond(l1, 1, 0); s.bond(l0, 1, 2); s.bond(l1, 2, 1)
    r0, r1 = s.reaction(C, W), s.reaction(C, W)
    s.rule(r0, 1, C, 1, C, C, 0)
    s.rule(r1, 1, C, 1, C, C, 1)
    s.rule(r1, 1, C, 1, C, E, 1)
    recs, _ = s.events(2, [(1, 4, r1), (0, 3, r0)])
    assert recs == [(0, 1, 0, 0), (0, 1, 1, 0), (1, 2, 0, 1), (1, 2, 1, 1)]          # (0, 1): once, for the first visit (reaction 0)
    assert (0, 1) in s.excl and (1, 2) not in s.excl
    s.dump()
    s.check(harness)


def test_join_refusals_and_order(harness):
    s = Script(8, [C, C, C, W, W, W, W, A])
    s.new_list()
    h0, h1 = s.create(), s.create(C, W)
    s.add(h0, 7, 6, 0.5)
    r = s.reaction(C, W)
    s.jrule(r, 1, h1, 0.25)
    s.jrule(r, 2, h0, 0.75)         # the reverse direction: refused wherever the first rule was accepted
    recs, added = s.events(3, [(0, 3, r), (1, 6, r), (2, 7, r)])      # 6 is a target already, 7 an anchor
    assert added == [(0, 3, 0.25), (7, 2, 0.75)]                      # (7 may anchor 2 as well; 2 may not anchor 7)
    assert [x[4] for x in s.jlog] == [3, 4, 4, 4, 4, 3]
    _, added = s.events(6, [(1, 4, r), (0, 5, r)])
    assert added == [(0, 5, 0.25), (1, 4, 0.25)]                      # canonical order; an anchor may carry two entries
    assert [e[3] for e in s.sets.entries(h1)] == [0, 1, 2]
    s.dump()
    s.check(harness)


@pytest.mark.parametrize("seed", range(8))
def test_random_scripts(harness, seed):
    rng = np.random.default_rng(seed)
    n = 40
    s = Script(n, rng.integers(0, 4, n).tolist())
    lists = [s.new_list(), s.new_list()]
    for _ in range(45):
        a, b = rng.choice(n, 2, replace=False)
        s.bond(lists[int(rng.integers(0, 2))], int(a), int(b))
    rxs = [s.reaction(int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(3)]
    for _ in range(6):
        s.rule(int(rng.choice(rxs)), int(rng.integers(1, 4)), int(rng.integers(0, 4)), int(rng.integers(1, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 2)))
    hs = [s.create(), s.create()]
    for _ in range(4):
        s.jrule(int(rng.choice(rxs)), int(rng.integers(1, 3)), int(rng.choice(hs)), float(rng.integers(1, 9)) / 8)
    nrem = 0
    for step in range(1, 5):
        for k in rng.choice(n, 5, replace=False):
            s.retype(int(k), int(rng.integers(0, 4)))
        s.lines.append("snap"); s.type0 = list(s.types)
        for k in rng.choice(n, 3, replace=False):                       # the step's own type changes, behind the snapshot
            s.retype(int(k), int(rng.integers(0, 4)))
        part = rng.permutation(n)[:12].reshape(6, 2)                     # a particle takes part in one event per step
        recs, _ = s.events(step, [(int(a), int(b), int(rng.choice(rxs))) for a, b in part])
        nrem += len(recs)
        s.dump()
    assert nrem > 0 and len(s.jlog) > 0
    s.check(harness)


def test_bindings_and_checker_refusals():
    assert _capi.NbRemove._fields_[0][0] == "reaction" and len(_capi.NbRemove._fields_) == 8
    import ctypes as Ct
    assert Ct.sizeof(_capi.NbRemove) == 32 and Ct.sizeof(_capi.BondRecord) == 32
    for name in ("reaction_remove_bond", "reaction_removed", "reaction_join", "fix_joins"):
        assert name in _capi.PRODUCT_ONLY and "chem_" + name in _capi.header_symbols()
    from oracle.oracle import OracleEngine
    o = OracleEngine()
    with pytest.raises(NotImplementedError, match="RemoveNeighboursBonds"):
        o.reaction_remove_bond(0, "type_1", 1, 1, 1, 2)
    with pytest.raises(NotImplementedError, match="JoinMolecule"):
        o.reaction_join(0, "type_1", 0, 0.5)
