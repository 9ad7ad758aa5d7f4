"""CPU-only test of bond REMOVAL in the host topology manager (chemlab_amd/csrc/chem_host.hpp: HostTopology::remove_bonds,
TupleSet::erase, TagRow::erase -- what a dissociation reaction step calls, include/chem_mi355.h chem_dissociation_add).
After every removal the lists, the bond graph, the exclusion rows (with their pair count and the append-only log the
device table is built from) and mol_id are compared with a brute-force recomputation from the surviving bonds.
The harness is compiled with g++ from tests/host/."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host") / "dissociation_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "dissociation_harness.cpp"), "-o", exe])
    return exe


def key(t):
    return min(tuple(t), tuple(reversed(t)))


class Model:
    """Brute force: the state is the bond lists, the angle list and the exclusion set; graph and labels are recomputed."""

    def __init__(self, n, types, nlists2, reg):
        self.n, self.types, self.reg = n, types, reg
        self.bonds = [[] for _ in range(nlists2)]
        self.angles = []
        self.excl = set()

    def graph(self):
        g = [set() for _ in range(self.n)]
        for l in self.bonds:
            for a, b in l:
                g[a].add(b); g[b].add(a)
        return g

    def add_bond(self, li, a, b):
        if key((a, b)) in {key(x) for x in self.bonds[li]}:
            return False
        self.bonds[li].append((a, b))
        self.excl.add(key((a, b)))
        g = self.graph()
        cands = [(x, a, b) for x in sorted(g[a]) if x != b] + [(a, b, m) for m in sorted(g[b]) if m != a]
        for t in cands:
            ty = tuple(self.types[x] for x in t)
            for r in self.reg:
                fwd, rev = ty == tuple(r), tuple(reversed(ty)) == tuple(r)
                if not (fwd or rev):
                    continue
                tt = t if fwd else tuple(reversed(t))
                if key(tt) not in {key(x) for x in self.angles}:
                    self.angles.append(tt)
                    self.excl.add(key((tt[0], tt[2])))
                break
        return True

    def remove(self, batch):
        for li, a, b, unex in batch:
            self.bonds[li] = [x for x in self.bonds[li] if key(x) != key((a, b))]
            if unex:
                self.excl.discard(key((a, b)))
        g = self.graph()
        cut = {key((a, b)) for _, a, b, _ in batch if b not in g[a]}
        self.angles = [t for t in self.angles if key(t[:2]) not in cut and key(t[1:]) not in cut]

    def mol(self):
        g = self.graph()
        mol = [-1] * self.n
        for s in range(self.n):
            if mol[s] >= 0:
                continue
            stack, comp = [s], {s}
            while stack:
                p = stack.pop()
                for q in g[p]:
                    if q not in comp:
                        comp.add(q); stack.append(q)
            for p in comp:
                mol[p] = min(comp)
        return mol

    def state(self):
        g = self.graph()
        rows = [sorted(b for (a, b) in self.excl if a == i) + sorted(a for (a, b) in self.excl if b == i) for i in range(self.n)]
        return dict(lists=[list(l) for l in self.bonds] + [list(self.angles)], graph=[sorted(x) for x in g],
                    excl=[sorted(r) for r in rows], npairs=len(self.excl), log=sorted(self.excl), mol=self.mol())


def parse_dumps(out, n, nlists):
    it = iter(out)
    dumps, ins = [], []
    for line in it:
        if line.startswith("ins"):
            ins.append(int(line.split()[1]))
            continue
        d = dict(lists=[], seen_ok=True)
        for _ in range(nlists):
            _, li, ar, cnt, _, used, allin = line.split()
            d["lists"].append([tuple(int(x) for x in next(it).split()) for _ in range(int(cnt))])
            d["seen_ok"] &= int(used) == int(cnt) and int(allin) == 1
            line = next(it)
        assert line == "graph"
        d["graph"] = [[int(x) for x in next(it).split(":")[1].split()] for _ in range(n)]
        d["npairs"] = int(next(it).split()[1])
        d["excl"] = [[int(x) for x in next(it).split(":")[1].split()] for _ in range(n)]
        nlog = int(next(it).split()[1])
        d["log"] = [tuple(int(x) for x in next(it).split()) for _ in range(nlog)]
        assert next(it) == "mol"
        d["mol"] = [int(next(it)) for _ in range(n)]
        assert next(it) == "end"
        dumps.append(d)
    return dumps, ins


def drive(exe, n, types, reg, script):
    """script: ('bond', li, a, b) | ('remove', [(li, a, b, unexclude), ...]); a dump follows every command."""
    lines = ["n %d" % n] + ["type %d %d" % (i, t) for i, t in enumerate(types)] + ["list 2", "list 2", "list 3"]
    lines += ["reg 2 %d %d %d" % tuple(r) for r in reg]
    m = Model(n, types, 2, reg)
    want, want_ins = [], []
    for cmd in script:
        if cmd[0] == "bond":
            lines.append("bond %d %d %d" % cmd[1:])
            want_ins.append(int(m.add_bond(*cmd[1:])))
        else:
            lines.append("remove %d " % len(cmd[1]) + " ".join("%d %d %d %d" % b for b in cmd[1]))
            m.remove(cmd[1])
        lines.append("dump")
        want.append(m.state())
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    got, ins = parse_dumps(out, n, 3)
    assert ins == want_ins
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["seen_ok"], "de-duplication set out of step with its list after command %d" % k
        for f in ("lists", "graph", "excl", "npairs", "log", "mol"):
            assert g[f] == w[f], (k, script[k], f)
    return got


def test_removal_in_a_ring_splits_nothing(harness):
    n = 12
    ring = [("bond", 0, k + 2, (k + 1) % 8 + 2) for k in range(8)]            # tags 2..9; 0, 1, 10, 11 stay alone
    script = ring + [("remove", [(0, 5, 4, 1)])]                                # given reversed: the key is orientation-free
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script)
    assert got[-1]["mol"][2:10] == [2] * 8 and len(got[-1]["lists"][0]) == 7
    assert len(got[-2]["lists"][2]) == 8 and len(got[-1]["lists"][2]) == 6    # the two angles across the broken bond left
    # a second cut splits the open chain 5-6-7-8-9-2-3-4 into 5-6-7 and 8-9-2-3-4
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script + [("remove", [(0, 7, 8, 1)])])
    mol = got[-1]["mol"]
    assert [mol[t] for t in (5, 6, 7)] == [5] * 3 and [mol[t] for t in (8, 9, 2, 3, 4)] == [2] * 5


def test_removal_in_a_tree_splits_two_fragments(harness):
    #        0
    #      /   \
    #     3     7 - 9
    #    / \    |
    #   5   1   8 - 2
    n = 10
    edges = [(0, 3), (0, 7), (3, 5), (3, 1), (7, 9), (7, 8), (8, 2)]
    script = [("bond", 0, a, b) for a, b in edges]
    script += [("remove", [(0, 0, 7, 0)])]                                      # exclusion kept
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script)
    mol = got[-1]["mol"]
    assert [mol[t] for t in (0, 1, 3, 5)] == [0] * 4 and [mol[t] for t in (2, 7, 8, 9)] == [2] * 4
    assert 7 in got[-1]["excl"][0]
    # several bonds of one particle in one batch, with and without their exclusions
    script2 = script + [("remove", [(0, 3, 5, 1), (0, 3, 1, 0), (0, 8, 7, 1)])]
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script2)
    assert got[-1]["mol"] == [0, 1, 2, 0, 4, 5, 6, 7, 2, 7]


def test_a_removed_bond_can_be_inserted_again(harness):
    n = 6
    script = [("bond", 0, 0, 1), ("bond", 0, 1, 2), ("bond", 0, 1, 0),          # the reversed duplicate is rejected
              ("remove", [(0, 1, 0, 1)]), ("bond", 0, 1, 0), ("bond", 0, 0, 1),
              ("remove", [(0, 0, 1, 1), (0, 2, 1, 1)]), ("bond", 0, 2, 1), ("bond", 0, 0, 1)]
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script)
    assert got[-1]["lists"][0] == [(2, 1), (0, 1)] and got[-1]["lists"][2] == [(0, 1, 2)]


def test_a_pair_held_by_another_list_stays_in_the_graph(harness):
    n = 5
    script = [("bond", 0, 0, 1), ("bond", 1, 1, 0), ("bond", 0, 1, 2), ("remove", [(0, 0, 1, 1)])]
    got = drive(harness, n, [0] * n, [(0, 0, 0)], script)
    assert got[-1]["graph"][0] == [1] and got[-1]["lists"][2] == [(0, 1, 2)] and got[-1]["mol"][:3] == [0, 0, 0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_removals_against_brute_force(harness, seed):
    """Hash-set erasure under load (backward shifts across wrapped probe runs), hubs with more than six partners (rows on
    the heap), typed angle spawning, batches that hit one particle several times."""
    rng = np.random.default_rng(seed)
    n = 70
    types = rng.integers(0, 2, n).tolist()
    reg = [(0, 0, 1), (1, 1, 1), (0, 1, 0)]
    script, have = [], []
    for a in range(1, 10):
        script.append(("bond", 0, 0, a)); have.append((0, 0, a))              # a hub
    for _ in range(6):
        for _ in range(25):
            a, b = (int(x) for x in rng.choice(n, 2, replace=False))
            li = int(rng.integers(0, 2))
            script.append(("bond", li, a, b)); have.append((li, a, b))
        pick = rng.permutation(len(have))[:12]
        batch = [have[i] + (int(rng.integers(0, 2)),) for i in pick]
        batch = [(li, b, a, u) if rng.integers(0, 2) else (li, a, b, u) for li, a, b, u in batch]
        script.append(("remove", batch))
        have = [h for i, h in enumerate(have) if i not in set(pick.tolist())]
    drive(harness, n, types, reg, script)
