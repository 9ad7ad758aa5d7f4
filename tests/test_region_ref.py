"""tests/region_ref.py, the numpy restatement of the region rules (include/chem_mi355.h, chem_region_add ff.), against the
header's own draw and against hand-made candidate sets.  Nothing here needs a GPU.

draw     region_draw in Python is chem_philox::region_draw of include/chem_philox.h (compiled into a tiny program);
modes    ties in the key broken by tag, num larger than |C|, fraction 0.999 of three candidates gives 2, prob 0 and 1;
box      lo is inside, hi is outside, the fold of chem_get_state(CHEM_STATE_POS);
order    rules in insertion order, a later rule sees the type an earlier one left; the interval."""
import os
import subprocess

import numpy as np

import react_ref as RR
import region_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = np.array([6.0, 6.0, 6.0])
ALL = ([0, 0, 0], BOX)


def test_region_draw_matches_the_header(tmp_path):
    cases = [(0, 0, 0, 0), (0, 1, 2, 3), (0x1234567887654321, 7, 123456, 5), (2 ** 64 - 1, 2 ** 33 + 5, 2 ** 27 - 1, 15)]
    src = tmp_path / "draw.cpp"
    src.write_text('#include <cstdio>\n#include "chem_philox.h"\nint main() {\n  uint32_t o[4];\n' +
                   "".join("  chem_philox::region_draw(%dull, %dull, %du, %du, o); printf(\"%%u %%u %%u %%u\\n\", o[0], o[1], o[2], o[3]);\n" % c for c in cases) +
                   "  return 0;\n}\n")
    exe = str(tmp_path / "draw")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for c, line in zip(cases, out):
        assert tuple(int(x) for x in line.split()) == G.region_draw(*c)
    # a stream of its own: not the ATRP draw of that tag, and the rule index matters
    assert G.region_draw(5, 9, 3, 0) != tuple(RR.atrp_draw(5, 9, 3))
    assert G.region_draw(5, 9, 3, 0) != G.region_draw(5, 9, 3, 1)


def test_mode_all_and_prob_limits():
    cand = [7, 3, 11, 5]
    assert G.pick(G.rule(*ALL, 1, 2), 0, 4, cand) == [3, 5, 7, 11]
    assert G.pick(G.rule(*ALL, 1, 2, mode=G.MODE_PROB, value=0.0, seed=9), 0, 4, cand) == []
    assert G.pick(G.rule(*ALL, 1, 2, mode=G.MODE_PROB, value=1.0, seed=9), 0, 4, cand) == [3, 5, 7, 11]
    # in between: exactly the tags whose uniform lies below the value
    r = G.rule(*ALL, 1, 2, mode=G.MODE_PROB, value=0.5, seed=9)
    tags = list(range(200))
    want = [t for t in tags if G.u01(G.region_draw(9, 4, t, 3)[1]) < 0.5]
    assert G.pick(r, 3, 4, tags) == want and 60 < len(want) < 140


def test_mode_num_takes_the_smallest_keys_and_caps_at_the_candidates():
    r = G.rule(*ALL, 1, 2, mode=G.MODE_NUM, num=3, seed=77)
    tags = list(range(40, 60))
    keys = sorted((G.region_draw(77, 10, t, 2)[0], t) for t in tags)
    assert G.pick(r, 2, 10, tags[::-1]) == sorted(t for _, t in keys[:3])
    r["num"] = 100
    assert G.pick(r, 2, 10, tags) == tags
    r["num"] = 0
    assert G.pick(r, 2, 10, tags) == []


def test_ties_in_the_key_are_broken_by_tag(monkeypatch):
    monkeypatch.setattr(G, "region_draw", lambda seed, step, tag, rule: (5 if tag in (2, 9, 4) else 6 + tag, 0, 0, 0))
    r = G.rule(*ALL, 1, 2, mode=G.MODE_NUM, num=2)
    assert G.pick(r, 0, 1, [9, 1, 4, 2]) == [2, 4]


def test_fraction_is_floored():
    tags = [1, 2, 3]
    for value, k in ((0.999, 2), (1.0, 3), (0.0, 0), (0.33, 0), (0.34, 1)):
        r = G.rule(*ALL, 1, 2, mode=G.MODE_FRACTION, value=value, seed=1)
        got = G.pick(r, 0, 3, tags)
        assert len(got) == k
        keys = sorted((G.region_draw(1, 3, t, 0)[0], t) for t in tags)
        assert got == sorted(t for _, t in keys[:k])


def test_box_edges_and_fold():
    r = G.rule([1.0, 0.0, 0.0], [2.0, 6.0, 6.0], 1, 2)
    pos = np.array([[1.0, 3, 3], [2.0, 3, 3], [np.nextafter(2.0, 0), 3, 3], [np.nextafter(1.0, 0), 3, 3], [7.5, 3, 3], [-4.5, 9, -3]])
    f = G.fold(pos, BOX)
    assert G.inside(r, f).tolist() == [True, False, True, False, True, True]
    assert np.all((f >= 0) & (f < BOX))
    assert G.fold(np.array([6.0, -0.0, 12.0]), BOX).tolist() == [0.0, 0.0, 0.0]


def test_rules_act_in_order_and_see_earlier_changes():
    pos = np.array([[0.5, 0.5, 0.5], [0.5, 3.0, 3.0], [3.0, 0.5, 3.0], [3.0, 3.0, 3.0]])
    types = np.array([1, 1, 1, 1])
    rules = [G.rule([0, 0, 0], [1, 6, 6], 1, 5), G.rule([0, 0, 0], [6, 1, 6], 1, 6), G.rule([0, 0, 0], [6, 6, 6], 6, 7)]
    ch, st = G.fire(rules, 1, pos, types)
    # the corner particle 0 is in both slabs: the first rule takes it, the second no longer sees type 1; the third rule sees
    # what the second made
    assert ch == [(1, 0, 0), (1, 1, 0), (1, 2, 1), (1, 2, 2)]
    assert st == [(1, 0, 2, 2), (1, 1, 1, 1), (1, 2, 1, 1)]
    assert types.tolist() == [5, 5, 7, 1]


def test_interval_and_enable():
    pos = {s: np.array([[0.5, 0.5, 0.5]]) for s in range(0, 8)}
    r = G.rule([0, 0, 0], [1, 1, 1], 1, 2, interval=3)
    assert [G.due(r, s) for s in range(8)] == [False, False, False, True, False, False, True, False]
    ch, st, ty = G.run([r], pos, [1], BOX)
    assert ch == [(3, 0, 0)] and ty.tolist() == [2]
    r["enabled"] = False
    assert G.run([r], pos, [1], BOX)[0] == []
