"""tests/reverse_ref.py against cases worked out by hand (no GPU, no product code): which bonds a visit removes, what a
removal leaves behind, which joins are accepted, where a joined target is put."""
import numpy as np

import fixdist_ref as FX
import reverse_ref as RV

A, C, E, W = 0, 1, 2, 3


def graph_of(n, bonds):
    g = [set() for _ in range(n)]
    for a, b in bonds:
        g[a].add(b); g[b].add(a)
    return g


def rule(**kw):
    return dict(dict(reaction=0, invoke_on=3, anchor_type=C, nb_level=1, type_1=C, type_2=E, unexclude=1), **kw)


def test_levels_on_a_chain_a_ring_and_a_star():
    chain = graph_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    assert RV.levels(chain, 2, 3) == {2: 0, 1: 1, 3: 1, 0: 2, 4: 2}
    ring = graph_of(5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)])
    assert RV.levels(ring, 0, 3) == {0: 0, 1: 1, 4: 1, 2: 2, 3: 2}          # nothing at distance 3 on a ring of five
    star = graph_of(5, [(0, 1), (0, 2), (0, 3), (0, 4)])
    assert RV.levels(star, 1, 2) == {1: 0, 0: 1, 2: 2, 3: 2, 4: 2}


def test_level_one_removes_the_anchors_own_bond():
    # 0(C) - 1(E) - 2(A); event (0, 3) of reaction C + W: role 1 is the C
    g, types = graph_of(4, [(0, 1), (1, 2)]), [C, E, A, W]
    assert RV.select_removals(g, types, [(C, W)], [rule()], [(0, 3, 0)]) == [(0, 1, 0, 1)]
    # the role's type is the reaction's own, not the particle's: a rule anchored on W visits role 2 only, and finds no C-E there
    assert RV.select_removals(g, types, [(C, W)], [rule(anchor_type=W)], [(0, 3, 0)]) == []
    # invoke_on = 2 never looks at role 1
    assert RV.select_removals(g, types, [(C, W)], [rule(invoke_on=2)], [(0, 3, 0)]) == []
    # another reaction's events do not count
    assert RV.select_removals(g, types, [(C, W), (C, W)], [rule(reaction=1)], [(0, 3, 0)]) == []


def test_level_two_and_three_take_the_bond_between_the_levels():
    # chain 0(C) - 1(A) - 2(C) - 3(E) - 4(C) - 5(E), event on 0
    g, types = graph_of(7, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]), [C, A, C, E, C, E, W]
    sel = lambda lvl: RV.select_removals(g, types, [(C, W)], [rule(nb_level=lvl)], [(0, 6, 0)])      # noqa: E731
    assert sel(1) == [] and sel(2) == []
    assert sel(3) == [(2, 3, 0, 1)]                 # near = the end closer to the anchor
    assert sel(4) == [(3, 4, 0, 1)]                 # {E, C} matches {C, E}: the pair is unordered
    # ring of four 0(C) 1(E) 2(C) 3(E): level 2 from 0 finds (1, 2) and (3, 2), by (p, q); (0, 1) and (0, 3) are level 1
    ring, rt = graph_of(5, [(0, 1), (1, 2), (2, 3), (3, 0)]), [C, E, C, E, W]
    assert RV.select_removals(ring, rt, [(C, W)], [rule(nb_level=2)], [(0, 4, 0)]) == [(1, 2, 0, 1), (3, 2, 0, 1)]
    assert RV.select_removals(ring, rt, [(C, W)], [rule(nb_level=1)], [(0, 4, 0)]) == [(0, 1, 0, 1), (0, 3, 0, 1)]
    # a bond inside one level (a triangle's far side) lies between no two levels
    tri, tt = graph_of(4, [(0, 1), (0, 2), (1, 2)]), [A, C, E, W]
    assert RV.select_removals(tri, tt, [(A, W)], [rule(anchor_type=A, nb_level=2)], [(0, 3, 0)]) == []


def test_types_are_those_before_the_events():
    # the event itself turns 1 from E into A (type0 still says E): the bond C-E is found
    g = graph_of(3, [(0, 1)])
    assert RV.select_removals(g, [C, E, W], [(C, W)], [rule()], [(0, 2, 0)]) == [(0, 1, 0, 1)]
    assert RV.select_removals(g, [C, A, W], [(C, W)], [rule()], [(0, 2, 0)]) == []


def test_a_bond_found_twice_counts_for_the_first_visit():
    # 0(C) - 1(C), two events (0, 2) and (1, 3) of reactions 0 and 1 with one rule each on C-C
    g, types = graph_of(4, [(0, 1)]), [C, C, W, W]
    rules = [rule(reaction=0, type_2=C, unexclude=0), rule(reaction=1, type_2=C, unexclude=1)]
    assert RV.select_removals(g, types, [(C, W), (C, W)], rules, [(0, 2, 0), (1, 3, 1)]) == [(0, 1, 0, 0)]


def test_removal_from_two_lists_and_fragment_labels():
    g = graph_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    lists = [[(0, 1), (1, 2), (2, 3), (3, 4)], [(2, 1), (4, 3)]]
    excl, mol = {(0, 1), (1, 2), (2, 3), (3, 4)}, [0] * 5
    recs = RV.apply_removals(g, lists, excl, mol, [(1, 2, 0, 1), (3, 4, 7, 0)])
    assert recs == [(1, 2, 0, 0), (1, 2, 1, 0), (3, 4, 0, 7), (3, 4, 1, 7)]
    assert lists == [[(0, 1), (2, 3)], []]
    assert excl == {(0, 1), (2, 3), (3, 4)}                                  # unexclude = 0 keeps (3, 4) excluded
    assert mol == [0, 0, 2, 2, 4]
    assert g == [{1}, {0}, {3}, {2}, set()]


def test_joins_accept_and_refuse():
    s = FX.Sets(6)
    h = s.create()
    rules = [(0, 1, h, 0.25), (0, 2, h, 0.5)]
    # event (0, 3): rule 1 joins 3 to 0; rule 2 would join 0 to 3, but 3 is a target and 0 an anchor by then
    log, added = RV.apply_joins(s, rules, [(0, 3, 0), (1, 4, 1), (2, 0, 0)], 5)
    assert log == [(5, h, 0, 3, 3), (5, h, 3, 0, 4), (5, h, 2, 0, 4), (5, h, 0, 2, 3)]
    assert added == [(0, 3, 0.25), (0, 2, 0.5)]
    assert [e[:4] for e in s.entries(h)] == [(0, 3, 0.25, 0), (0, 2, 0.5, 1)]     # insertion order continues, refusals take no index


def test_placement():
    box = np.array([4.0, 4.0, 4.0])
    x = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3.75, 0.5, 0.5], [3.75, 3.75, 3.75], [1.0, 2.0, 2.0]])
    v = np.arange(15.0).reshape(5, 3)
    # target on the anchor: u = (1, 0, 0); across a face; across a corner
    x1, v1 = RV.place(x, v, [(0, 1, 0.25)], box)
    assert np.array_equal(x1[1], [0.75, 0.5, 0.5]) and np.array_equal(v1[1], v[0])
    x2, _ = RV.place(x, v, [(0, 2, 0.25)], box)
    assert np.array_equal(x2[2], [4.25, 0.5, 0.5])                           # on the image it was on: 0.25 to the left of x = 4.5
    x3, _ = RV.place(x, v, [(0, 3, np.sqrt(3.0) / 4)], box)
    assert np.allclose(x3[3], [4.25, 4.25, 4.25], rtol=0, atol=1e-15)
    assert np.array_equal(np.delete(x1, 1, 0), np.delete(x, 1, 0))
