"""Reverse reactions (include/chem_mi355.h, chem_reaction_remove_bond / chem_reaction_join) restated in plain Python / numpy on
top of tests/react_ref.py (the association events) and tests/fixdist_ref.py (the sets and the constraint).  Imports nothing
from the product.

Order inside one reaction step: association events (react_ref.Reference.step), REMOVALS, JOINS; the caller goes on with the
release by reaction and by type (fixdist_ref.Sets), as the header orders them.

Removal   events of the rule's reaction in (min id, max id) order, role 1 before role 2, rules in insertion order; a role is
          visited if invoke_on includes it and the reaction's own type of that role equals anchor_type; from the anchor every
          bond (p, q) of the graph (this step's new bonds in, nothing of this step out yet) with d(anchor, p) = nb_level - 1 and
          d(anchor, q) = nb_level, by (p, q), whose unordered type pair AT THE START of the association phase equals
          {type_1, type_2}.  A bond found twice counts for the first visit.  The pair leaves every pair list that holds it
          (one record per list, lists in handle order), the graph, with unexclude its exclusion; every fragment gets
          mol_id = its lowest particle; res_id stays.
Join      per event, per rule of its reaction in insertion order: (anchor = the reactant in the rule's role, target = the
          other one, dist) is appended to the set if fixdist_ref.Sets.add accepts the pair (cause 3), else logged with cause 4.
Placement fixdist_ref.constrain."""
import numpy as np

import fixdist_ref as FX
import react_ref as RR

CAUSE_JOINED, CAUSE_REFUSED = 3, 4


def levels(graph, root, upto):
    """{particle: graph distance from root} for distances 0 .. upto"""
    dist, frontier = {root: 0}, [root]
    for lvl in range(1, upto + 1):
        nxt = []
        for p in frontier:
            for nb in sorted(graph[p]):
                if nb not in dist:
                    dist[nb] = lvl; nxt.append(nb)
        frontier = nxt
    return dist


def select_removals(graph, type0, reactions, rules, events):
    """rules: dicts (reaction, invoke_on, anchor_type, nb_level, type_1, type_2, unexclude); reactions: (type_1, type_2) per
    reaction; events: (a, b, reaction) in canonical order.  Returns [(p, q, reaction, unexclude)] in visit order."""
    out, found = [], set()
    for a, b, r in events:
        for role in (1, 2):
            for rl in rules:
                if rl["reaction"] != r or not (rl["invoke_on"] & role) or reactions[r][role - 1] != rl["anchor_type"]:
                    continue
                dist = levels(graph, a if role == 1 else b, rl["nb_level"])
                for p in sorted(x for x, d in dist.items() if d == rl["nb_level"] - 1):
                    for q in sorted(graph[p]):
                        if dist.get(q) != rl["nb_level"] or {type0[p], type0[q]} != {rl["type_1"], rl["type_2"]}:
                            continue
                        if (min(p, q), max(p, q)) in found:
                            continue
                        found.add((min(p, q), max(p, q)))
                        out.append((p, q, r, rl["unexclude"]))
    return out


def apply_removals(graph, lists, excl, mol, rem):
    """rem from select_removals.  Updates the pair lists (lists of (a, b), survivors in order), the graph, the exclusion set of
    (lo, hi) and mol in place; returns the records (p, q, list, reaction), one per list that held the pair."""
    recs = []
    for p, q, r, unex in rem:
        for li, l in enumerate(lists):
            if any({e[0], e[1]} == {p, q} for e in l):
                l[:] = [e for e in l if {e[0], e[1]} != {p, q}]
                recs.append((p, q, li, r))
    for p, q, r, unex in rem:
        graph[p].discard(q); graph[q].discard(p)
        if unex:
            excl.discard((min(p, q), max(p, q)))
    for p, q, r, unex in rem:
        for root in (p, q):
            comp = sorted(levels(graph, root, len(graph)))
            for x in comp:
                mol[x] = comp[0]
    return recs


def apply_joins(sets, join_rules, events, step):
    """join_rules: (reaction, role, set, dist); events (a, b, reaction) in canonical order.  Returns (log records
    (step, set, anchor, target, cause), new entries (anchor, target, dist))."""
    log, added = [], []
    for a, b, r in events:
        for rr, role, h, d in join_rules:
            if rr != r:
                continue
            an, tg = (a, b) if role == 1 else (b, a)
            ok = sets.add(h, [(an, tg)], d)
            log.append((int(step), h, an, tg, CAUSE_JOINED if ok else CAUSE_REFUSED))
            if ok:
                added.append((an, tg, d))
    return log, added


class Reverse:
    """react_ref.Reference plus the pair lists by handle, the removal rules, the join rules and the fixed-distance sets.
    Particles are tags (index in ascending id order) inside, ids in everything reported."""

    def __init__(self, spec):
        self.ref = RR.Reference(spec)
        tag = {int(i): t for t, i in enumerate(self.ref.ids)}
        self.lists = [[(tag[int(a)], tag[int(b)]) for a, b in np.asarray(l["ids"]).reshape(-1, 2)] for l in spec.get("lists", [])]
        self.bond_list = len(self.lists)          # workloads.apply creates the reaction's list behind the spec's lists
        self.lists.append([])
        self.sets = FX.Sets(self.ref.n)
        self.rm_rules, self.join_rules = [], []   # dicts; (reaction, role, set, dist)
        self.removed, self.joins = [], []         # (step, id_near, id_far, list, reaction); (step, set, anchor id, target id, cause)

    def step(self, step, pos=None, after_events=None):
        """One reaction step up to and including the joins.  after_events(events in tags): what the caller does between the
        events and the removals (neighbour changes: react_ref has none).  Returns (events, removal records, new entries
        (a, t, d) in tags)."""
        R = self.ref
        type0 = R.type.copy()
        nb0 = len(R.bonds)
        ev, _ = R.step(step, pos)
        tag = {int(i): t for t, i in enumerate(R.ids)}
        self.lists[self.bond_list] += [(tag[a], tag[b]) for a, b in R.bonds[nb0:]]
        events = [(tag[a], tag[b], r) for _, a, b, r, _ in ev]
        if after_events is not None:
            after_events(events)
        rem = select_removals(R.graph, type0, [(x["type_1"], x["type_2"]) for x in R.rx], self.rm_rules, events)
        recs = [(int(step), int(R.ids[p]), int(R.ids[q]), li, r) for p, q, li, r in apply_removals(R.graph, self.lists, R.excl, R.mol, rem)]
        R.bonds = [(int(R.ids[a]), int(R.ids[b])) for a, b in self.lists[self.bond_list]]
        self.removed += recs
        log, added = apply_joins(self.sets, self.join_rules, events, step)
        self.joins += [(s_, h, int(R.ids[a]), int(R.ids[t]), c) for s_, h, a, t, c in log]
        return ev, recs, added

    def list_ids(self, h):
        return np.asarray([(int(self.ref.ids[a]), int(self.ref.ids[b])) for a, b in self.lists[h]], dtype=np.int64).reshape(-1, 2)


def place(x, v, added, box):
    """positions (unfolded) and velocities after the placement of the new entries"""
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    for a, t, d in added:
        x[t] = FX.constrain(x[a], x[t], np.float64(d), box)
        v[t] = v[a]
    return x, v
