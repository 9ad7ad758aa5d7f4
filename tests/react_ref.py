"""The association reaction step restated in plain Python / numpy, and a zoo of frozen systems built to reach what thermal
melts never reach.

The rules are those of include/chem_mi355.h (chem_reaction_desc, chem_event, chem_reaction_init), include/chem_philox.h
(reaction_draw, u01) and the comment blocks of the reaction kernels; nothing here calls the oracle or the engine.

Candidates   every unordered pair once, from its lower tag (tag = rank of the id); excluded pairs never; for each active
             reaction the forward role assignment (lower tag = type_1) first, then the reversed one; type and half-open state
             windows; intraresidual / intramolecular; mincut2 <= d2 < cut2 with d2 the fp64 minimum-image distance in the
             operation order of minimgD and dist2_unfused: d = x_lo - x_hi, d -= L * rint(d * (1 / L)), (dx dx + dy dy) + dz dz.
             Every zoo box edge is a power of two, so L * rint(..) and d * (1 / L) are exact and a fused multiply-add in minimgD
             gives the same bits: nothing in the chain is left unrestated.  prob = rate * dt * interval; below 1 the pair is
             accepted iff u01(out[0]) < prob, out = reaction_draw(seed, step, tag_lo, tag_hi, r).
Resolve      UniqueA (per role-1 particle the smallest (key, partner tag, reaction)), UniqueB on its survivors, then greedy in
             (key, role-1 tag) order; key = d2 (nearest) or out[1]; max_per_interval keeps the first k of that order.
Apply        state deltas; a CHANGE of type sets the mass, a named type sets the charge; a bond (role 1, role 2) goes into the
             list in (min id, max id) order of the step's events unless the reaction is virtual, with its 1-2 exclusion; with
             all bonds of the step in the graph, each bond in that order gives its cluster mol_id = the lowest particle id and
             res_id = min(res_id[a], res_id[b]) as they are at its turn (chem_reaction_init states this rule).
Round model  rounds(): the number of k_res_round launches after which no survivor is undecided.

What hangs onto a reaction, by the rules of the same header (chem_reaction_restrict, chem_reaction_constraint, chem_event.pad,
chem_topology_register, chem_reaction_neighbour_change, chem_atrp_desc):
Restrict     a restricted reaction accepts only the unordered id pairs of its list; calls accumulate.
Constraint   one per reaction, the last call wins; the holder of the constrained role after the role assignment above (forward
             first, no retry) needs a bonded neighbour of nb_type with state in [min, max); graph, types and states as they are
             when the scan starts.
pad          with count_intra_inter: 1 when both reactants had one mol_id before this step's bonds.
Spawn        after the relabelling, per new bond in canonical order, on the types the events left: _spawn / _spawn_tuple.
Nb change    after the spawn: events in canonical order, role 1 before role 2, rules in insertion order, the exact shell of
             nb_level bonds in ascending tag; every visit reads what the visits before it wrote.
ATRP         atrp_model: one firing; member() fires it behind the reaction step where both fall on one step.
"""
import numpy as np

from test_philox import philox_py

RC, SKIN, DT = 1.5, 0.3, 0.001
GRID = 1.0 / 1024.0
_RX = dict(delta_1=0, delta_2=0, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1, rate=1e9, min_cutoff=0.0,
           intramolecular=False, intraresidual=False, is_virtual=False, active=True, new_type_1=-1, new_type_2=-1, new_q_1=0.0, new_q_2=0.0)


def u01(x):
    return (float(x) + 0.5) * (1.0 / 4294967296.0)


def reaction_draw(seed, step, lo, hi, r):
    ctr = (int(lo), int(hi), int(step) & 0xffffffff, ((int(r) << 24) & 0xffffffff) ^ ((int(step) >> 32) & 0xffffffff))
    key = ((int(seed) & 0xffffffff) ^ 0x52454143, (int(seed) >> 32) & 0xffffffff)
    return philox_py(ctr, key)


def atrp_draw(seed, step, tag):
    ctr = (int(tag), int(step) & 0xffffffff, (int(step) >> 32) & 0xffffffff, 0x41545250)
    key = ((int(seed) & 0xffffffff) ^ 0x41435456, (int(seed) >> 32) & 0xffffffff)
    return philox_py(ctr, key)


def dist2(L, xi, xj):
    """|minimum image of xi - xj|^2 for one xi against rows xj, unfused, in the header's order."""
    d = xi - xj
    d = d - L * np.rint(d * (1.0 / L))
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return (xx + yy) + zz


def atrp_model(types, states, mass, q, A, step):
    """One firing of the ATRP activator by the rule set of chem_atrp_desc, brute force: every particle of the pool draws
    atrp_draw(seed, step, tag); the num_particles smallest (out[0], tag) are visited in that order; a visited particle that matches
    a centre (the first in insertion order with its type and state) flips where u01(out[1]) < k * the consumed share, which moves
    min(delta_catalyst / num_particles, share) to the other side.  Changes types, states, mass, q and A's two shares in place;
    returns (stats row, [(tag, type, state, mass, q)] of the flips in visit order)."""
    cen = A["centers"]

    def center_of(t):
        for c, C_ in enumerate(cen):
            if C_["type_id"] == types[t] and C_["state"] == states[t]:
                return c
        return -1
    pool, ncand = [], 0
    for t in range(len(types)):
        c = center_of(t)
        ncand += c >= 0
        if c < 0 and not A["select_from_all"]:
            continue
        o = atrp_draw(A["seed"], step, t)
        pool.append((o[0], t, o[1], c))
    pool.sort(key=lambda s: (s[0], s[1]))
    pool = pool[:A["num_particles"]]
    dc = A["delta_catalyst"] / float(A["num_particles"])
    row = dict(step=int(step), candidates=int(ncand), selected=len(pool), activated=0, deactivated=0)
    flips = []
    for _, t, u, c in pool:
        if c < 0:
            continue
        C_ = cen[c]
        p = A["k_deactivate"] * A["ratio_deactivator"] if C_["is_activator"] else A["k_activate"] * A["ratio_activator"]
        if not (u01(u) < p):
            continue
        if C_["new_type"] >= 0 and C_["new_type"] != types[t]:
            types[t] = C_["new_type"]; mass[t] = C_["new_mass"]; q[t] = C_.get("new_q", 0.0)
        states[t] += C_.get("delta_state", 0)
        flips.append((t, int(types[t]), int(states[t]), float(mass[t]), float(q[t])))
        if C_["is_activator"]:
            m = min(dc, A["ratio_deactivator"]); A["ratio_deactivator"] -= m; A["ratio_activator"] += m; row["deactivated"] += 1
        else:
            m = min(dc, A["ratio_activator"]); A["ratio_activator"] -= m; A["ratio_deactivator"] += m; row["activated"] += 1
    row["ratio_activator"], row["ratio_deactivator"] = A["ratio_activator"], A["ratio_deactivator"]
    return row, flips


class Reference:
    """State of one system across reaction steps.  Tags are 0 .. n-1 in ascending id order; everything reported uses ids."""

    def __init__(self, spec):
        self.ids = np.asarray(spec["ids"], dtype=np.int64)
        assert np.all(np.diff(self.ids) > 0)
        n = self.n = len(self.ids)
        tag = {int(i): t for t, i in enumerate(self.ids)}
        self.L = np.asarray(spec["box"], dtype=np.float64)
        self.pos = np.asarray(spec["pos"], dtype=np.float64).copy()
        self.type = np.asarray(spec["types"], dtype=np.int64).copy()
        self.state = np.asarray(spec.get("state", np.zeros(n)), dtype=np.int64).copy()
        self.res = np.asarray(spec.get("res_id", self.ids), dtype=np.int64).copy()
        self.mass = np.broadcast_to(np.asarray(spec["mass"], dtype=np.float64), (n,)).copy()
        self.q = np.zeros(n)
        self.mol = np.arange(n)
        self.graph = [set() for _ in range(n)]
        self.excl = set()
        for a, b in np.asarray(spec.get("exclusions", []), dtype=np.int64).reshape(-1, 2):
            self.excl.add((min(tag[int(a)], tag[int(b)]), max(tag[int(a)], tag[int(b)])))
        self.lists = []                          # every list of the spec in handle order: dict(arity, reg, ent, seen); the reaction bonds are self.bonds
        for l in spec.get("lists", []):          # bonds that exist from the start: graph and cluster labels, no exclusion of their own
            ar = l["arity"]
            ent = [tuple(tag[int(x)] for x in row) for row in np.asarray(l["ids"], dtype=np.int64).reshape(-1, ar)]
            self.lists.append(dict(arity=ar, reg=[tuple(int(x) for x in g) for g in l.get("register", [])], ent=ent, seen={min(t, t[::-1]) for t in ent}))
            if ar == 2:
                for a, b in ent:
                    self._link(a, b)
                self._relabel(ent, res=False)
        rx = spec["reaction"]
        self.interval, self.nearest, self.mpi, self.seed = rx["interval"], rx["nearest"], rx.get("max_per_interval", 0), rx["seed"]
        self.rx = []
        for r in rx["reactions"]:
            r = dict(_RX, **r)
            for k in (1, 2):
                if r["new_type_%d" % k] >= 0:
                    r["new_mass_%d" % k] = rx["type_mass"][r["new_type_%d" % k]]
            r["cut2"], r["mincut2"] = r["cutoff"] * r["cutoff"], r["min_cutoff"] * r["min_cutoff"]
            r["prob"] = r["rate"] * spec["dt"] * float(self.interval)
            self.rx.append(r)
        assert len(self.rx) <= 16
        self.bonds, self.events, self.pads, self.spawn_log = [], [], [], []
        ext = spec.get("ext", {})
        self.intra_inter = bool(ext.get("options", {}).get("count_intra_inter", 0))
        self.restrict = {}                       # reaction -> set of (tag lo, tag hi); calls accumulate
        for r, pairs in ext.get("restrict", []):
            self.restrict.setdefault(r, set()).update((min(tag[int(a)], tag[int(b)]), max(tag[int(a)], tag[int(b)])) for a, b in np.asarray(pairs).reshape(-1, 2))
        self.cons = {}                           # reaction -> (role, nb_type, min, max): one per reaction, the last call wins
        for r, role, nbt, lo, hi in ext.get("constraint", []):
            self.cons[r] = (role, nbt, lo, hi)
        self.nb_rules = [dict(dict(new_q=0.0, set_state=0, new_state=0, window=None), **rl) for rl in ext.get("nb_change", [])]
        at = spec.get("atrp")
        self.atrp = None if at is None else dict(at, seed=at.get("seed", spec.get("seed", 0)), select_from_all=at.get("select_from_all", True))
        self.atrp_rows = []

    # ---- labels ----
    def _link(self, a, b):
        self.graph[a].add(b); self.graph[b].add(a)

    def _relabel(self, bonds, res=True):
        """bonds (a, b), all in the graph already, in (min id, max id) order: the cluster that holds them gets the lowest tag
        as mol_id and, from each bond in turn, min(res_id[a], res_id[b]) as these are when its turn comes."""
        for a, b in bonds:
            comp, stack = {a}, [a]
            while stack:
                for nb in self.graph[stack.pop()]:
                    if nb not in comp:
                        comp.add(nb); stack.append(nb)
            c = sorted(comp)
            self.mol[c] = c[0]
            if res:
                self.res[c] = min(self.res[a], self.res[b])

    # ---- one reaction step ----
    def candidates(self, step, pos=None):
        """[(a, b, r, d2, h)] in tags; h is None where nothing needs the draw."""
        pos = self.pos if pos is None else np.asarray(pos, dtype=np.float64)
        act = [(k, R) for k, R in enumerate(self.rx) if R["active"]]
        maxcut2 = max(R["cut2"] for _, R in act)
        out = []
        for i in range(self.n - 1):
            d2 = dist2(self.L, pos[i], pos[i + 1:])
            for jj in np.nonzero(d2 < maxcut2)[0]:
                j = i + 1 + int(jj)
                if (i, j) in self.excl:
                    continue
                dd = float(d2[jj])
                for k, R in act:
                    fits = lambda p, w: self.type[p] == R["type_%d" % w] and R["min_state_%d" % w] <= self.state[p] < R["max_state_%d" % w]   # noqa: E731
                    if fits(i, 1) and fits(j, 2):
                        a, b = i, j
                    elif fits(j, 1) and fits(i, 2):
                        a, b = j, i
                    else:
                        continue
                    if not R["intraresidual"] and self.res[i] == self.res[j]:
                        continue
                    if not R["intramolecular"] and self.mol[i] == self.mol[j]:
                        continue
                    if not (R["mincut2"] <= dd < R["cut2"]):
                        continue
                    if k in self.restrict and (i, j) not in self.restrict[k]:
                        continue
                    if k in self.cons:           # judged on the holder of the role after the assignment above: forward first, no retry
                        role, nbt, lo, hi = self.cons[k]
                        if not any(self.type[x] == nbt and lo <= self.state[x] < hi for x in self.graph[a if role == 1 else b]):
                            continue
                    h = None
                    if R["prob"] < 1.0 or not self.nearest:
                        o = reaction_draw(self.seed, step, i, j, k)
                        if R["prob"] < 1.0 and not (u01(o[0]) < R["prob"]):
                            continue
                        h = o[1]
                    out.append((a, b, k, dd, h))
        return out

    def _key(self, c):
        return c[3] if self.nearest else c[4]

    def unique(self, cand):
        for side, other in ((0, 1), (1, 0)):
            best = {}
            for c in cand:
                kq = (self._key(c), c[other], c[2])
                if c[side] not in best or kq < best[c[side]][0]:
                    best[c[side]] = (kq, c)
            cand = [v[1] for v in best.values()]
        return sorted(cand, key=lambda c: (self._key(c), c[0]))

    @staticmethod
    def greedy(surv):
        used, acc = set(), []
        for c in surv:
            if c[0] in used or c[1] in used:
                continue
            used.update(c[:2]); acc.append(c)
        return acc

    @staticmethod
    def rounds(surv):
        """(rounds, accepted) of the parallel matching on survivors given in priority order: in a round an undecided
        survivor dies beside an accepted one, is accepted where no undecided neighbour precedes it, waits otherwise."""
        byp = {}
        for k, c in enumerate(surv):
            byp.setdefault(c[0], []).append(k); byp.setdefault(c[1], []).append(k)
        st, n = [1] * len(surv), 0
        while 1 in st:
            n += 1
            new = list(st)
            for k, c in enumerate(surv):
                if st[k] != 1:
                    continue
                nb = [o for p in c[:2] for o in byp[p] if o != k]
                if any(st[o] == 2 for o in nb):
                    new[k] = 0
                elif not any(st[o] == 1 and o < k for o in nb):
                    new[k] = 2
            st = new
        return n, [c for k, c in enumerate(surv) if st[k] == 2]

    def step(self, step, pos=None, model=False):
        """Runs the reaction step `step`; returns its events [(step, id_a, id_b, reaction, d2)] in (min id, max id) order and
        a dict of what the zoo's conditions are stated on."""
        cand = self.candidates(step, pos)
        surv = self.unique(cand)
        acc = self.greedy(surv)
        info = dict(candidates=len(cand), survivors=len(surv), distinct_d2=len({c[3] for c in acc}), cand=cand)
        if model:
            info["rounds"], par = self.rounds(surv)
            assert par == acc
        if self.mpi > 0:
            acc = acc[:self.mpi]
        acc.sort(key=lambda c: (min(c[0], c[1]), max(c[0], c[1])))
        ev, new = [], []
        for a, b, k, d2, _ in acc:
            R = self.rx[k]
            for p, w in ((a, 1), (b, 2)):
                self.state[p] += R["delta_%d" % w]
                nt = R["new_type_%d" % w]
                if nt >= 0:
                    if self.type[p] != nt:
                        self.type[p] = nt; self.mass[p] = R["new_mass_%d" % w]
                    self.q[p] = R["new_q_%d" % w]
            ev.append((int(step), int(self.ids[a]), int(self.ids[b]), k, d2))
            self.pads.append(1 if self.intra_inter and self.mol[a] == self.mol[b] else 0)      # the labels are those before this step's bonds
            if not R["is_virtual"]:
                self.bonds.append((int(self.ids[a]), int(self.ids[b])))
                self.excl.add((min(a, b), max(a, b)))
                self._link(a, b); new.append((a, b))
        self._relabel(new)
        n_log = len(self.spawn_log)
        self._spawn(new)
        info["spawned"] = self.spawn_log[n_log:]
        info["nb_changed"] = self._neighbour_changes(acc)
        info["pad"] = self.pads[len(self.events):]
        self.events += ev
        return ev, info

    # ---- chem_topology_register: HostTopology::spawn_for_new_bonds / spawn_tuple restated ----
    def _spawn_tuple(self, t):
        """t goes to the first list of its arity, in handle order, that has a registered type tuple matching it forward or
        reversed (forward preferred), in the matching orientation; a list that holds it already, in either orientation, takes
        nothing (and no later list is tried); the (first, last) exclusion is added only where the tuple was inserted."""
        ty = tuple(int(self.type[p]) for p in t)
        hit = self.match(ty)
        if hit is None:
            return
        l, tt = self.lists[hit[0]], t[::-1] if hit[1] else t
        new = min(tt, tt[::-1]) not in l["seen"]
        if new:
            l["seen"].add(min(tt, tt[::-1])); l["ent"].append(tt)
            self.excl.add((min(tt[0], tt[-1]), max(tt[0], tt[-1])))
        self.spawn_log.append((t, ty, hit[0], hit[1], new))      # (tuple as emitted, its types, list, stored reversed, inserted)

    def match(self, ty):
        """(list index, reversed) of the first registered type tuple that equals `ty` forward or reversed, or None."""
        for k, l in enumerate(self.lists):
            if l["arity"] != len(ty):
                continue
            for reg in l["reg"]:
                if ty == reg or ty[::-1] == reg:
                    return k, ty != reg
        return None

    def _spawn(self, new):
        """new: this step's bonds (role 1, role 2) in canonical order, all linked already; types as the events left them."""
        any3 = any(l["arity"] == 3 and l["reg"] for l in self.lists)
        any4 = any(l["arity"] == 4 and l["reg"] for l in self.lists)
        g = lambda p: sorted(self.graph[p])      # noqa: E731
        for a, b in new:
            if any3:
                for n1 in g(a):
                    if n1 != b:
                        self._spawn_tuple((n1, a, b))
                for m in g(b):
                    if m != a:
                        self._spawn_tuple((a, b, m))
            if any4:
                for n1 in g(a):
                    if n1 == b:
                        continue
                    for n2 in g(n1):
                        if n2 != a and n2 != b:
                            self._spawn_tuple((n2, n1, a, b))
                    for m in g(b):
                        if m != a and m != n1:
                            self._spawn_tuple((n1, a, b, m))
                for m in g(b):
                    if m == a:
                        continue
                    for m2 in g(m):
                        if m2 != b and m2 != a:
                            self._spawn_tuple((a, b, m, m2))

    # ---- chem_reaction_neighbour_change ----
    def _shell(self, root, level):
        """Particles whose graph distance from root is exactly `level`, ascending."""
        seen, front = {root}, [root]
        for _ in range(level):
            nxt = []
            for p in front:
                for x in self.graph[p]:
                    if x not in seen:
                        seen.add(x); nxt.append(x)
            front = nxt
        return sorted(front)

    def _neighbour_changes(self, acc):
        """acc: this step's events in canonical order.  Role 1 before role 2, rules in insertion order; every visit reads the
        types and states as the visits before it left them.  Returns [(tag, rule index)] of the changes."""
        done = []
        for a, b, k, _, _ in acc:
            for role, root in ((1, a), (2, b)):
                for q, rl in enumerate(self.nb_rules):
                    if rl["reaction"] != k or not (rl["invoke_on"] & role):
                        continue
                    for p in self._shell(root, rl["nb_level"]):
                        if self.type[p] != rl["old_type"]:
                            continue
                        w = rl["window"]
                        if w is not None and w[0] < w[1] and not (w[0] <= self.state[p] < w[1]):
                            continue
                        self.type[p] = rl["new_type"]; self.mass[p] = rl["new_mass"]; self.q[p] = rl["new_q"]
                        if rl["set_state"] == 1:
                            self.state[p] = rl["new_state"]
                        elif rl["set_state"] == 2:
                            self.state[p] += rl["new_state"]
                        done.append((p, q))
        return done

    # ---- chem_atrp_init: one firing ----
    def atrp_fire(self, step):
        row, _ = atrp_model(self.type, self.state, self.mass, self.q, self.atrp, step)
        self.atrp_rows.append(row)
        return row

    def snapshot(self):
        snap = dict(bonds=np.asarray(self.bonds, dtype=np.int64).reshape(-1, 2), state=self.state.copy(), type=self.type.copy(),
                    mass=self.mass.copy(), molid=self.ids[self.mol], resid=self.res.copy(),
                    excl=np.asarray(sorted((int(self.ids[a]), int(self.ids[b])) for a, b in self.excl), dtype=np.int64).reshape(-1, 2),
                    charge=self.q.copy(), pad=np.asarray(self.pads, dtype=np.int64), atrp=np.asarray([_atrp_row(r) for r in self.atrp_rows]).reshape(-1, 7))
        for i, l in enumerate(self.lists):
            if l["arity"] > 2:
                snap["list%d" % i] = self.ids[np.asarray(l["ent"], dtype=np.int64).reshape(-1, l["arity"])]
        return snap


_ATRP_COLS = ("step", "candidates", "selected", "activated", "deactivated", "ratio_activator", "ratio_deactivator")


def _atrp_row(r):
    """A stats row as seven doubles (the counts are far below 2^53): compared exactly."""
    return [float(r[k]) for k in _ATRP_COLS]


def engine_snapshot(e, h, spec=None):
    """What Reference.snapshot holds, read back from an engine; spec names the arity-3 / arity-4 lists and whether ATRP runs."""
    snap = dict(bonds=e.get_list(h["reaction_bonds"]), state=e.get_state("STATE"), type=e.get_state("TYPE"), mass=e.get_state("MASS"),
                molid=e.get_state("MOLID"), resid=e.get_state("RESID"), excl=e.get_exclusions(),
                charge=e.get_state("CHARGE"), pad=np.asarray(e.get_events()["pad"], dtype=np.int64))
    rows = e.atrp_stats() if spec is not None and spec.get("atrp") else []
    snap["atrp"] = np.asarray([_atrp_row(r) for r in rows]).reshape(-1, 7)
    for i, l in enumerate((spec or {}).get("lists", [])):
        if l["arity"] > 2:
            snap["list%d" % i] = e.get_list(h[i])
    return snap


def engine_events(ev):
    """Event records of an engine as the reference reports them, r2 compared through its bits."""
    return [(int(e["step"]), int(e["id_a"]), int(e["id_b"]), int(e["reaction"]), float(e["r2"]).hex()) for e in ev]


def ref_events(ev):
    return [(s, a, b, r, float(d2).hex()) for s, a, b, r, d2 in ev]


# ======================================================================================================================
# the zoo
# ======================================================================================================================
def _spec(box, pos, types, reactions, state=None, res_id=None, interval=3, nearest=True, max_per_interval=0, steps=1, vel=None, **kw):
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    L = np.asarray(box, dtype=np.float64)
    reactions = [dict(_RX, **r) for r in reactions]
    spec = dict(box=[float(x) for x in box], rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, n + 1), types=np.asarray(types, dtype=np.int32),
                pos=pos - np.floor(pos / L) * L, mass=np.ones(n), vel=np.zeros((n, 3)) if vel is None else vel,
                state=np.zeros(n, dtype=np.int32) if state is None else np.asarray(state, dtype=np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32) if res_id is None else np.asarray(res_id, dtype=np.int32),
                rebuild_criterion=1, steps=steps,
                reaction=dict(bond=("HARMONIC", [0.0, 1.0]), interval=interval, nearest=nearest, max_per_interval=max_per_interval, seed=77,
                              type_mass={t: 1.0 + 0.5 * t for t in range(16)}, reactions=reactions))
    spec.update(kw)
    return spec


def on_grid(spec):
    q = np.asarray(spec["pos"]) / GRID
    return bool(np.all(q == np.rint(q)))


def snake(n=160, g0=800, x0=20.0, x1=44.0, y0=2.0, z0=3.0):
    """n points; link k has length (g0 - k) / 1024.  Runs along +x from x0 to x1, climbs two links in y, runs back."""
    p, d, up = [np.array([x0, y0, z0])], 1, 0
    for k in range(n - 1):
        g = (g0 - k) * GRID
        q = p[-1].copy()
        if up or (d > 0 and q[0] + g > x1) or (d < 0 and q[0] - g < x0):
            q[1] += g
            if up:
                d = -d
            up = 1 - up
        else:
            q[0] += d * g
        p.append(q)
    return np.array(p)


def lattice_block(k, org, a=0.75):
    g = np.arange(k) * a
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(org, dtype=np.float64)


def _aa(cutoff, wide=False, **kw):
    """A + A on type 0; wide: up to six events per particle (the lattice's coordination), one state step each."""
    r = dict(type_1=0, type_2=0, cutoff=cutoff, **kw)
    if wide:
        r.update(delta_1=1, delta_2=1, max_state_1=6, max_state_2=6, intraresidual=True)      # (res_id merges with the cluster: the molecule flag alone decides)
    return r


CHAIN_CUT = 0.8


def chain(box=(32.0, 32.0, 32.0), cascade=False, intramolecular=False):
    return _spec(box, snake(), np.zeros(160), [_aa(CHAIN_CUT, wide=cascade, intramolecular=intramolecular)], steps=4 if cascade else 1)


BLOCK_CUT, SAT_MIN, SAT_CUT = 0.8125, 0.25, 0.5
SAT_GAPS = (SAT_CUT, SAT_MIN, SAT_MIN - GRID, SAT_CUT - GRID)      # on the cutoff: no; on the minimum: yes; inside it: no; inside the cutoff: yes


def ties(box=(32.0, 32.0, 32.0), k=6, org=(10.0, 10.0, 10.0), sixteen=False, cascade=False, intramolecular=False):
    """The lattice block (type 0, every nearest-neighbour d2 the same bits) and, one lattice step and a quarter beside it, four
    satellite pairs along y.  Plain: reactions 0 and 1 are identical A + A rules (0 must win), reaction 2 is B + B with a
    minimum cutoff on satellites of type 1 whose gaps sit on and beside both radii.  sixteen: 16 reactions; 0 and 15 are A + A
    rules that differ in the state window only, 1 .. 14 name types nobody has; the block (state 0) fits both, satellites of
    type 0 in state 1 fit 15 alone."""
    blk = lattice_block(k, org)
    sx = org[0] + (k - 1) * 0.75 + 1.0
    sat = np.array([[sx, org[1] + dy, org[2] + z] for z, g in enumerate(SAT_GAPS) for dy in (0.0, g)])
    pos = np.concatenate([blk, sat])
    nb, ns = len(blk), len(sat)
    if sixteen:
        rx = [_aa(BLOCK_CUT)] + [dict(type_1=5 + q % 3, type_2=9, cutoff=BLOCK_CUT) for q in range(14)] + [_aa(BLOCK_CUT, max_state_1=2, max_state_2=2)]
        return _spec(box, pos, np.zeros(nb + ns), rx, state=np.concatenate([np.zeros(nb), np.ones(ns)]))
    rx = [_aa(BLOCK_CUT, wide=cascade, intramolecular=intramolecular), _aa(BLOCK_CUT, wide=cascade, intramolecular=intramolecular),
          dict(type_1=1, type_2=1, cutoff=SAT_CUT, min_cutoff=SAT_MIN)]
    return _spec(box, pos, np.concatenate([np.zeros(nb), np.ones(ns)]), rx, steps=4 if cascade else 1)


def roles(box=(32.0, 32.0, 32.0), s=8.0, cascade=False):
    """Isolated pairs on a grid of spacing s (pair gap s / 32 per axis, cutoff s / 16).  A pair whose grid point lies on a face,
    an edge or the corner of the box is laid across it (along (1, 0, 0), (1, 1, 0), (1, 1, 1) and their kin).  Reaction 0:
    type 0 in [2, 5) + type 1 in [0, 1), neither intraresidual nor intramolecular, role 1 becomes type 2 (a new mass), role 2 is
    told to become type 1, which it is (its mass stays); reaction 1: type 4 + type 5, both flags set.  Every pair is written
    with the type_2 particle FIRST (lower tag), so the reversed role assignment decides all of them."""
    gap, cut = s / 32.0, s / 16.0
    m = int(round(box[0] / s))
    slots = [np.array([i, j, k]) * s for i in range(m) for j in range(int(round(box[1] / s))) for k in range(int(round(box[2] / s)))][::-1]
    dirs = [np.array(d, dtype=np.float64) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    pos, typ, st, res, excl, bonds = [], [], [], [], [], []

    def pair(slot, t_lo, t_hi, s_lo=0, s_hi=0, same_res=False, excluded=False, via=None):
        c = slots[slot]
        d = (c == 0).astype(np.float64) if (c == 0).any() else dirs[slot % 3]
        i = len(pos)
        pos.extend([c - 0.5 * gap * d, c + 0.5 * gap * d]); typ.extend([t_lo, t_hi]); st.extend([s_lo, s_hi])
        res.extend([i + 1, i + 1 if same_res else i + 2])
        if excluded:
            excl.append((i + 1, i + 2))
        if via is not None:                              # an inert third particle bonded to both: one molecule, the pair itself not excluded
            pos.append(c + gap * dirs[(slot + 1) % 3]); typ.append(via); st.append(0); res.append(i + 3)
            bonds.extend([(i + 1, i + 3), (i + 2, i + 3)]); excl.extend([(i + 1, i + 3), (i + 2, i + 3)])
    k = 0
    for s1 in (1, 2, 4, 5):                              # min - 1, min, max - 1, max of the role-1 window
        pair(k, 1, 0, 0, s1); k += 1
    for s2 in (-1, 0, 1):                                # the role-2 window [0, 1)
        pair(k, 1, 0, s2, 3); k += 1
    for tl, th in ((1, 0), (5, 4)):                      # each flag value: refused by reaction 0, accepted by reaction 1
        pair(k, tl, th, 0, 3, same_res=True); k += 1
        pair(k, tl, th, 0, 3, via=7); k += 1
    pair(k, 1, 0, 0, 3, excluded=True); k += 1
    while k < len(slots):                                # the rest of the grid: plain reversed pairs
        pair(k, 1, 0, 0, 2 + k % 3); k += 1
    rx = [dict(type_1=0, type_2=1, cutoff=cut, min_state_1=2, max_state_1=5, delta_1=1 if cascade else 3, delta_2=0 if cascade else 1,
               new_type_1=2, new_type_2=1),
          dict(type_1=4, type_2=5, cutoff=cut, min_state_1=2, max_state_1=5, delta_1=3, delta_2=1, intramolecular=True, intraresidual=True)]
    return _spec(box, pos, typ, rx, state=st, res_id=res, exclusions=np.asarray(excl), steps=4 if cascade else 1,
                 lists=[dict(arity=2, kind="HARMONIC", params=[0.0, 1.0], ids=np.asarray(bonds))])


def random_mode(max_per_interval=0):
    """Chain and block together, nearest = False (the priority is the pair hash), prob = 0.5."""
    pos = np.concatenate([snake(), lattice_block(6, (10.0, 10.0, 10.0))])
    rate = 0.5 / (DT * 3)
    return _spec((32.0, 32.0, 32.0), pos, np.zeros(len(pos)), [_aa(BLOCK_CUT, rate=rate)], nearest=False, max_per_interval=max_per_interval)


def cluster(copies=1):
    """The block alone in the 32^3 box; copies = 16: sixteen identical reactions, more candidates than the buffer holds."""
    pos = lattice_block(6, (10.0, 10.0, 10.0))
    return _spec((32.0, 32.0, 32.0), pos, np.zeros(len(pos)), [_aa(BLOCK_CUT) for _ in range(copies)])


def cand_capacity(n):
    return max(8 * n, 1024)


CLOSE_INTERVAL, CLOSE_MARGIN = 10, 0.02
_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]


def closing_pairs(cell_edge=32.0 / 17.0):
    """64 isolated A + B pairs, reaction cutoff = rc, centred on corners of the cell grid nearest to the points of an 8-grid
    (the first index of every axis is the periodic face) and shifted along x by -0.1 .. 0.2, along axes, face diagonals and body
    diagonals: the partners start in different cells, and the scan's x-window, cut on quarter cells, ends between where a partner
    is and where it was binned for some of them.  Closing pairs start at
    rc + 0.9 skin - 0.02 and approach at 0.45 skin per partner in `interval` steps; receding pairs start at rc - 0.9 skin + 0.02
    and leave.  The lower tag is the type_2 particle in every second pair."""
    v = 0.45 * SKIN / (CLOSE_INTERVAL * DT)
    pos, vel, typ, closing = [], [], [], []
    slot = 0
    for i in range(4):
        for j in range(4):
            for k in range(4):
                c = np.rint(np.array([i, j, k]) * 8.0 / cell_edge) * cell_edge
                c[0] += 0.1 * (slot % 4 - 1)      # (the x-window is cut on quarter cells: sample where in a quarter the partner was binned)
                u = np.array(_DIRS[slot % 13], dtype=np.float64)
                u /= np.sqrt(u @ u)
                recede = 13 <= slot < 26
                sep = RC - 0.9 * SKIN + CLOSE_MARGIN if recede else RC + 0.9 * SKIN - CLOSE_MARGIN
                sgn = 1.0 if recede else -1.0
                pos.extend([c - 0.5 * sep * u, c + 0.5 * sep * u]); vel.extend([-sgn * v * u, sgn * v * u])
                typ.extend([slot % 2, 1 - slot % 2]); closing.append(not recede)
                slot += 1
    rx = [dict(type_1=0, type_2=1, cutoff=RC)]
    return _spec((32.0, 32.0, 32.0), pos, typ, rx, interval=CLOSE_INTERVAL, vel=np.asarray(vel), closing=np.asarray(closing))


# ---- members for what hangs onto a reaction: restrict, constraint, neighbour change, spawned tuples, pad, ATRP ----------------
def _blk(ix, iy, iz, k=6):
    """id of the block particle at lattice index (ix, iy, iz) (lattice_block order, ids from 1)."""
    return (ix * k + iy) * k + iz + 1


RESTRICT_X, RESTRICT_SAT = _blk(5, 0, 0), 217      # X's listed partner is a lattice step away, the unlisted satellite (the last id) is nearer


def restrict_lists():
    """(list of reaction 0 / row 0, list of row 15) on the 6^3 block.  List 0: disjoint nearest-neighbour pairs along y, every
    second one written (higher id, lower id); a hub with three listed partners; two pairs 1.5 apart (beyond the cutoff);
    X with its -x neighbour.  List 15 shares some of list 0's pairs and has pairs along z of its own."""
    l0, l15 = [], []
    for ix in range(2, 6):
        for iz in range(6):
            for iy in (0, 2, 4):
                if (ix + iy // 2 + iz) % 3 == 0 and (ix, iy, iz) != (5, 0, 0):
                    p = (_blk(ix, iy, iz), _blk(ix, iy + 1, iz))
                    l0.append(p[::-1] if len(l0) % 2 else p)
                    if iz % 2:
                        l15.append(p)                        # listed for both rows: reaction 0 wins
    hub = _blk(3, 3, 3)
    l0 += [(hub, _blk(4, 3, 3)), (_blk(3, 3, 4), hub), (hub, _blk(3, 3, 2))]
    l0 += [(_blk(2, 0, 0), _blk(2, 0, 2)), (_blk(4, 5, 5), _blk(2, 5, 5))]
    l0.append((RESTRICT_X, _blk(4, 0, 0)))
    for ix in range(2, 6):
        for iy in range(6):
            if (ix + iy) % 2 == 0:
                l15.append((_blk(ix, iy, 5), _blk(ix, iy, 4)))   # listed for row 15 only
    return np.asarray(l0), np.asarray(l15)


def restrict(sixteen=False, restricted=True):
    """The lattice block plus one satellite half a unit beside X = block (5, 0, 0).  Plain: x-layers 0 and 1 are type 1 and react
    through reaction 1, unrestricted; layers 2 .. 5 and the satellite are type 0 and react through reaction 0, restricted to
    restrict_lists()[0].  sixteen: all type 0; rows 0 and 15 are the same A + A rule, restricted to different lists; rows 1 .. 14 name
    types nobody has.  restricted = False: the same system without the lists (what the conditions compare with)."""
    org = (10.0, 10.0, 10.0)
    blk = lattice_block(6, org)
    pos = np.concatenate([blk, [[org[0] + 5 * 0.75 + 0.5, org[1], org[2]]]])
    l0, l15 = restrict_lists()
    if sixteen:
        typ = np.zeros(len(pos))
        rx = [_aa(BLOCK_CUT)] + [dict(type_1=5 + q % 3, type_2=9, cutoff=BLOCK_CUT) for q in range(14)] + [_aa(BLOCK_CUT)]
        ext = dict(restrict=[(0, l0), (15, l15)])
    else:
        typ = np.concatenate([(np.arange(216) // 36 < 2).astype(int), [0]])
        rx = [_aa(BLOCK_CUT), dict(type_1=1, type_2=1, cutoff=BLOCK_CUT)]
        ext = dict(restrict=[(0, l0[:7]), (0, l0[7:])])                    # two calls: they accumulate
    return _spec((32.0, 32.0, 32.0), pos, typ, rx, ext=ext if restricted else {})


class _Cells:
    """Isolated groups of particles on the grid of `roles`: spacing s, reacting partners one gap = s / 32 apart along the cell's
    axis u, cutoff s / 16.  A cell whose grid point lies on a face, an edge or the corner of the box has u = (1, 0, 0), (1, 1, 0),
    (1, 1, 1) or their kin and its offsets 0 and 1 straddle the point; bonded by-standers sit along a second axis v."""

    def __init__(self, box, s, shift=0.0):
        self.box, self.s, self.gap, self.cut, self.shift = box, s, s / 32.0, s / 16.0, shift
        self.slots = [np.array([i, j, k]) * s for i in range(int(round(box[0] / s))) for j in range(int(round(box[1] / s)))
                      for k in range(int(round(box[2] / s)))][::-1]
        self.pos, self.typ, self.st, self.bonds, self.k, self.cellid = [], [], [], [], 0, []

    def cell(self):
        c = self.slots[self.k]
        u = (c == 0).astype(np.float64) if (c == 0).any() else np.eye(3)[self.k % 3]
        v = np.array([1.0, -1.0, 0.0]) if u.sum() == 3 else np.eye(3)[[d for d in range(3) if u[d] == 0][-1]]      # v is orthogonal to u
        self.k += 1
        self.c, self.u, self.v = c - 0.5 * self.gap * u + self.shift, u, v
        return self

    def add(self, ou, ov, typ, state=0, bond=None):
        """A particle at offset ou gaps along u and ov gaps along v; returns its id.  bond: ids it is bonded to from the start."""
        self.pos.append(self.c + self.gap * (ou * self.u + ov * self.v)); self.typ.append(typ); self.st.append(state); self.cellid.append(self.k - 1)
        i = len(self.pos)
        for b in ([] if bond is None else [bond] if isinstance(bond, int) else bond):
            self.bonds.append((b, i))
        return i

    def spec(self, rx, steps=1, **kw):
        b = np.asarray(self.bonds, dtype=np.int64).reshape(-1, 2)
        return _spec(self.box, self.pos, self.typ, rx, state=self.st, exclusions=b, steps=steps,
                     lists=[dict(arity=2, kind="HARMONIC", params=[0.0, 1.0], ids=b)] + kw.pop("lists", []), **kw)


CONS_WIN = (2, 5)
_EDGE_STATES = (CONS_WIN[0] - 1, CONS_WIN[0], CONS_WIN[1] - 1, CONS_WIN[1])


def constraint(box=(32.0, 32.0, 32.0), s=8.0, second_call=True):
    """Isolated pairs, each with bonded by-standers, under neighbour-state constraints (window CONS_WIN on type 6):
    reaction 0: 0 + 1, constraint on role 1;  reaction 1: 2 + 3, constraint on role 2 (set by a SECOND call; the first call names
    role 1);  reaction 2: 4 + 4, role 1;  reaction 3: 5 + 5, role 2.  Every pair is written with the type_2 particle at the lower
    tag.  spec["expect"]: {lower id of the pair: reaction or None}."""
    C, exp = _Cells(box, s), {}
    rx = [dict(type_1=0, type_2=1, cutoff=C.cut), dict(type_1=2, type_2=3, cutoff=C.cut), dict(type_1=4, type_2=4, cutoff=C.cut),
          dict(type_1=5, type_2=5, cutoff=C.cut)]

    def pair(t_lo, t_hi, on_lo=(), on_hi=(), want=None):
        """on_lo / on_hi: (type, state) of the by-standers bonded to the lower / higher tag, in tag order."""
        C.cell()
        lo, hi = C.add(0, 0, t_lo), C.add(1, 0, t_hi)
        for k, (t, st) in enumerate(on_lo):
            C.add(0, 1 + k, t, st, bond=lo)
        for k, (t, st) in enumerate(on_hi):
            C.add(1, -1 - k, t, st, bond=hi)
        exp[lo] = want
    for st in _EDGE_STATES:                                  # the window's edges, on either role
        ok = CONS_WIN[0] <= st < CONS_WIN[1]
        pair(1, 0, on_hi=[(6, st)], want=0 if ok else None)
        pair(3, 2, on_lo=[(6, st)], want=1 if ok else None)
    pair(1, 0, on_hi=[(7, 3)])                               # a neighbour of the wrong type
    pair(1, 0, on_lo=[(6, 3)])                               # the right neighbour, bonded to the other reactant only
    pair(3, 2, on_hi=[(6, 3)])                               # ... which the first call for reaction 1 (role 1) would have accepted
    pair(4, 4, on_lo=[(6, 3)], want=2)                       # both assignments fit: the forward one (lower tag = role 1) is judged
    pair(4, 4, on_hi=[(6, 3)])                               # ... and is not retried reversed
    pair(5, 5, on_hi=[(6, 3)], want=3)
    pair(5, 5, on_lo=[(6, 3)])
    pair(1, 0, on_hi=[(6, 0), (7, 3), (6, 5), (6, 1), (7, 2), (6, 9), (6, 3)], want=0)      # a hub of seven: only the highest tag qualifies
    pair(1, 0, on_hi=[(6, 0), (7, 3), (6, 5), (6, 1), (7, 2), (6, 9), (6, 5)])              # ... and one where none does
    while C.k < len(C.slots):                                # the rest of the grid, faces, edges and the corner among it
        st = _EDGE_STATES[(C.k + 2) % 4]                     # (the corner, the last slot, gets min)
        ok = CONS_WIN[0] <= st < CONS_WIN[1]
        if C.k % 2:
            pair(1, 0, on_hi=[(6, st)], want=0 if ok else None)
        else:
            pair(3, 2, on_lo=[(6, st)], on_hi=[(6, 3)], want=1 if ok else None)
    cons = [(0, 1, 6) + CONS_WIN, (1, 1, 6) + CONS_WIN, (2, 1, 6) + CONS_WIN, (3, 2, 6) + CONS_WIN]
    if second_call:
        cons.append((1, 2, 6) + CONS_WIN)
    return C.spec(rx, ext=dict(constraint=cons), expect=exp)


def constraint_cascade():
    """Three steps.  A (type 0) is bonded to N (type 6) and sits one gap from B (type 1); reaction 0 is A + B with B in state 1 and
    the constraint "A carries a type 6 in CONS_WIN".  B reaches state 1 in step 1 through the virtual reaction 1 with H (type 8),
    so A + B is first tried in step 2, on what step 1 left of N:
      kind 0  N = 3 stays: accepted in step 2 (the control);
      kind 1  N = 3 reacts itself in step 1 (virtual reaction 2 with M, type 9, delta + 5): refused in steps 2 and 3;
      kind 2  N = 3 is bonded to P (type 10); P's virtual reaction 3 with Q (type 11) in step 1 carries a neighbour rule that SETS
              the state of a type 6 to 9 without reading one: refused;
      kind 3  as kind 2 without Q: the control of the rule, accepted in step 2;
      kind 4  N = 0 climbs by 1 per step through the virtual reaction 4 with R (type 12): 1 at the scan of step 2 (refused), 2 at
              the scan of step 3 (accepted)."""
    C, exp = _Cells((32.0, 32.0, 32.0), 8.0), {}
    while C.k < len(C.slots):
        kind = C.k % 5
        C.cell()
        a = C.add(0, 0, 0)
        b = C.add(1, 0, 1)
        C.add(2, 0, 8)
        n = C.add(0, 2, 6, 0 if kind == 4 else 3, bond=a)
        if kind == 1:
            C.add(1, 2, 9)
        if kind in (2, 3):
            p = C.add(0, 4, 10, bond=n)
            if kind == 2:
                C.add(1, 4, 11)
        if kind == 4:
            C.add(1, 2, 12)
        exp[a] = {0: 2, 1: None, 2: None, 3: 2, 4: 3}[kind]
    rx = [dict(type_1=0, type_2=1, cutoff=C.cut, min_state_2=1, max_state_2=2),
          dict(type_1=1, type_2=8, cutoff=C.cut, delta_1=1, delta_2=1, is_virtual=True),
          dict(type_1=6, type_2=9, cutoff=C.cut, min_state_1=3, max_state_1=4, delta_1=5, delta_2=1, is_virtual=True),
          dict(type_1=10, type_2=11, cutoff=C.cut, delta_1=1, delta_2=1, is_virtual=True),
          dict(type_1=6, type_2=12, cutoff=C.cut, max_state_1=2, max_state_2=2, delta_1=1, delta_2=1, is_virtual=True)]
    ext = dict(constraint=[(0, 1, 6) + CONS_WIN],
               nb_change=[dict(reaction=3, invoke_on=1, old_type=6, nb_level=1, new_type=6, new_mass=1.0, set_state=1, new_state=9)])
    return C.spec(rx, steps=3, ext=ext, expect=exp)


def exchange():
    """A:B + C -> A:C + B as the reference's set-up builds it: a virtual A + C reaction, the constraint "A carries a B in [0, 2)",
    and a neighbour rule on role 1 that retypes that B with incr_state 1 inside the same window.  Reaction 0 keeps B's type
    (0 + 1, B = 2), so a B in state 0 serves two exchanges; reaction 1 (4 + 5, B = 6 -> 7) serves one.  B starts in -1, 0, 1, 2."""
    C, exp = _Cells((32.0, 32.0, 32.0), 8.0), {}
    while C.k < 44:
        fam, st = C.k % 2, (-1, 0, 1, 2)[(C.k // 2) % 4]
        C.cell()
        c = C.add(0, 0, 5 if fam else 1)                     # C first: the lower tag holds role 2
        a = C.add(1, 0, 4 if fam else 0)
        C.add(1, 2, 6 if fam else 2, st, bond=a)
        exp[c] = (1 if st in (0, 1) else 0) if fam else max(0, min(2, 2 - st)) if st >= 0 else 0      # number of exchanges in three steps
    rx = [dict(type_1=0, type_2=1, cutoff=C.cut, is_virtual=True), dict(type_1=4, type_2=5, cutoff=C.cut, is_virtual=True)]
    ext = dict(constraint=[(0, 1, 2, 0, 2), (1, 1, 6, 0, 2)],
               nb_change=[dict(reaction=0, invoke_on=1, old_type=2, nb_level=1, new_type=2, new_mass=1.0, set_state=2, new_state=1, window=(0, 2)),
                          dict(reaction=1, invoke_on=1, old_type=6, nb_level=1, new_type=7, new_mass=4.5, new_q=0.25, set_state=2, new_state=1, window=(0, 2))])
    return C.spec(rx, steps=3, ext=ext, expect=exp)


NB_WIN = (2, 5)


def nbchange(box=(32.0, 32.0, 32.0), s=8.0, typed=False):
    """Two steps.  Reaction 0 bonds A (0) + B (1) in step 1; reaction 1, virtual, is P (2, state 1) + Q (3) and fires in step 2
    alone, a step without a new bond.  Pre-bonded tails hang on A (t1 t2 t3) and B (s1 s2 s3).  Rules, in this order:
      0  reaction 0, role 1, level 1, X (4) -> Y (5), state kept            1  reaction 0, role 1, level 1, Y -> Z (6), state = 7
         (chained: an X ends as Z because rule 0 comes first)
      2  reaction 0, role 2, level 2, W (7) -> 8, state += 1 inside NB_WIN (s2 starts at min - 1, min, max - 1, max)
      3  reaction 0, both roles, level 3, K (9) -> 10 (t3 from A and s3 from B; t2 and s2, three bonds from the other root, are no K)
      4  reaction 0, role 1, level 1, S (12) -> 12, state += 1 inside [0, 2): an S bonded to the A of TWO events climbs to 2
      5  reaction 0, role 1, level 4, G (13) -> 14       6  reaction 0, role 1, level 2, G -> 15
         (the six-ring r0 .. r5 closed by r0 + r5: r2 is two bonds from r0 one way and four the other, r4 two through the new bond;
          no particle of a six-ring is four bonds away, so rule 5, although it comes first, finds nothing)
      7  reaction 0, role 2, level 1, T (11) -> P, state = 1: makes the reactant of step 2
      8  reaction 1, both roles, level 2, A -> Z, state += 10: from P = s1 through B and the bond of step 1 (Q has no bonds).
    A t1 of type Z stands for the old_type mismatch.  spec["kinds"]: {id of A or r0: kind}.
    typed: the bonds that exist from the start are also held by a by-types harmonic list (created by the tests' set-up helper) with
    parameters for every type pair that occurs, so every retyping re-resolves slots; the reaction bonds get parameters as well,
    masses are HEAVY times the type factor and no coordinate is 0: the variant serves the force comparison."""
    C, kinds = _Cells(box, s, GRID if typed else 0.0), {}
    M = HEAVY if typed else 1.0
    while C.k < len(C.slots):
        m = C.k
        C.cell()
        if m % 8 == 5:                                       # the ring: a pre-bonded chain r0 .. r5 whose ends react
            r0 = C.add(0, 0, 0)
            prev = r0
            for (ou, ov), t in zip(((0, -2), (0, -4), (1, -4), (1, -2)), (4, 13, 9, 13)):
                prev = C.add(ou, ov, t, bond=prev)
            C.add(1, 0, 1, bond=prev)
            kinds[r0] = "ring"
        elif m % 8 == 2:                                     # two events around one S
            a1 = C.add(0, 0, 0)
            C.add(1, 0, 1)
            a2 = C.add(0, 4, 0)
            C.add(1, 4, 1)
            C.add(0, 2, 12, bond=[a1, a2])
            kinds[a1] = "shared"
        else:
            a = C.add(0, 0, 0)
            b = C.add(1, 0, 1)
            t = C.add(0, -2, 6 if m % 4 == 3 else 4, bond=a)
            t = C.add(0, -4, 7, 3, bond=t)
            C.add(0, -6, 9, bond=t)
            q = m % 2 == 0
            t = C.add(1, 2, 11 if q else 6, bond=b)
            t = C.add(1, 4, 7, _EDGE_STATES[(m // 2) % 4], bond=t)
            C.add(1, 6, 9, bond=t)
            if q:
                C.add(2, 2, 3)
            kinds[a] = "chain"
    rx = [dict(type_1=0, type_2=1, cutoff=C.cut, delta_1=1, delta_2=1, intramolecular=True),
          dict(type_1=2, type_2=3, cutoff=C.cut, min_state_1=1, max_state_1=2, delta_1=1, delta_2=1, is_virtual=True)]

    def rule(reaction, invoke_on, level, old, new, **kw):
        return dict(reaction=reaction, invoke_on=invoke_on, nb_level=level, old_type=old, new_type=new, new_mass=M * (1.0 + 0.5 * new), **kw)
    nb = [rule(0, 1, 1, 4, 5), rule(0, 1, 1, 5, 6, set_state=1, new_state=7, new_q=0.125),
          rule(0, 2, 2, 7, 8, set_state=2, new_state=1, window=NB_WIN), rule(0, 3, 3, 9, 10, new_q=-0.5),
          rule(0, 1, 1, 12, 12, set_state=2, new_state=1, window=(0, 2)), rule(0, 1, 4, 13, 14), rule(0, 1, 2, 13, 15),
          rule(0, 2, 1, 11, 2, set_state=1, new_state=1), rule(1, 3, 2, 0, 6, set_state=2, new_state=10)]
    spec = C.spec(rx, steps=2, ext=dict(nb_change=nb), kinds=kinds, cell=np.asarray(C.cellid))
    if typed:
        spec["mass"] = M * np.ones(len(spec["ids"]))
        spec["reaction"]["type_mass"] = {t: M * (1.0 + 0.5 * t) for t in range(16)}
        spec["reaction"]["bond"] = ("HARMONIC", [2.0, 0.2])
        ref, b, pairs = Reference(spec), spec["lists"][0]["ids"], set()
        for k in range(3):                                   # the type pairs the bonds show at the start and after either step
            pairs |= {tuple(sorted((int(ref.type[i - 1]), int(ref.type[j - 1])))) for i, j in b.tolist()}
            if k < 2:
                ref.step(3 * (k + 1))
        spec["ext"]["typed_lists"] = [dict(arity=2, kind="HARMONIC", ids=b, typed=[(tp, [1.0 + 0.25 * tp[0] + 0.125 * tp[1], 0.2 + 0.01 * (tp[1] - tp[0])])
                                                                                   for tp in sorted(pairs)])]
    return spec


HEAVY = 2.0 ** 80      # masses of the members that carry bonded forces: nothing moves (dt^2 f / m is 1e-30 of a grid step)
SPAWN_REG = {1: [(2, 1, 4), (4, 1, 1), (5, 4, 1), (7, 4, 1)], 2: [(4, 1, 1), (2, 4, 1), (6, 4, 1), (7, 1, 4), (4, 1, 3)],
             3: [(4, 1, 1, 4), (5, 4, 1, 1), (7, 7, 4, 1), (7, 7, 1, 4)], 4: [(4, 1, 1, 4), (2, 4, 1, 1), (6, 4, 1, 1), (7, 4, 1, 7), (3, 1, 1, 4)]}
_LINE = ((-1, 0, 1), (0, 0, 0), (1, 1, 0), (2, 1, 1), (3, 0, 1), (4, 1, 2), (1, 2, -1))       # c0 .. c5 and the branch beside c2
_RING = ((0, 0, 0), (1, -1, -2), (-2, 2, -2), (0, 2, 3), (3, -1, 2), (1, 1, 0))                # r0 .. r5


def spawn():
    """Three steps of chain growth with spawned angles and dihedrals on two lists per arity (handles 1, 2 and 3, 4; SPAWN_REG).
    Reaction 0: 0 + 1, role 1 becomes type 4; reaction 1: 1 + 1, both in state 1; reaction 2: 1 in state 2 + 3.  A neighbour
    rule of reaction 0 retypes a type-2 neighbour of role 1 to 5, after the step's tuples were spawned.  Kinds of cell:
      line   c0-c1  c2  c3  c4-c5, br beside c2 (types 2|6 0 1 1 0 2, br 3).  Step 1: c1-c2 and c4-c3; step 2: c2-c3; step 3: c2-br.
      flank  as line with c2-c3 and c2-x bonded from the start (x = type 2 at br's place): both bonds of step 1 find (c1 c2 c3 c4).
      ring   r0 .. r5 bonded in a row (types 0 7 7 7 7 1), closed by r0 + r5 in step 1.
    Adjacent members are gap * sqrt(2) apart, inside the cutoff 2 gap; every other pair that could react is beyond it.  Masses
    are HEAVY times the type factor, the bonded parameters are not zero: the member also serves the force comparison."""
    box, s = (32.0, 32.0, 32.0), 8.0
    gap, cut = s / 32.0, s / 16.0
    slots = [np.array([i, j, k]) * s for i in range(4) for j in range(4) for k in range(4)][::-1]
    pos, typ, bonds, kinds, cell = [], [], [], {}, []
    for m, c in enumerate(slots):
        ax = np.eye(3)[[m % 3, (m + 1) % 3, (m + 2) % 3]]
        at = lambda o: c + GRID + gap * (np.asarray(o, dtype=np.float64) @ ax)      # noqa: E731  (one grid step off the planes: no coordinate is 0, where 1e-30 would show)
        i0 = len(pos) + 1
        if m % 4 == 3:
            pos += [at(o) for o in _RING]; typ += [0, 7, 7, 7, 7, 1]
            bonds += [(i0 + k, i0 + k + 1) for k in range(5)]
            kinds[i0] = "ring"
        else:
            flank = m % 4 == 1
            pos += [at(o) for o in _LINE]; typ += [6 if m % 8 == 0 else 2, 0, 1, 1, 0, 2, 2 if flank else 3]
            bonds += [(i0, i0 + 1), (i0 + 4, i0 + 5)] + ([(i0 + 2, i0 + 3), (i0 + 2, i0 + 6)] if flank else [])
            kinds[i0] = "flank" if flank else "line"
        cell += [m] * (len(pos) - len(cell))
    b = np.asarray(bonds, dtype=np.int64)
    lists = [dict(arity=2, kind="HARMONIC", params=[3.0, 0.3], ids=b),
             dict(arity=3, kind="ANG_HARMONIC", params=[5.0, 1.9], ids=np.zeros((0, 3), dtype=np.int64), register=SPAWN_REG[1]),
             dict(arity=3, kind="ANG_HARMONIC", params=[7.0, 2.1], ids=np.zeros((0, 3), dtype=np.int64), register=SPAWN_REG[2]),
             dict(arity=4, kind="DIH_NCOS", params=[1.5, 0.4, 2.0], ids=np.zeros((0, 4), dtype=np.int64), register=SPAWN_REG[3]),
             dict(arity=4, kind="DIH_NCOS", params=[2.5, -0.7, 3.0], ids=np.zeros((0, 4), dtype=np.int64), register=SPAWN_REG[4])]
    rx = [dict(type_1=0, type_2=1, cutoff=cut, delta_1=1, delta_2=1, new_type_1=4, intramolecular=True),
          dict(type_1=1, type_2=1, cutoff=cut, min_state_1=1, max_state_1=2, min_state_2=1, max_state_2=2, delta_1=1, delta_2=1, intramolecular=True),
          dict(type_1=1, type_2=3, cutoff=cut, min_state_1=2, max_state_1=3, delta_1=1, delta_2=1)]
    nb = [dict(reaction=0, invoke_on=1, nb_level=1, old_type=2, new_type=5, new_mass=HEAVY * 3.5)]
    spec = _spec(box, pos, typ, rx, exclusions=b, steps=3, lists=lists, ext=dict(nb_change=nb), kinds=kinds, cell=np.asarray(cell))
    spec["mass"] = HEAVY * (1.0 + 0.5 * np.asarray(typ, dtype=np.float64))
    spec["reaction"]["type_mass"] = {t: HEAVY * (1.0 + 0.5 * t) for t in range(16)}
    spec["reaction"]["bond"] = ("HARMONIC", [2.0, 0.2])
    return spec


def atrp(select_from_all=True):
    """Twelve run(1) calls; the reaction step falls on every third step, the ATRP firing on every second, both on 6 and 12.
    A cell is a dormant chain end (type 2) and three monomers (type 1) in a row, one gap apart.  The activator turns a dormant
    end (2, state 0) into an active one (type 0, charge 0.25) and back; reaction 0 bonds an active end to the next monomer,
    which becomes the active end (new_type_2 = 0) while a neighbour rule retypes the old end to 3.  Of a pool of 256 (all) or at
    most 64 (centres) 40 are selected per firing; delta_catalyst = 8 moves 0.2 per flip, so the third activation in a row takes what is
    left of the activator's share (0.55 - 2 * 0.2) and leaves exactly 0: the clamp."""
    C = _Cells((32.0, 32.0, 32.0), 8.0)
    while C.k < len(C.slots):
        C.cell()
        for k in range(4):
            C.add(k, 0, 2 if k == 0 else 1)
    rx = [dict(type_1=0, type_2=1, cutoff=C.cut, delta_1=1, new_type_2=0, new_q_2=0.25)]
    nb = [dict(reaction=0, invoke_on=2, nb_level=1, old_type=0, new_type=3, new_mass=2.5, new_q=-0.125)]
    at = dict(interval=2, num_particles=40, ratio_activator=0.55, ratio_deactivator=0.45, delta_catalyst=8.0, k_activate=0.9, k_deactivate=0.8,
              select_from_all=select_from_all, seed=4242,
              centers=[dict(type_id=2, state=0, is_activator=False, new_type=0, new_mass=1.0, new_q=0.25),
                       dict(type_id=0, state=0, is_activator=True, new_type=2, new_mass=2.0, new_q=0.0)])
    return C.spec(rx, steps=12, run_each=1, ext=dict(nb_change=nb), atrp=at)


def intra_flag(on=True):
    """cascade_ties_intra with the option count_intra_inter: ring closures inside the growing block carry pad = 1."""
    return dict(ties(cascade=True, intramolecular=True), ext=dict(options=dict(count_intra_inter=1 if on else 0)))


ZOO = {
    "chain": chain, "chain_aniso": lambda: chain(box=(32.0, 16.0, 64.0)),
    "ties": ties, "ties16": lambda: ties(sixteen=True), "roles": roles,
    "cascade_chain": lambda: chain(cascade=True), "cascade_chain_intra": lambda: chain(cascade=True, intramolecular=True),
    "cascade_ties": lambda: ties(cascade=True), "cascade_ties_intra": lambda: ties(cascade=True, intramolecular=True),
    "cascade_roles": lambda: roles(cascade=True),
    "random": random_mode, "random_max7": lambda: random_mode(7), "cluster": cluster,
}
NEW = {        # what hangs onto a reaction (part of ZOO; named apart so that tests can address them)
    "restrict": restrict, "restrict16": lambda: restrict(sixteen=True), "constraint": constraint, "constraint_cascade": constraint_cascade,
    "exchange": exchange, "intra_flag": intra_flag, "nbchange": nbchange, "spawn": spawn,
    "atrp": atrp, "atrp_centres": lambda: atrp(select_from_all=False), "nbchange_typed": lambda: nbchange(typed=True),
}
ZOO.update(NEW)
SMALL = {      # under three cells per axis: the brute-force list
    "ties_4": lambda: ties(box=(4.0, 4.0, 4.0), k=4, org=(0.0, 0.0, 0.0)),
    "roles_4": lambda: roles(box=(4.0, 4.0, 4.0), s=1.0),
    "constraint_4": lambda: constraint(box=(4.0, 4.0, 4.0), s=1.0),
    "nbchange_4": lambda: nbchange(box=(4.0, 4.0, 4.0), s=1.0),
}
_CACHE = {}


def member(name):
    """(spec, per-step [(events, info, snapshot)]) of a static member, computed once."""
    if name not in _CACHE:
        spec = (ZOO.get(name) or SMALL[name])()
        ref = Reference(spec)
        out = []
        iv = spec["reaction"]["interval"]
        each = spec.get("run_each", iv)          # MD steps per run() call; spec["steps"] counts the calls
        for k in range(1, spec["steps"] + 1):
            ev, info = ref.step(k * each, model=True) if (k * each) % iv == 0 else ([], {})
            if ref.atrp is not None and (k * each) % ref.atrp["interval"] == 0:      # behind the reaction step where both fall on one step
                info["atrp"] = ref.atrp_fire(k * each)
            out.append((ev, info, ref.snapshot()))
        _CACHE[name] = (spec, out)
    return _CACHE[name]
