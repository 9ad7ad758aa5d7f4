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


def dist2(L, xi, xj):
    """|minimum image of xi - xj|^2 for one xi against rows xj, unfused, in the header's order."""
    d = xi - xj
    d = d - L * np.rint(d * (1.0 / L))
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return (xx + yy) + zz


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
        for l in spec.get("lists", []):          # bonds that exist from the start: graph and cluster labels, no exclusion of their own
            assert l["arity"] == 2
            pre = [(tag[int(a)], tag[int(b)]) for a, b in np.asarray(l["ids"]).reshape(-1, 2)]
            for a, b in pre:
                self._link(a, b)
            self._relabel(pre, res=False)
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
        self.bonds, self.events = [], []

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
            if not R["is_virtual"]:
                self.bonds.append((int(self.ids[a]), int(self.ids[b])))
                self.excl.add((min(a, b), max(a, b)))
                self._link(a, b); new.append((a, b))
        self._relabel(new)
        self.events += ev
        return ev, info

    def snapshot(self):
        return dict(bonds=np.asarray(self.bonds, dtype=np.int64).reshape(-1, 2), state=self.state.copy(), type=self.type.copy(),
                    mass=self.mass.copy(), molid=self.ids[self.mol], resid=self.res.copy(),
                    excl=np.asarray(sorted((int(self.ids[a]), int(self.ids[b])) for a, b in self.excl), dtype=np.int64).reshape(-1, 2))


def engine_snapshot(e, h):
    return dict(bonds=e.get_list(h["reaction_bonds"]), state=e.get_state("STATE"), type=e.get_state("TYPE"), mass=e.get_state("MASS"),
                molid=e.get_state("MOLID"), resid=e.get_state("RESID"), excl=e.get_exclusions())


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


ZOO = {
    "chain": chain, "chain_aniso": lambda: chain(box=(32.0, 16.0, 64.0)),
    "ties": ties, "ties16": lambda: ties(sixteen=True), "roles": roles,
    "cascade_chain": lambda: chain(cascade=True), "cascade_chain_intra": lambda: chain(cascade=True, intramolecular=True),
    "cascade_ties": lambda: ties(cascade=True), "cascade_ties_intra": lambda: ties(cascade=True, intramolecular=True),
    "cascade_roles": lambda: roles(cascade=True),
    "random": random_mode, "random_max7": lambda: random_mode(7), "cluster": cluster,
}
SMALL = {      # under three cells per axis: the brute-force list
    "ties_4": lambda: ties(box=(4.0, 4.0, 4.0), k=4, org=(0.0, 0.0, 0.0)),
    "roles_4": lambda: roles(box=(4.0, 4.0, 4.0), s=1.0),
}
_CACHE = {}


def member(name):
    """(spec, per-step [(events, info, snapshot)]) of a static member, computed once."""
    if name not in _CACHE:
        spec = (ZOO.get(name) or SMALL[name])()
        ref = Reference(spec)
        out = []
        for k in range(1, spec["steps"] + 1):
            ev, info = ref.step(k * spec["reaction"]["interval"], model=True)
            out.append((ev, info, ref.snapshot()))
        _CACHE[name] = (spec, out)
    return _CACHE[name]
