"""Dissociation reactions on the HIP path (chem_dissociation_add; rule set in include/chem_mi355.h).

The CPU oracle has no bond removal, so the rule set is restated here in a few lines of numpy (`predict`: a distance, a
state window, one Philox draw per bond) and everything AFTER a break -- forces, energies, trajectory -- is checked against
an oracle built from the read-back configuration and the reduced topology.

Sizes: 2000 particles as 1000 dimers in a cubic box of edge 14 (rc 2.5 + skin 0.3: five cells per axis, the smallest grid
the LDS tiles take; 1000 flat entries = four workgroups of the scan with a partial last wave).  Dimer centres sit on a
jittered 10^3 lattice whose first layer lies 0.15 behind the low face of every axis and the dimers point along body
diagonals, so bonds cross the periodic boundary of every axis (their far ends fold to within 0.3 of the high faces) as well
as cell and tile borders.  LJ sigma is 0.4 so that no two particles of neighbouring molecules sit on the repulsive wall.

Tolerances are those of tests/test_gpu_parity.py for bonded systems: forces 1e-10 (fp64) / 5e-5 (fp32, TOL_STIFF32) of the
largest force, list energies 1e-11 / 1e-5, LJ energy 1e-11 / 2e-6, fp64 trajectory 1e-9 of the largest coordinate."""
import numpy as np
import pytest

from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError, Engine
from conftest import rel_err
from test_philox import philox_py

pytestmark = pytest.mark.gpu

BOX, RC, SKIN, DT = 14.0, 2.5, 0.3, 1e-4
K_BOND, R0 = 30.0, 1.0
SEED = 0x1234567887654321
TOL_F = {64: 1e-10, 32: 5e-5}
TOL_EL = {64: 1e-11, 32: 1e-5}
TOL_ELJ = {64: 1e-11, 32: 2e-6}
LJ = [(a, b, 1.0, 0.4, RC) for a in range(3) for b in range(a, 3)]


# ---- systems ---------------------------------------------------------------------------------------------------------------

def lattice(nside, box, rng, keep=None):
    g = np.arange(nside)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if keep is not None:
        sites = sites[keep(sites)]
    return sites * (box / nside) + 0.15 + rng.uniform(-0.05, 0.05, sites.shape)


def diagonals(rng, m):
    return rng.choice([-1.0, 1.0], (m, 3)) / np.sqrt(3.0)


def make_spec(pos, types, bonds, box=BOX, state=None, extra_lists=(), exclusions=None, split_lists=False):
    n = len(pos)
    bonds = np.asarray(bonds, dtype=np.int64)
    if split_lists:     # two harmonic lists of different K: more than one parameter slot, i.e. the work-list kernel
        half = len(bonds) // 2
        lists = [dict(arity=2, kind="HARMONIC", params=[K_BOND, R0], ids=bonds[:half]),
                 dict(arity=2, kind="HARMONIC", params=[20.0, R0], ids=bonds[half:])]
    else:
        lists = [dict(arity=2, kind="HARMONIC", params=[K_BOND, R0], ids=bonds)]
    return dict(n=n, box=[box] * 3, rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, n + 1), types=np.asarray(types, np.int32), pos=pos,
                vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32) if state is None else np.asarray(state, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), lj=LJ, kT=1.0, gamma=0.0, seed=1, rebuild_criterion=1,
                lists=lists + list(extra_lists), exclusions=bonds if exclusions is None else exclusions)


def dimers(lengths, box=BOX, nside=10, seed=7, keep=None):
    """Dimer k = particles 2k+1 (type 0), 2k+2 (type 1); every third list entry is stored (type 1, type 0)."""
    rng = np.random.default_rng(seed)
    c = lattice(nside, box, rng, keep)[:len(lengths)]
    m = len(c)
    assert m == len(lengths)
    d, h = diagonals(rng, m), 0.5 * np.asarray(lengths, dtype=np.float64)[:, None]
    pos = np.empty((2 * m, 3))
    pos[0::2], pos[1::2] = c - h * d, c + h * d
    ids = np.arange(1, 2 * m + 1)
    bonds = np.stack([ids[0::2], ids[1::2]], 1)
    bonds[2::3] = bonds[2::3, ::-1].copy()
    return pos, np.tile([0, 1], m), bonds


def bent_trimers_and_hubs(seed=11):
    """Even-sum sites of a 7^3 lattice (spacing 2): bent trimers a(0)-b(1)-c(0) whose bonds a-b, c-b are (1.3, 0.9),
    (0.9, 0.9), (1.3, 1.3), (1.3, 1.3) long in turn; the last 12 sites carry hubs -- a type-1 centre with five type-0
    partners along the axes (three at 1.3, two at 0.9)."""
    rng = np.random.default_rng(seed)
    c = lattice(7, BOX, rng, keep=lambda s: s.sum(1) % 2 == 0)
    nhub = 12
    ntri = len(c) - nhub
    pos, types, bonds, kinds = [], [], [], []
    for k in range(ntri):
        d1 = diagonals(rng, 1)[0]
        d2 = d1.copy(); d2[rng.integers(3)] *= -1.0
        l1, l2 = [(1.3, 0.9), (0.9, 0.9), (1.3, 1.3), (1.3, 1.3)][k % 4]
        i0 = len(pos) + 1
        pos += [c[k] - l1 * d1, c[k], c[k] + l2 * d2]; types += [0, 1, 0]
        bonds += [(i0, i0 + 1), (i0 + 2, i0 + 1)]; kinds.append(("trimer", i0))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float64)
    for k in range(ntri, ntri + nhub):
        i0 = len(pos) + 1
        pos.append(c[k]); types.append(1)
        for j in range(5):
            pos.append(c[k] + (1.3 if j in (0, 2, 4) else 0.9) * axes[j]); types.append(0)
            bonds.append((i0, i0 + 1 + j) if j % 2 else (i0 + 1 + j, i0))
        kinds.append(("hub", i0))
    return np.array(pos), np.array(types), np.array(bonds), kinds


# ---- the rule set, restated ------------------------------------------------------------------------------------------------

def u01(x):
    return (x + 0.5) * (1.0 / 4294967296.0)


def predict(pos, box, types, states, bond_lists, rxs, step, seed=SEED, dt=DT, interval=1):
    """rxs: dicts(index, list, type_1, type_2, w1, w2, cutoff, diss_rate).  Returns events [(id_a, id_b, index, r2)] and the
    surviving lists."""
    events, left = [], []
    for li, bonds in enumerate(bond_lists):
        keep = []
        for a, b in np.asarray(bonds).tolist():
            ta, tb = a - 1, b - 1
            d = pos[ta] - pos[tb]
            d = d - box * np.rint(d / box)
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            broke = False
            for rx in rxs:
                if rx["list"] != li:
                    continue
                fwd = types[ta] == rx["type_1"] and types[tb] == rx["type_2"]
                rev = types[tb] == rx["type_1"] and types[ta] == rx["type_2"]
                if not (fwd or rev):
                    continue
                p1, p2 = (ta, tb) if (ta < tb if fwd and rev else fwd) else (tb, ta)
                if not (rx["w1"][0] <= states[p1] < rx["w1"][1] and rx["w2"][0] <= states[p2] < rx["w2"][1]):
                    continue
                brk = rx["cutoff"] > 0 and r2 >= rx["cutoff"] * rx["cutoff"]
                p = rx["diss_rate"] * dt * interval
                if not brk and p > 0:
                    lo, hi = min(ta, tb), max(ta, tb)
                    out = philox_py((lo, hi, step & 0xffffffff, ((rx["index"] << 24) ^ (step >> 32)) & 0xffffffff),
                                    ((seed & 0xffffffff) ^ 0x44495353, seed >> 32))
                    brk = u01(out[0]) < p
                if brk:
                    events.append((p1 + 1, p2 + 1, rx["index"], r2)); broke = True
                    break
            if not broke:
                keep.append((a, b))
        left.append(keep)
    return events, left


def clusters(n, bond_lists):
    """lowest id of every bonded cluster, by id"""
    parent = list(range(n + 1))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for bonds in bond_lists:
        for a, b in bonds:
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(1, n + 1)])


def event_rows(eng):
    ev = eng.get_events()
    assert np.all(ev["pad"] == 0)
    return [(int(e["step"]), int(e["id_a"]), int(e["id_b"]), int(e["reaction"])) for e in ev], ev["r2"]


def canonical(events, step):
    return sorted(((step, a, b, r) for a, b, r, _ in events), key=lambda e: (min(e[1], e[2]), max(e[1], e[2])))


RX = dict(type_1=0, type_2=1, delta_1=1, delta_2=2, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1)


def rx_row(index, li, cutoff, diss_rate, **kw):
    d = dict(RX, **kw)
    return dict(index=index, list=li, type_1=d["type_1"], type_2=d["type_2"], w1=(d["min_state_1"], d["max_state_1"]),
                w2=(d["min_state_2"], d["max_state_2"]), cutoff=cutoff, diss_rate=diss_rate)


def build(spec, prec, diss=(), seed=SEED, interval=1):
    """diss: (list index, cutoff, diss_rate, extra keywords) per dissociation reaction; the reaction extension is
    initialised and connected even where nothing is registered.  Returns engine, handles, indices."""
    g = Engine(device=0, precision=prec)
    h = W.apply(spec, g, thermostat=False, reactions=False)
    idx = []
    g.reaction_init(interval, True, 0, seed)
    for li, cutoff, rate, kw in diss:
        idx.append(g.dissociation_add(diss_rate=rate, cutoff=cutoff, bond_list=h[li], **dict(RX, **kw)))
    g.reactions_enable(True)
    return g, h, idx


def oracle_after(make_oracle, spec, g, h):
    """Oracle on the configuration and the topology the engine reads back."""
    o = make_oracle()
    s2 = dict(spec, pos=g.get_state("POS"), vel=g.get_state("VEL"), types=g.get_state("TYPE"), state=g.get_state("STATE"),
              mass=g.get_state("MASS"), exclusions=g.get_exclusions(),
              lists=[dict(l, ids=g.get_list(h[i])) for i, l in enumerate(spec["lists"])])
    W.apply(s2, o, thermostat=False, reactions=False)
    return o


def compare_forces(g, o, prec):
    g.run(0); o.run(0)
    fg, fo = g.get_state("FORCE"), o.get_state("FORCE")
    print("force rel err %.3e (prec %d)" % (rel_err(fg, fo), prec))
    assert rel_err(fg, fo) < TOL_F[prec]
    og, oo = g.observe(), o.observe()
    assert og["list_size"] == oo["list_size"]
    for a, b in zip(og["epot_list"], oo["epot_list"]):
        assert a == pytest.approx(b, rel=TOL_EL[prec], abs=1e-12)
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=TOL_ELJ[prec])
    return fg


# ---- 1, 4, 5: the distance rule on the base system; forces and trajectory afterwards ---------------------------------------

LENGTHS = np.where(np.arange(1000) % 2 == 0, 0.9, 1.3)


@pytest.fixture(scope="module")
def base():
    """The base system after run(1) with cutoff = 1.1, diss_rate = 0, in both precisions (shared, read-only)."""
    pos, types, bonds = dimers(LENGTHS)
    spec = make_spec(pos, types, bonds)
    out = {"spec": spec, "bonds": bonds}
    for prec in (64, 32):
        g, h, idx = build(spec, prec, [(0, 1.1, 0.0, dict(new_type_1=2, new_mass_1=1.5))])
        g.run(1)
        out[prec] = (g, h, idx)
    yield out
    for prec in (64, 32):
        out[prec][0].close()


@pytest.mark.parametrize("prec", [64, 32])
def test_distance_rule(base, prec):
    g, h, idx = base[prec]
    spec, bonds = base["spec"], base["bonds"]
    n = spec["n"]
    x = g.get_state("POS")
    want_ev, left = predict(x, BOX, spec["types"], spec["state"], [bonds], [rx_row(idx[0], 0, 1.1, 0.0)], step=1)
    assert len(want_ev) == 500 and {min(a, b) for a, b, _, _ in want_ev} == set(range(3, n + 1, 4))     # exactly the long bonds
    got, r2 = event_rows(g)
    assert got == canonical(want_ev, 1)
    assert all(spec["types"][a - 1] == 0 and spec["types"][b - 1] == 1 for _, a, b, _ in got)           # roles
    want_r2 = {(a, b): r for a, b, _, r in want_ev}
    err = max(abs(r - want_r2[(e[1], e[2])]) / want_r2[(e[1], e[2])] for e, r in zip(got, r2))
    print("r2 rel err %.3e" % err)
    assert err < 1e-12
    state, ty, mass = spec["state"].copy(), spec["types"].copy(), spec["mass"].copy()
    for a, b, _, _ in want_ev:
        state[a - 1] += 1; state[b - 1] += 2; ty[a - 1] = 2; mass[a - 1] = 1.5
    assert np.array_equal(g.get_list(h[0]), np.array(left[0]))
    assert np.array_equal(g.get_exclusions(), np.array(sorted((min(p), max(p)) for p in left[0])))
    assert np.array_equal(g.get_state("STATE"), state)
    assert np.array_equal(g.get_state("TYPE"), ty)
    assert np.array_equal(g.get_state("MASS"), mass)
    assert np.array_equal(g.get_state("MOLID"), clusters(n, left))
    assert g.observe()["list_size"] == [500]


def test_distance_rule_same_events_in_both_precisions(base):
    assert event_rows(base[64][0])[0] == event_rows(base[32][0])[0]


@pytest.mark.parametrize("prec", [64, 32])
def test_forces_after_a_break_inline_bonds(base, make_oracle, prec):
    g, h, _ = base[prec]
    o = oracle_after(make_oracle, base["spec"], g, h)
    fg = compare_forces(g, o, prec)
    assert np.abs(fg).max() > 1.0


def test_trajectory_after_a_break(base, make_oracle):
    g, h, _ = build(base["spec"], 64, [(0, 1.1, 0.0, dict(new_type_1=2, new_mass_1=1.5))])      # (the shared engines stay as they are)
    g.run(1)
    assert len(g.get_events()) == 500
    o = oracle_after(make_oracle, base["spec"], g, h)
    g.reactions_enable(False)
    g.run(40); o.run(40)
    xg, xo = g.get_state("POS"), o.get_state("POS")
    d = xg - xo
    d -= BOX * np.rint(d / BOX)
    print("trajectory err %.3e" % (np.abs(d).max() / np.abs(xo).max()))
    assert np.abs(d).max() / np.abs(xo).max() < 1e-9
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-8
    g.close()


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("mode", ["two_lists", "keep_exclusion"])
def test_forces_after_a_break_other_paths(make_oracle, prec, mode):
    """two_lists: harmonic lists of different K (two parameter slots: the bonded work-list kernel), one dissociation
    reaction per list.  keep_exclusion: unexclude = 0, the broken pair stays excluded -- neither a bond force nor an LJ
    force between the two -- and the inline-bond mode ends (the exclusion set is no longer the bond set)."""
    pos, types, bonds = dimers(LENGTHS)
    spec = make_spec(pos, types, bonds, split_lists=mode == "two_lists")
    if mode == "two_lists":
        g, h, idx = build(spec, prec, [(0, 1.1, 0.0, {}), (1, 1.1, 0.0, dict(delta_1=5))])
    else:
        g, h, idx = build(spec, prec, [(0, 1.1, 0.0, dict(unexclude=False))])
    try:
        g.run(1)
        got, _ = event_rows(g)
        assert len(got) == 500
        if mode == "two_lists":
            assert idx == [0, 1] and sorted(set(e[3] for e in got)) == [0, 1]
            assert g.observe()["list_size"] == [250, 250]
            st = g.get_state("STATE")
            assert sorted(set(st[[e[1] - 1 for e in got if e[3] == 1]].tolist())) == [5]
        else:
            assert len(g.get_exclusions()) == 1000 and g.observe()["list_size"] == [500]
        o = oracle_after(make_oracle, spec, g, h)
        compare_forces(g, o, prec)
        if mode == "keep_exclusion":      # no force at all between the two ends of a broken, still excluded pair
            a, b = got[0][1], got[0][2]
            o2 = make_oracle()
            keep = np.ones(spec["n"], bool); keep[b - 1] = False
            s2 = dict(spec, n=spec["n"] - 1, pos=g.get_state("POS")[keep], types=g.get_state("TYPE")[keep], ids=spec["ids"][keep],
                      vel=spec["vel"][keep], mass=spec["mass"][keep], state=spec["state"][keep], res_id=spec["res_id"][keep],
                      exclusions=np.array([p for p in g.get_exclusions().tolist() if b not in p]),
                      lists=[dict(spec["lists"][0], ids=g.get_list(h[0]))])
            W.apply(s2, o2, thermostat=False, reactions=False)
            o2.run(0)
            fa = g.get_state("FORCE")[a - 1]
            assert np.abs(fa - o2.get_state("FORCE")[a - 1 - (1 if b < a else 0)]).max() < TOL_F[prec] * np.abs(g.get_state("FORCE")).max()
    finally:
        g.close()


# ---- 2: the rate rule, predicted exactly -----------------------------------------------------------------------------------

BOX2 = 22.3


@pytest.fixture(scope="module")
def rate_system():
    pos, types, bonds = dimers(np.full(4000, 1.0), box=BOX2, nside=16, seed=9)
    return make_spec(pos, types, bonds, box=BOX2), bonds


def run_rate(spec, prec, diss_rate, seed=SEED, steps=1):
    g, h, idx = build(spec, prec, [(0, 0.0, diss_rate, {})], seed=seed)
    try:
        g.run(steps)
        return event_rows(g)[0], idx[0], g.get_list(h[0]), g.get_state("STATE")
    finally:
        g.close()


def test_rate_rule_predicted_exactly(rate_system):
    spec, bonds = rate_system
    rate = 0.25 / DT
    got, index, left, state = run_rate(spec, 64, rate)
    want, wleft = predict(spec["pos"], BOX2, spec["types"], spec["state"], [bonds], [rx_row(index, 0, 0.0, rate)], step=1)
    print("broken %d of 4000 at p = %.17g" % (len(got), rate * DT * 1))
    assert got == canonical(want, 1)
    assert abs(len(got) - 1000) <= 137                      # 5 sigma of Binomial(4000, 0.25)
    assert np.array_equal(left, np.array(wleft[0]))
    assert state.sum() == 3 * len(got)
    assert run_rate(spec, 64, rate)[0] == got               # same seed, same events
    assert run_rate(spec, 32, rate)[0] == got               # the draw does not depend on the precision
    other = run_rate(spec, 64, rate, seed=SEED + 1)[0]
    assert other != got and abs(len(other) - 1000) <= 137


def test_rate_rule_certain_and_never(rate_system):
    spec, bonds = rate_system
    got, _, left, _ = run_rate(spec, 64, 1.0 / DT)          # p = 1: every qualifying bond
    assert len(got) == 4000 and len(left) == 0
    # p = 0: nothing breaks, and every table and the trajectory are bit-identical to a run without the registration
    a, ha, _ = build(spec, 64, [(0, 0.0, 0.0, {})])
    b, hb, _ = build(spec, 64, [])
    try:
        a.run(5); b.run(5)
        assert len(a.get_events()) == 0
        for what in ("POS_UNFOLDED", "VEL", "FORCE", "STATE", "TYPE", "MASS", "MOLID", "RESID", "IMAGE"):
            assert np.array_equal(a.get_state(what), b.get_state(what)), what
        assert np.array_equal(a.get_list(ha[0]), b.get_list(hb[0])) and np.array_equal(a.get_exclusions(), b.get_exclusions())
        oa, ob = a.observe(), b.observe()                   # (the list energy is an atomic sum: equal to rounding, not to the bit)
        assert {k: v for k, v in oa.items() if k != "epot_list"} == {k: v for k, v in ob.items() if k != "epot_list"}
        assert oa["epot_list"] == pytest.approx(ob["epot_list"], rel=1e-11)
        a.reaction_set_rate(0, 1.0 / DT)                    # chem_reaction_set_rate on a dissociation index sets diss_rate
        a.run(1)
        assert len(a.get_events()) == 4000
    finally:
        a.close(); b.close()


# ---- 3: state windows and multiplicity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_state_windows_and_multiplicity(make_oracle, prec):
    pos, types, bonds, kinds = bent_trimers_and_hubs()
    n = len(pos)
    state = np.zeros(n, np.int32)
    closed = [i0 for k, (kind, i0) in enumerate(kinds) if kind == "trimer" and k % 5 == 0]
    state[np.array(closed) - 1] = 5                           # particle a of every fifth trimer is outside its window
    spec = make_spec(pos, types, bonds, state=state)
    assert len(bonds) > 256
    g, h, idx = build(spec, prec, [(0, 1.1, 0.0, dict(delta_2=3))])
    try:
        g.run(1)
        x = g.get_state("POS")
        want, left = predict(x, BOX, types, state, [bonds], [rx_row(idx[0], 0, 1.1, 0.0)], step=1)
        assert event_rows(g)[0] == canonical(want, 1)
        st = g.get_state("STATE")
        exp = state.copy()
        for a, b, _, _ in want:
            exp[a - 1] += 1; exp[b - 1] += 3
        assert np.array_equal(st, exp)
        for k, (kind, i0) in enumerate(kinds):
            if kind == "hub":
                assert st[i0 - 1] == 9                        # three of five bonds lost
            elif k % 5 == 0:
                assert st[i0 - 1] == 5 and st[i0] == (3 if k % 4 >= 2 else 0)      # a-b survived, long or not
            else:
                assert st[i0] == [3, 0, 6, 6][k % 4]          # the middle particle: delta per lost bond
        assert np.array_equal(g.get_list(h[0]), np.array(left[0]))
        assert np.array_equal(g.get_state("MOLID"), clusters(n, left))
        compare_forces(g, oracle_after(make_oracle, spec, g, h), prec)
    finally:
        g.close()


# ---- 6: angles -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_angles_across_a_broken_bond_leave(make_oracle, prec):
    pos, types, bonds, kinds = bent_trimers_and_hubs(seed=13)
    tri = np.array([i0 for kind, i0 in kinds if kind == "trimer"])
    angles = np.stack([tri, tri + 1, tri + 2], 1)
    excl = np.concatenate([bonds, angles[:, [0, 2]]])
    spec = make_spec(pos, types, bonds, exclusions=excl,
                     extra_lists=[dict(arity=3, kind="ANG_HARMONIC", params=[1.25, 2.0], ids=angles)])
    g, h, idx = build(spec, prec, [(0, 1.1, 0.0, {})])
    try:
        g.run(1)
        x = g.get_state("POS")
        want, left = predict(x, BOX, types, spec["state"], [bonds], [rx_row(idx[0], 0, 1.1, 0.0)], step=1)
        assert event_rows(g)[0] == canonical(want, 1)
        cut = {frozenset((a, b)) for a, b, _, _ in want}
        keep = [t for t in angles.tolist() if frozenset(t[:2]) not in cut and frozenset(t[1:]) not in cut]
        assert 0 < len(keep) < len(angles)
        assert g.get_list(h[1]).tolist() == keep
        # 1-2 exclusions of the broken bonds lifted, the 1-3 exclusions of the removed angles stay (documented limit)
        wex = sorted((min(p), max(p)) for p in excl.tolist() if frozenset(p) not in cut)
        assert g.get_exclusions().tolist() == [list(p) for p in wex]
        compare_forces(g, oracle_after(make_oracle, spec, g, h), prec)
    finally:
        g.close()


# ---- 7: reversibility ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("unexclude", [True, False])
def test_break_and_rebond_in_the_same_step(unexclude):
    """125 dimers 1.15 long on every second lattice site (the only type-1 particle within 1.2 of a type-0 particle is its own
    partner).  Dissociation (cutoff 1.1, window [1, 2), delta -1) in front of an association (cutoff 1.2, window [0, 1),
    delta +1, certain): the bond breaks and forms again within the step.  With unexclude = 0 the pair stays excluded and the
    association scan, which honours exclusions, does not see it."""
    pos, types, bonds = dimers(np.full(125, 1.15), keep=lambda s: np.all(s % 2 == 0, 1))
    n = len(pos)
    spec = make_spec(pos, types, bonds, state=np.ones(n, np.int32))
    g, h, _ = build(spec, 64, [])
    try:
        win = dict(min_state_1=1, max_state_1=2, min_state_2=1, max_state_2=2, delta_1=-1, delta_2=-1)
        d = g.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h[0], unexclude=unexclude, **dict(RX, **win))
        a = g.reaction_add(0, 1, 1, 1, 0, 1, 0, 1, 1e12, 1.2, bond_list=h[0])
        assert (d, a) == (0, 1)                               # one index space
        g.reactions_enable(True)
        g.run(1)
        got, _ = event_rows(g)
        pairs = sorted((int(min(p)), int(max(p))) for p in bonds.tolist())
        assert [e for e in got if e[3] == d] == [(1, p[0], p[1], d) for p in pairs]        # type 0 = the odd, lower id = role 1
        if unexclude:
            assert [e for e in got if e[3] == a] == [(1, p[0], p[1], a) for p in pairs]
            assert got[:125] == [e for e in got if e[3] == d]                              # the break is logged in front
            assert g.get_list(h[0]).tolist() == [list(p) for p in pairs]
            assert np.all(g.get_state("STATE") == 1)
            assert g.get_exclusions().tolist() == [list(p) for p in pairs]
            assert np.array_equal(g.get_state("MOLID"), clusters(n, [pairs]))
        else:
            assert len(got) == 125 and len(g.get_list(h[0])) == 0
            assert np.all(g.get_state("STATE") == 0)
            assert g.get_exclusions().tolist() == [list(p) for p in pairs]
            assert np.array_equal(g.get_state("MOLID"), np.arange(1, n + 1))
    finally:
        g.close()


# ---- 8: the espressopp shim ------------------------------------------------------------------------------------------------

def test_shim_dissociation_reaction(base):
    from chemlab_amd import espp
    spec, bonds = base["spec"], base["bonds"]
    prev = espp._factory[0]
    try:
        espp.set_engine_factory(lambda: Engine(device=0, precision=64))
        system = espp.System()
        system.rng = espp.esutil.RNG(77)
        system.skin = SKIN
        box = (BOX,) * 3
        system.bc = espp.bc.OrthorhombicBC(system.rng, box)
        system.storage = espp.storage.DomainDecomposition(system, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), RC, SKIN))
        integrator = espp.integrator.VelocityVerlet(system)
        integrator.dt = DT
        plist = [[int(i + 1), int(spec["types"][i]), espp.Real3D(*spec["pos"][i]), 1.0] for i in range(spec["n"])]
        system.storage.addParticles(plist, "id", "type", "pos", "mass")
        system.storage.decompose()
        vl = espp.VerletList(system, cutoff=RC, exclusionlist=espp.DynamicExcludeList(integrator, [tuple(p) for p in bonds.tolist()]))
        lj = espp.interaction.VerletListLennardJones(vl)
        for t1, t2, eps, sig, rc in LJ:
            lj.setPotential(type1=t1, type2=t2, potential=espp.interaction.LennardJones(eps, sig, rc))
        system.addInteraction(lj, "lj")
        fpl = espp.FixedPairList(system.storage)
        fpl.addBonds([tuple(p) for p in bonds.tolist()])
        system.addInteraction(espp.interaction.FixedPairListHarmonic(system, fpl, espp.interaction.Harmonic(K_BOND, R0)), "bonds")
        tm = espp.integrator.TopologyManager(system)
        ar = espp.integrator.ChemicalReaction(system, vl, system.storage, tm, 1)
        r = espp.integrator.DissociationReaction(type_1=0, type_2=1, delta_1=1, delta_2=2, min_state_1=0, max_state_1=1,
                                                 min_state_2=0, max_state_2=1, rate=0.0, fpl=fpl, cutoff=1.1)
        r.diss_rate = 0.0
        assert r.get_reaction_cutoff().cutoff == 1.1
        pp = espp.integrator.PostProcessChangeProperty()
        pp.add_change_property(0, espp.integrator.TopologyParticleProperties(type=2, mass=1.5, q=0.0))
        r.add_postprocess(pp, "type_1")
        ar.add_reaction(r)
        integrator.addExtension(ar)
        integrator.run(1)
        eng = system.engine
        assert event_rows(eng)[0] == event_rows(base[64][0])[0]
        assert np.array_equal(eng.get_state("TYPE"), base[64][0].get_state("TYPE"))
        assert np.array_equal(eng.get_state("MASS"), base[64][0].get_state("MASS"))
        assert fpl.getAllBonds() == [tuple(p) for p in base[64][0].get_list(base[64][1][0]).tolist()]
        eng.close()
    finally:
        espp.set_engine_factory(prev)


# ---- 9: refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu):
    pos, types, bonds = dimers(LENGTHS)
    spec = make_spec(pos, types, bonds, extra_lists=[dict(arity=3, kind="ANG_HARMONIC", params=[1.0, 2.0], ids=np.zeros((0, 3), np.int64))])
    g = make_gpu(64)
    h = W.apply(spec, g, thermostat=False, reactions=False)
    with pytest.raises(ChemError) as ex:
        g.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h[0], **RX)
    assert ex.value.code == _capi.ESTATE                      # chem_reaction_init first
    g.reaction_init(1, True, 0, SEED)
    with pytest.raises(ChemError) as ex:
        g.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h[1], **RX)
    assert ex.value.code == _capi.EINVAL                      # an arity-3 list
    assert g.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h[0], **RX) == 0
    with pytest.raises(ChemError) as ex:
        g.comm_init_local(2, 0, 4711)
    assert ex.value.code == _capi.ENOTIMPL and "dissociation" in str(ex.value)
    # the other way round: a context that joined a decomposition refuses the registration
    g2 = make_gpu(64)
    h2 = W.apply(spec, g2, thermostat=False, reactions=False)
    g2.comm_init_local(1, 0, 4712)
    g2.reaction_init(1, True, 0, SEED)
    with pytest.raises(ChemError) as ex:
        g2.dissociation_add(diss_rate=0.0, cutoff=1.1, bond_list=h2[0], **RX)
    assert ex.value.code == _capi.ENOTIMPL
