"""Hybrid pair lists on the HIP path (chem_list_set_hybrid: k_bonded_work_hyb, k_bonded_hyb; rule set in
include/chem_mi355.h): a bond made by a reaction acts with lambda = min(1, lambda0 + rate (step - birth step)).

The CPU oracle has no hybrid lists.  Reference: the oracle on the read-back configuration WITHOUT the hybrid list (its pairs
stay excluded) plus the per-bond terms lambda F, lambda U of tests/hybrid_ref.py, each bond with its own lambda, which comes
from the event log (birth = step of the event that made the bond), not from the engine.  Where all hybrid bonds share one
lambda and are harmonic, the oracle with K lambda is a second, independent reference.

System: the even-sum sites of a lattice of spacing 1.4 (nearest sites 1.98 apart) in a box of edge 14 (rc 2.5 + skin 0.3:
five cells per axis), first layer 0.15 behind the low faces, so molecules straddle the periodic boundary, cell and tile
borders.  Every site carries a type-1 centre and, 0.70 or 0.75 away along body diagonals, its partners-to-be:
  A  centre + type 0                       reaction R0: 0 + 1
  B  centre + type 2                       reaction R1: 2 + 1
  C  type 0 + centre + type 2              the centre ends with two hybrid bonds, of different cohorts when R1 opens later
  D  type 0 + centre + type 4              centre - type 4 is a plain harmonic bond (K 20) of another list from the start
in the order A A B C D: 500 molecules, 1200 particles.  Reaction cutoff 0.85: a partner of another molecule is at least
1.98 - 0.75 - 0.1 = 1.13 from a centre, so exactly the intended pairs react (asserted).  The type-1 state window [0, 2)
allows two bonds per centre.  LJ sigma 0.4 on every type pair: its force at 0.7 is ~1.1, 6 % of the largest force (the plain
bonds' 12..18), so a hybrid pair that were not excluded at lambda = 0 would show.  Hybrid bonds: K 30, r0 1.0, force 15..18 at
full strength.  Velocities start at zero; dt 1e-4 (1e-3 in the trajectory test).

Tolerances are those of tests/test_gpu_dissociation.py (same system size, same kernels, one more multiplication): forces
1e-10 (fp64) / 5e-5 (fp32) of the largest force, list energies 1e-11 / 1e-5, LJ energy 1e-11 / 2e-6, fp64 trajectory 1e-9 of
the largest coordinate."""
import numpy as np
import pytest

import hybrid_ref as H
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError, Engine
from conftest import rel_err
from test_gpu_dissociation import TOL_EL, TOL_ELJ, TOL_F
from test_gpu_parity import _HUB, _run_ranks

pytestmark = pytest.mark.gpu

RC, SKIN, DT = 2.5, 0.3, 1e-4
K_HYB, R0 = 30.0, 1.0
K_PLAIN = 20.0
REACT_CUT = 0.85
SPACING = 1.4
LJ = [(a, b, 1.0, 0.4, RC) for a in range(5) for b in range(a, 5)]
INF = 1e30


# ---- the system ------------------------------------------------------------------------------------------------------------

def molecules(box=(14.0, 14.0, 14.0), kinds="AABCD", seed=5, dt=DT):
    """Returns the spec (lists: the plain D bonds and an empty angle-free rest; the hybrid list is created by build()) and
    the expected reacting pairs, 0-based (partner, centre): r0 for reaction 0 + 1, r1 for 2 + 1."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, dtype=np.float64)
    ns = np.rint(box / SPACING).astype(int)
    sites = np.stack(np.meshgrid(*[np.arange(m) for m in ns], indexing="ij"), -1).reshape(-1, 3)
    sites = sites[sites.sum(1) % 2 == 0]
    c = sites * SPACING + 0.15 + rng.uniform(-0.05, 0.05, sites.shape)
    pos, types, plain, triples, r0, r1 = [], [], [], [], [], []
    for k in range(len(c)):
        kind = kinds[k % len(kinds)]
        d1 = rng.choice([-1.0, 1.0], 3) / np.sqrt(3.0)
        d2 = d1.copy(); d2[rng.integers(3)] *= -1.0
        l1, l2 = (0.70, 0.75) if k % 2 else (0.75, 0.70)
        ctr = len(pos)
        pos.append(c[k]); types.append(1)
        if kind in "ACD":
            pos.append(c[k] - l1 * d1); types.append(0); r0.append((ctr + 1, ctr))
        if kind in "BC":
            pos.append(c[k] + l2 * d2); types.append(2); r1.append((len(pos) - 1, ctr))
        if kind == "D":
            pos.append(c[k] + l2 * d2); types.append(4)
            plain.append((ctr + 1, ctr + 3)); triples.append((ctr + 2, ctr + 1, ctr + 3))
    n = len(pos)
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=dt, ids=np.arange(1, n + 1), types=np.asarray(types, np.int32), pos=np.array(pos),
                vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32), lj=LJ,
                kT=1.0, gamma=0.0, seed=1, rebuild_criterion=1,
                lists=[dict(arity=2, kind="HARMONIC", params=[K_PLAIN, R0], ids=np.asarray(plain, np.int64).reshape(-1, 2))] if plain else [],
                exclusions=np.asarray(plain, np.int64).reshape(-1, 2))
    spec = W.snap_to_grid(spec)
    spec["triples"] = np.asarray(triples, np.int64).reshape(-1, 3)
    # isolation: within the reaction cutoff of a centre lie exactly its own partners
    x, ty = spec["pos"], spec["types"]
    ctrs = np.nonzero(ty == 1)[0]
    for t, want in ((0, r0), (2, r1)):
        part = np.nonzero(ty == t)[0]
        d = x[part][:, None, :] - x[ctrs][None, :, :]
        d -= box * np.rint(d / box)
        r = np.sqrt((d * d).sum(2))
        assert np.abs(r - REACT_CUT).min() > 1e-3
        got = sorted((int(part[i]), int(ctrs[j])) for i, j in zip(*np.nonzero(r < REACT_CUT)))
        assert got == sorted(want)
    return spec, r0, r1


@pytest.fixture(scope="module")
def base():
    spec, r0, r1 = molecules()
    assert spec["n"] == 1200 and len(r0) == 400 and len(r1) == 200
    return dict(spec=spec, r0=r0, r1=r1)


def build(spec, prec, lambda0=0.0, rate=0.25, hybrid=True, kind="HARMONIC", params=(K_HYB, R0), typed=None, r1_rate=0.0, opts=None,
          engine=None, table=None):
    """Engine with the spec's lists, then the reaction list (hybrid unless hybrid = False) and the reactions R0 (open) and
    R1 (rate r1_rate).  typed: {(t1, t2): params} for a by-types list.  Returns engine, handles (hyb = the reaction list)."""
    g = engine if engine is not None else Engine(device=0, precision=prec)
    for k, v in (opts or {}).items():
        g.set_option(k, v)
    h = W.apply(spec, g, thermostat=False, reactions=False)
    hh = g.list_create(2, kind, typed is not None)
    if table is not None:
        params = [g.table_create(*table)]
    if typed is None:
        g.list_set_params(hh, list(params))
    else:
        for tt, p in typed.items():
            g.list_set_params(hh, list(p), types=tt)
    if hybrid:
        g.list_set_hybrid(hh, lambda0, rate)
    h["hyb"] = hh
    g.reaction_init(1, True, 0, 4)
    common = dict(delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=2, cutoff=REACT_CUT, bond_list=hh,
                  intramolecular=True, intraresidual=True)
    h["R0"] = g.reaction_add(0, 1, rate=INF, **common)
    h["R1"] = g.reaction_add(2, 1, rate=r1_rate, **common)
    g.reactions_enable(True)
    return g, h


def event_rows(g):
    return [(int(e["step"]), int(e["id_a"]), int(e["id_b"]), int(e["reaction"])) for e in g.get_events()]


def expected_lambda(g, h, lambda0, rate):
    bonds = g.get_list(h["hyb"])
    birth = H.births(event_rows(g), {h["R0"], h["R1"]}, bonds)
    return bonds, birth, H.ramp(lambda0, rate, g.step, birth)


def oracle_on(make_oracle, spec, g, lists):
    o = make_oracle()
    s2 = dict(spec, pos=g.get_state("POS"), vel=g.get_state("VEL"), types=g.get_state("TYPE"), state=g.get_state("STATE"),
              mass=g.get_state("MASS"), exclusions=g.get_exclusions(), lists=lists)
    W.apply(s2, o, thermostat=False, reactions=False)
    o.run(0)
    return o


def check(g, h, spec, prec, make_oracle, lam, fun, same_lambda=None, label=""):
    """forces and energies of g against oracle-without-the-hybrid-list + sum of lambda-weighted bond terms; with
    same_lambda (all bonds harmonic at that lambda) also against the oracle with K lambda"""
    g.run(0)
    x = g.get_state("POS")
    bonds = g.get_list(h["hyb"])
    o = oracle_on(make_oracle, spec, g, spec["lists"])
    Fh, eh = H.bond_terms(x, spec["box"], bonds - 1, lam, fun)
    Fref = o.get_state("FORCE") + Fh
    fg = g.get_state("FORCE")
    og, oo = g.observe(), o.observe()
    err = rel_err(fg, Fref)
    print("%s prec %d: %d hybrid bonds, force rel err %.3e, hybrid part %.3e of the largest force" % (label, prec, len(bonds), err, np.abs(Fh).max() / np.abs(Fref).max()))
    assert err < TOL_F[prec]
    assert og["list_size"][h["hyb"]] == len(bonds)
    assert og["epot_list"][h["hyb"]] == pytest.approx(eh, rel=TOL_EL[prec], abs=1e-12)
    for k in range(len(spec["lists"])):
        assert og["epot_list"][k] == pytest.approx(oo["epot_list"][k], rel=TOL_EL[prec], abs=1e-12)
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=TOL_ELJ[prec])
    o.close()
    if same_lambda is not None:
        o2 = oracle_on(make_oracle, spec, g, spec["lists"] + [dict(arity=2, kind="HARMONIC", params=[K_HYB * same_lambda, R0], ids=bonds)])
        err2 = rel_err(fg, o2.get_state("FORCE"))
        print("   against the oracle with K * %.2f: %.3e" % (same_lambda, err2))
        assert err2 < TOL_F[prec]
        assert og["epot_list"][h["hyb"]] == pytest.approx(o2.observe()["epot_list"][len(spec["lists"])], rel=TOL_EL[prec], abs=1e-12)
        o2.close()
    return fg, Fh


def id_pairs(pairs):
    return sorted((a + 1, b + 1) for a, b in pairs)


# ---- 1: the ramp ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_ramp(base, make_oracle, prec):
    spec = base["spec"]
    g, h = build(spec, prec, 0.0, 0.25)
    try:
        assert len(g.list_get_lambda(h["hyb"])) == 0
        g.run(1)
        assert sorted((a, b) for _, a, b, _ in event_rows(g)) == id_pairs(base["r0"])
        g.reactions_enable(False)
        want_excl = sorted([tuple(p) for p in spec["exclusions"].tolist()] + [(min(a, b), max(a, b)) for a, b in id_pairs(base["r0"])])
        assert [tuple(p) for p in g.get_exclusions().tolist()] == want_excl          # excluded from the moment the bond exists
        bonds, birth, lam = expected_lambda(g, h, 0.0, 0.25)
        assert np.all(birth == 1) and np.array_equal(g.list_get_lambda(h["hyb"]), np.zeros(400))
        fg, Fh = check(g, h, spec, prec, make_oracle, lam, H.harmonic(K_HYB, R0), same_lambda=0.0, label="lambda 0")
        assert np.abs(Fh).max() == 0.0
        full = H.bond_terms(g.get_state("POS"), spec["box"], bonds - 1, np.ones(400), H.harmonic(K_HYB, R0))[0]
        assert np.abs(full).max() > 0.5 * np.abs(fg).max()                           # (at full strength they would dominate)
        for k, want in enumerate([0.25, 0.5, 0.75, 1.0, 1.0]):
            g.run(1)
            got = g.list_get_lambda(h["hyb"])
            assert np.array_equal(got, np.full(400, want)), (k, got[:4])
            _, _, lam = expected_lambda(g, h, 0.0, 0.25)
            assert np.array_equal(lam, got)
            check(g, h, spec, prec, make_oracle, lam, H.harmonic(K_HYB, R0), same_lambda=want, label="lambda %.2f" % want)
    finally:
        g.close()


@pytest.mark.parametrize("prec", [64, 32])
def test_split_run_is_bit_identical(base, prec):
    out = []
    for split in ((2, 3), (5,)):
        g, h = build(base["spec"], prec, 0.0, 0.25)
        g.run(1)
        g.reactions_enable(False)
        for k in split:
            g.run(k)
        out.append((g.get_state("POS"), g.get_state("VEL"), g.list_get_lambda(h["hyb"])))
        g.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert np.abs(out[0][1]).max() > 0


# ---- 2: two cohorts in one list ---------------------------------------------------------------------------------------------

def two_cohorts(spec, prec, rate=0.125, wait=3, lambda0=0.0, before_run=None, **kw):
    """R0 at step 1, R1 opened after `wait` more steps: bonds of birth 1 and 2 + wait in one list"""
    g, h = build(spec, prec, lambda0, rate, **kw)
    if before_run is not None:
        before_run(g, h)
    g.run(1 + wait)
    g.reaction_set_rate(h["R1"], INF)
    g.run(1)
    return g, h


@pytest.mark.parametrize("prec", [64, 32])
def test_two_cohorts_in_one_list(base, make_oracle, prec):
    spec = base["spec"]
    g, h = two_cohorts(spec, prec)
    try:
        g.run(1)                                                       # step 6: cohort 1 at 5/8, cohort 2 at 1/8
        ev = event_rows(g)
        assert sorted((a, b) for s, a, b, r in ev if r == h["R0"]) == id_pairs(base["r0"]) and {s for s, _, _, r in ev if r == h["R0"]} == {1}
        assert sorted((a, b) for s, a, b, r in ev if r == h["R1"]) == id_pairs(base["r1"]) and {s for s, _, _, r in ev if r == h["R1"]} == {5}
        bonds, birth, lam = expected_lambda(g, h, 0.0, 0.125)
        assert sorted(set(lam.tolist())) == [0.125, 0.625] and (lam == 0.625).sum() == 400 and (lam == 0.125).sum() == 200
        assert np.array_equal(g.list_get_lambda(h["hyb"]), lam)
        # a centre with two hybrid bonds of different cohorts (C), one with a hybrid and a plain bond (D)
        deg = {}
        for (a, b), l in zip(bonds.tolist(), lam.tolist()):
            for p in (a, b):
                deg.setdefault(p, []).append(l)
        assert sum(1 for v in deg.values() if sorted(v) == [0.125, 0.625]) == 100
        plain_members = set(spec["lists"][0]["ids"].ravel().tolist())
        assert sum(1 for p, v in deg.items() if p in plain_members and v == [0.625]) == 100
        check(g, h, spec, prec, make_oracle, lam, H.harmonic(K_HYB, R0), label="two cohorts")
    finally:
        g.close()


# ---- 3: every kernel path ---------------------------------------------------------------------------------------------------

TABLE = (0.3, 0.01, 25.0 * (0.3 + 0.01 * np.arange(121) - 0.9) ** 2 + 0.5 * np.sin(3.0 * (0.3 + 0.01 * np.arange(121))),
         -50.0 * (0.3 + 0.01 * np.arange(121) - 0.9) - 1.5 * np.cos(3.0 * (0.3 + 0.01 * np.arange(121))))

PATHS = {
    "harmonic": dict(),                                                                   # bonds-only work-list kernel
    "full": dict(angles=True, kind="TABULATED", table=TABLE),                             # full work-list kernel
    "inline_system": dict(kinds="AABC"),                                                  # exclusions = bonds, one K
    "by_types": dict(typed={(0, 1): (K_HYB, R0), (2, 1): (45.0, 0.9)}),
    "fene": dict(kind="FENE", params=(30.0, 0.0, 1.5)),
    "bonds_inline_0": dict(kinds="AABC", opts={"bonds_inline": 0}),
    "bond_pass_0": dict(kinds="AABC", opts={"bond_pass": 0}),
    "unfused": dict(opts={"fused_rebuild": 0}),                                           # k_bonded_prep of its own launch
    "no_tiles": dict(opts={"tiles": 0}),                                                  # per-particle k_bonded_hyb<.., false>
}


def path_fun(cfg, spec, bonds):
    if "table" in cfg:
        return H.table(*cfg["table"])
    if "typed" in cfg:
        ty = spec["types"]
        return [H.harmonic(*cfg["typed"][(int(ty[a - 1] if ty[a - 1] != 1 else ty[b - 1]), 1)]) for a, b in bonds.tolist()]
    if cfg.get("kind") == "FENE":
        return H.fene(*cfg["params"])
    return H.harmonic(K_HYB, R0)


@pytest.fixture(scope="module")
def path_specs():
    out = {}
    for kinds in ("AABCD", "AABC"):
        out[kinds] = molecules(kinds=kinds)
    return out


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_kernel_path(path_specs, make_oracle, path, prec):
    cfg = PATHS[path]
    spec, r0, r1 = path_specs[cfg.get("kinds", "AABCD")]
    if cfg.get("angles"):
        spec = dict(spec, lists=spec["lists"] + [dict(arity=3, kind="ANG_HARMONIC", params=[4.0, 1.9], ids=spec["triples"])])
    kw = {k: cfg[k] for k in ("kind", "params", "typed", "opts", "table") if k in cfg}
    g, h = two_cohorts(spec, prec, rate=0.125, wait=1, **kw)            # births 1 and 3
    try:
        g.run(2)                                                         # step 5: lambda 1/2 and 1/4
        bonds, birth, lam = expected_lambda(g, h, 0.0, 0.125)
        assert sorted(set(lam.tolist())) == [0.25, 0.5] and len(bonds) == len(r0) + len(r1)
        assert np.array_equal(g.list_get_lambda(h["hyb"]), lam)
        fun = path_fun(cfg, spec, bonds)
        fg, Fh = check(g, h, spec, prec, make_oracle, lam, fun, label=path)
        full = H.bond_terms(g.get_state("POS"), spec["box"], bonds - 1, np.ones(len(bonds)), fun)[0]
        assert rel_err(Fh, full) > 0.4                                   # (full strength is far outside the tolerance)
    finally:
        g.close()
    if path == "inline_system":
        # the same spec without set_hybrid runs its bonds inline and still matches the oracle: the hybrid list left that mode,
        # nothing broke it
        p, hp = two_cohorts(spec, prec, rate=0.125, wait=1, hybrid=False)
        try:
            p.run(2)
            assert np.array_equal(p.list_get_lambda(hp["hyb"]), np.ones(len(bonds)))
            o = oracle_on(make_oracle, spec, p, [dict(arity=2, kind="HARMONIC", params=[K_HYB, R0], ids=p.get_list(hp["hyb"]))])
            p.run(0)
            assert rel_err(p.get_state("FORCE"), o.get_state("FORCE")) < TOL_F[prec]
            assert p.observe()["epot_list"][hp["hyb"]] == pytest.approx(o.observe()["epot_list"][0], rel=TOL_EL[prec])
            tm = p.timers()
            print("plain list: bonded launches sampled", tm["bonded_kernel_launches"])
        finally:
            p.close()


# ---- 4: lambda0 = 1 is a plain list -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kinds", ["AABCD"])
def test_lambda0_one_is_bit_identical_to_a_plain_list(path_specs, kinds):
    spec = path_specs[kinds][0]
    out = []
    for hybrid in (True, False):
        g, h = two_cohorts(spec, 64, rate=0.25, wait=1, lambda0=1.0, hybrid=hybrid)
        g.run(0)
        f = g.get_state("FORCE")
        e = g.observe()["epot_list"]
        g.run(20)
        out.append((f, g.get_state("POS"), g.get_state("VEL"), e, g.list_get_lambda(h["hyb"])))
        g.close()
    assert np.all(out[0][4] == 1.0) and np.all(out[1][4] == 1.0) and len(out[0][4]) == 600
    assert np.array_equal(out[0][0], out[1][0]) and np.abs(out[0][0]).max() > 10.0
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    # (list energies are summed by atomic adds, whose order differs from launch to launch: equal to rounding, not bit for bit)
    assert out[0][3] == pytest.approx(out[1][3], rel=1e-13)


# ---- 5: trajectory across the ramp ------------------------------------------------------------------------------------------

def test_trajectory_across_the_ramp(make_oracle):
    """fp64, 40 steps of 1e-3 across a ramp of 16 steps, two cohorts (births 1 and 5).  Reference: velocity Verlet written out
    here, the forces of every step from an oracle that is rebuilt with one harmonic list per cohort, K scaled by that
    cohort's lambda at that step."""
    dt = 1e-3
    spec, r0, r1 = molecules(dt=dt)
    rate = 1.0 / 16
    g, h = two_cohorts(spec, 64, rate=rate, wait=3)
    try:
        g.reactions_enable(False)
        s0 = g.step
        assert s0 == 5
        bonds, birth, _ = expected_lambda(g, h, 0.0, rate)
        cohorts = [bonds[birth == b] for b in (1, 5)]
        assert [len(c) for c in cohorts] == [400, 200]
        box = np.asarray(spec["box"])
        x, v, m = g.get_state("POS"), g.get_state("VEL"), g.get_state("MASS")[:, None]
        base_cfg = dict(spec, types=g.get_state("TYPE"), state=g.get_state("STATE"), exclusions=g.get_exclusions())

        def forces(x, step):
            lists = spec["lists"] + [dict(arity=2, kind="HARMONIC", params=[K_HYB * float(H.ramp(0.0, rate, step, b)), R0], ids=c)
                                     for b, c in zip((1, 5), cohorts)]
            o = make_oracle()
            W.apply(dict(base_cfg, pos=x - np.floor(x / box) * box, vel=np.zeros_like(x), lists=lists), o, thermostat=False, reactions=False)
            o.run(0)
            f = o.get_state("FORCE")
            o.close()
            return f
        f = forces(x, s0)
        for s in range(s0, s0 + 40):
            v = v + (0.5 * dt) * f / m
            x = x + dt * v
            f = forces(x, s + 1)
            v = v + (0.5 * dt) * f / m
        g.run(40)
        assert sorted(set(g.list_get_lambda(h["hyb"]).tolist())) == [1.0]
        xg = g.get_state("POS")
        d = xg - x
        d -= box * np.rint(d / box)
        moved = xg - spec["pos"]
        moved -= box * np.rint(moved / box)
        print("trajectory err %.3e, largest displacement %.3e" % (np.abs(d).max() / np.abs(xg).max(), np.abs(moved).max()))
        assert np.abs(moved).max() > 1e-3
        assert np.abs(d).max() / np.abs(xg).max() < 1e-9
        assert rel_err(g.get_state("VEL"), v) < 1e-8
    finally:
        g.close()


# ---- 6: dissociation on a hybrid list ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_dissociation_on_a_hybrid_list(base, make_oracle, prec):
    """Mid-ramp, with the association closed, a dissociation reaction breaks about half of the 0 - 1 bonds (one Philox draw
    per bond, p = 1/2); one step later the association is open again and the broken pairs bond anew."""
    spec = base["spec"]
    rate = 0.0625
    def add_dissociation(g, h):
        h["dz"] = g.dissociation_add(0, 1, -1, -1, 1, 2, 1, 3, diss_rate=0.0, cutoff=0.0, bond_list=h["hyb"])
    g, h = two_cohorts(spec, prec, rate=rate, wait=1, before_run=add_dissociation)   # births 1 (0 - 1) and 3 (2 - 1)
    try:
        dz = h["dz"]
        g.run(1)                                                          # step 4
        before = [tuple(p) for p in g.get_list(h["hyb"]).tolist()]
        g.reaction_set_rate(h["R0"], 0.0)
        g.reaction_set_rate(dz, 0.5 / DT)                                # p = diss_rate * dt * interval = 1/2
        g.run(1)                                                          # step 5: bonds break, none forms
        g.reaction_set_rate(dz, 0.0)
        broken = sorted((a, b) for s, a, b, r in event_rows(g) if r == dz)
        assert {s for s, _, _, r in event_rows(g) if r == dz} == {5}
        assert 120 < len(broken) < 280 and set(broken) <= set(id_pairs(base["r0"]))
        left = [p for p in before if (min(p), max(p)) not in {(min(q), max(q)) for q in broken}]
        assert [tuple(p) for p in g.get_list(h["hyb"]).tolist()] == left                 # order of the survivors kept
        bonds, birth, lam = expected_lambda(g, h, 0.0, rate)
        assert sorted(set(birth.tolist())) == [1, 3] and np.array_equal(g.list_get_lambda(h["hyb"]), lam)   # the survivors' lambda go on
        check(g, h, spec, prec, make_oracle, lam, H.harmonic(K_HYB, R0), label="after the break")
        g.reaction_set_rate(h["R0"], INF)
        g.run(1)                                                          # step 6: the broken pairs bond again
        g.run(2)                                                          # step 8
        bonds, birth, lam = expected_lambda(g, h, 0.0, rate)
        assert len(bonds) == 600 and (birth == 6).sum() == len(broken) and (birth == 1).sum() == 400 - len(broken) and (birth == 3).sum() == 200
        assert sorted(set(lam.tolist())) == [2 * rate, 5 * rate, 7 * rate]                # a pair that bonds again starts at lambda0
        assert np.array_equal(g.list_get_lambda(h["hyb"]), lam)
        check(g, h, spec, prec, make_oracle, lam, H.harmonic(K_HYB, R0), label="bonded again")
    finally:
        g.close()


# ---- 7: two slabs -------------------------------------------------------------------------------------------------------------

def test_two_slabs(make_gpu, make_oracle):
    spec, r0, r1 = molecules(box=(14.0, 14.0, 28.0))
    P, zb = 2, 14.0
    z = spec["pos"][:, 2] - np.floor(spec["pos"][:, 2] / 28.0) * 28.0
    side = [(z[a] < zb, z[b] < zb) for a, b in r0 + r1]
    assert sum(1 for s in side if s == (True, True)) > 100 and sum(1 for s in side if s == (False, False)) > 100
    assert sum(1 for s in side if s[0] != s[1]) >= 10                    # bonds form across the slab boundary (and the periodic one)
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        _, h = build(spec, 64, 0.0, 0.125, engine=g)
        g.run(2)
        g.reaction_set_rate(h["R1"], INF)
        g.run(1)                                                          # births 1 and 3
        g.run(2)                                                          # step 5
        g.run(0)
        return dict(x=g.get_state("POS"), f=g.get_state("FORCE"), lam=g.list_get_lambda(h["hyb"]), bonds=g.get_list(h["hyb"]), h=h,
                    ev=event_rows(g), ob=g.observe())
    out = _run_ranks(P, rank)
    assert np.array_equal(out[0]["x"], out[1]["x"])
    assert np.array_equal(out[0]["lam"], out[1]["lam"]) and np.array_equal(out[0]["bonds"], out[1]["bonds"])
    h, bonds = out[0]["h"], out[0]["bonds"]
    assert sorted((min(a, b), max(a, b)) for a, b in bonds.tolist()) == sorted((min(a, b), max(a, b)) for a, b in id_pairs(r0 + r1))
    birth = H.births(out[0]["ev"], {h["R0"], h["R1"]}, bonds)
    lam = H.ramp(0.0, 0.125, 5, birth)
    assert sorted(set(lam.tolist())) == [0.25, 0.5] and np.array_equal(out[0]["lam"], lam)
    excl = sorted([tuple(p) for p in spec["exclusions"].tolist()] + [(min(a, b), max(a, b)) for a, b in bonds.tolist()])
    o = make_oracle()
    W.apply(dict(spec, pos=out[0]["x"], exclusions=np.array(excl)), o, thermostat=False, reactions=False)
    o.run(0)
    Fh, eh = H.bond_terms(out[0]["x"], spec["box"], bonds - 1, lam, H.harmonic(K_HYB, R0))
    Fref = o.get_state("FORCE") + Fh
    for r in range(P):
        print("rank %d: force rel err %.3e" % (r, rel_err(out[r]["f"], Fref)))
        assert rel_err(out[r]["f"], Fref) < TOL_F[64]
        assert out[r]["ob"]["epot_list"][h["hyb"]] == pytest.approx(eh, rel=TOL_EL[64])
    full = H.bond_terms(out[0]["x"], spec["box"], bonds - 1, np.ones(len(bonds)), H.harmonic(K_HYB, R0))[0]
    assert rel_err(Fh, full) > 0.4


# ---- 8: the espressopp shim, end to end ----------------------------------------------------------------------------------------

def test_shim_end_to_end(base):
    from chemlab_amd import espp
    spec = base["spec"]
    box = tuple(spec["box"])
    prev = espp._factory[0]
    try:
        espp.set_engine_factory(lambda: Engine(device=0, precision=64))
        system = espp.System()
        system.rng = espp.esutil.RNG(4)
        system.skin = SKIN
        system.bc = espp.bc.OrthorhombicBC(system.rng, box)
        system.storage = espp.storage.DomainDecomposition(system, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), RC, SKIN))
        integrator = espp.integrator.VelocityVerlet(system)
        integrator.dt = DT
        plist = [[int(i + 1), int(spec["types"][i]), espp.Real3D(*spec["pos"][i]), 1.0] for i in range(spec["n"])]
        system.storage.addParticles(plist, "id", "type", "pos", "mass")
        system.storage.decompose()
        plain = [tuple(p) for p in spec["lists"][0]["ids"].tolist()]
        vl = espp.VerletList(system, cutoff=RC, exclusionlist=espp.DynamicExcludeList(integrator, plain))
        lj = espp.interaction.VerletListLennardJones(vl)
        for t1, t2, eps, sig, rc in LJ:
            lj.setPotential(type1=t1, type2=t2, potential=espp.interaction.LennardJones(eps, sig, rc))
        system.addInteraction(lj, "lj")
        fpl0 = espp.FixedPairList(system.storage)
        fpl0.addBonds(plain)
        system.addInteraction(espp.interaction.FixedPairListHarmonic(system, fpl0, espp.interaction.Harmonic(K_PLAIN, R0)), "bonds")
        fpl = espp.FixedPairListLambda(system.storage, 0.0)
        inter = espp.interaction.FixedPairListLambdaHarmonic(system, fpl, espp.interaction.Harmonic(K_HYB, R0))
        system.addInteraction(inter, "fpl_0")
        ext = espp.integrator.FixedListDynamicResolution(system)
        ext.register_pair_list(fpl, 0.25)
        integrator.addExtension(ext)
        tm = espp.integrator.TopologyManager(system)
        ar = espp.integrator.ChemicalReaction(system, vl, system.storage, tm, 1)
        r = espp.integrator.Reaction(type_1=0, type_2=1, delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=2,
                                     rate=INF, fpl=fpl, cutoff=REACT_CUT)
        r.intramolecular = r.intraresidual = True
        ar.nearest_mode = True
        ar.add_reaction(r)
        integrator.addExtension(ar)
        res = espp.analysis.ResolutionFixedPairList(system, fpl)
        mon = espp.analysis.SystemMonitor(system, integrator, None)
        mon.add_observable("count_0", espp.analysis.NFixedPairListEntries(system, fpl))
        mon.add_observable("res_fpl_0", res)
        mon.add_observable("fpl_0", espp.analysis.PotentialEnergy(system, inter))
        assert res.compute() == 0.0                                      # empty list
        eng = system.engine
        for want in (0.0, 0.25, 0.5, 0.75, 1.0, 1.0):
            integrator.run(1)
            assert res.compute() == want and fpl.getAllLambda() == [want] * 400
            mon.perform_action()
            names, row = mon.last
            assert names == ["step", "time", "count_0", "res_fpl_0", "fpl_0"] and row[2] == 400.0 and row[3] == want
            bonds = np.array(fpl.getAllBonds())
            eh = H.bond_terms(eng.get_state("POS"), spec["box"], bonds - 1, np.full(400, want), H.harmonic(K_HYB, R0))[1]
            assert row[4] == pytest.approx(eh, rel=TOL_EL[64], abs=1e-12)
        assert sorted(tuple(p) for p in bonds.tolist()) == id_pairs(base["r0"])
        eng.close()
    finally:
        espp.set_engine_factory(prev)


# ---- 9: refusals through the C ABI --------------------------------------------------------------------------------------------

def test_set_hybrid_refusals(base, make_gpu):
    spec = base["spec"]
    g = make_gpu(64)
    h = W.apply(dict(spec, lists=spec["lists"] + [dict(arity=3, kind="ANG_HARMONIC", params=[4.0, 1.9], ids=spec["triples"])]), g,
                thermostat=False, reactions=False)
    empty = g.list_create(2, "FENE_LJ")
    for args, code in (((h[1], 0.0, 0.1), _capi.EINVAL), ((empty, -0.1, 0.1), _capi.EINVAL), ((empty, 1.5, 0.1), _capi.EINVAL),
                       ((empty, 0.5, -1.0), _capi.EINVAL), ((empty, float("nan"), 0.1), _capi.EINVAL), ((empty, 0.5, float("inf")), _capi.EINVAL),
                       ((h[0], 0.0, 0.1), _capi.ESTATE), ((99, 0.0, 0.1), _capi.EINVAL)):
        with pytest.raises(ChemError) as ex:
            g.list_set_hybrid(*args)
        assert ex.value.code == code, args
    g.list_set_hybrid(empty, 0.0, 0.0)
    g.list_set_hybrid(empty, 0.5, 0.02)                                  # again on an empty list: allowed
    assert np.array_equal(g.list_get_lambda(h[0]), np.ones(len(spec["lists"][0]["ids"])))
    assert len(g.list_get_lambda(empty)) == 0
