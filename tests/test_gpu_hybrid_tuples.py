"""Hybrid triple and quadruple lists on the HIP path (chem_list_set_hybrid_tuples: the HYB and COUL instantiations of the bonded
kernels, k_bonded_virial_tensor; rule set in include/chem_mi355.h): an angle or dihedral the topology manager spawns around a new
bond acts with lambda = min(1, lambda0 + rate (step - birth step)).

The CPU oracle has no hybrid lists.  Reference: the oracle on the read-back configuration WITHOUT the hybrid tuple lists (their
1-3 / 1-4 pairs stay excluded) plus tests/hybrid_tuples_ref.py: lambda_e U_e per entry and -grad of their sum by autograd, every
entry with its own lambda, which comes from the event log (birth = step of the event whose bond spawned the tuple; what is
spawned is restated there from the bond graph), not from the engine.

System: hybrid_tuples_ref.scene() -- 216 chains of 4..6 beads with one or two gaps that the reactions R0 (0 + 1, open from the
start) and R1 (2 + 1, opened later) close; 993 particles in a box of edge 14, five cells per axis.  Lists, in this order, so that
the row of one bead of the D chains holds entries of width 1, 1, 2, 2, 2, 1 interleaved:
  0 plain bonds (harmonic)   1 plain angles   2 HYBRID angles   3 plain dihedrals   4 HYBRID dihedrals   5 reaction bonds
Rates are powers of two, so every expected lambda is an exact double.  Velocities start at zero; dt 1e-4.

Tolerances are those of tests/test_gpu_dissociation.py and tests/test_gpu_bonded.py, as in tests/test_gpu_hybrid_bonds.py (same
kernels, one more multiplication): forces 1e-10 (fp64) / 5e-5 (fp32) of the largest force, list energies 1e-11 / 1e-5, LJ energy
1e-11 / 2e-6.  Every bending angle stays within 60..150 degrees (asserted on the read-back configuration), where the plain
bounds hold."""
import math

import numpy as np
import pytest

import hybrid_ref as H
import hybrid_tuples_ref as T
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError, Engine
from conftest import rel_err
from test_gpu_bonded import TOL_F as TOL_F_BONDED
from test_gpu_dissociation import TOL_EL, TOL_ELJ, TOL_F
from test_gpu_parity import _HUB, _run_ranks
from test_gpu_pressure import TOL as TOL_P

pytestmark = pytest.mark.gpu

INF = 1e30
LJ = [(a, b, 1.0, 0.4, T.SCENE_RC) for a in range(5) for b in range(a, 5)]
BOND0 = dict(arity=2, kind="HARMONIC", params=[20.0, 0.9])
ANG0 = dict(arity=3, kind="ANG_HARMONIC", params=[4.0, 1.9])
DIH0 = dict(arity=4, kind="DIH_HARMONIC", params=[3.0, 1.0])
RBOND = dict(arity=2, kind="HARMONIC", params=[30.0, 1.0])
ANG = dict(arity=3, kind="ANG_HARMONIC", params=[8.0, 1.6])
DIH = dict(arity=4, kind="DIH_NCOS", params=[2.0, 0.35, 3.0])
_TH = (math.pi / 180) * np.arange(181)
_PHI = -math.pi + (2.0 * math.pi / 720) * np.arange(721)
TAB_ANG = (0.0, math.pi / 180, 4.0 * (_TH - 1.6) ** 2 + np.cos(2.0 * _TH), -8.0 * (_TH - 1.6) + 2.0 * np.sin(2.0 * _TH))
TAB_DIH = (_PHI[0], 2.0 * math.pi / 720, 0.8 * (1 + np.cos(2 * _PHI - 0.3)), 1.6 * np.sin(2 * _PHI - 0.3))


@pytest.fixture(scope="module")
def base():
    s = T.scene()
    assert s["n"] == 993 and len(s["r0"]) == 173 and len(s["r1"]) == 86
    return s


def spec_of(scene):
    return dict({k: scene[k] for k in ("n", "box", "rc", "skin", "dt", "ids", "types", "pos", "vel", "mass", "state", "res_id", "kT", "gamma", "seed", "rebuild_criterion")},
                lj=LJ, exclusions=scene["exclusions"], lists=[])


def c14_pairs(scene):
    """pairs for a 1-4 Coulomb list: the last bead of an A chain with the last bead of the A chain on the next site (sites 5k + 4
    and 5k + 5).  Pair lists feed the bond graph; these edges (type 3 - type 3, behind the type-1 bead) complete no registered
    type tuple, so the topology manager spawns what it spawns without them."""
    last = {int(m): int(np.nonzero(scene["mol"] == m)[0][-1]) + 1 for m in np.unique(scene["mol"])}
    return np.array([(last[m], last[m + 1]) for m in sorted(last) if m % 5 == 4 and m + 1 in last], dtype=np.int64)


K14, RC14 = 1.5, 3.0


def make_list(g, lst, ids=None, hybrid=None, reg=()):
    """a list from its description (typed: [(key, params)], table: chem_table_create's arguments); hybrid = (lambda0, rate)"""
    h = g.list_create(lst["arity"], lst["kind"], lst.get("typed") is not None)
    if lst.get("typed") is not None:
        for key, p in lst["typed"]:
            g.list_set_params(h, list(p), types=key)
    elif lst.get("table") is not None:
        g.list_set_params(h, [g.table_create(*lst["table"])])
    else:
        g.list_set_params(h, list(lst["params"]))
    if hybrid is not None:
        (g.list_set_hybrid if lst["arity"] == 2 else g.list_set_hybrid_tuples)(h, *hybrid)
    if ids is not None and len(ids):
        g.list_add(h, ids)
    for r in reg:
        g.topology_register(h, list(r))
    return h


def build(scene, prec, lambda0=0.0, rate=0.125, hybrid=True, ang=ANG, dih=DIH, reg3=T.REG3, reg4=T.REG4, opts=None, engine=None, r1_rate=0.0,
          hybrid_bonds=None, coul14=False, retype=None, before_reactions=None):
    """Engine with the six lists of the module docstring (hybrid = False: lists 2 and 4 plain) and the reactions R0 (open), R1
    (rate r1_rate).  Returns engine, handles."""
    g = engine if engine is not None else Engine(device=0, precision=prec)
    for k, v in (opts or {}).items():
        g.set_option(k, v)
    spec = spec_of(scene)
    if coul14:
        spec["q"] = np.where(scene["types"] == 3, 0.5, -0.25)
    W.apply(spec, g, thermostat=False, reactions=False)
    hy = (lambda0, rate) if hybrid else None
    h = {}
    h["bond0"] = make_list(g, BOND0, scene["bonds0"])
    h["ang0"] = make_list(g, ANG0, scene["angles0"])
    h["h3"] = make_list(g, ang, hybrid=hy, reg=reg3)
    h["dih0"] = make_list(g, DIH0, scene["dihedrals0"])
    h["h4"] = make_list(g, dih, hybrid=hy, reg=reg4)
    h["rb"] = make_list(g, RBOND, hybrid=hybrid_bonds)
    if coul14:      # a 1-4 Coulomb list in the context: it runs the COUL family
        h["c14"] = g.list_create(2, "COULOMB_BOND")
        g.list_set_params(h["c14"], [K14, RC14])
        g.list_add(h["c14"], c14_pairs(scene))
    g.reaction_init(1, True, 0, 4)
    common = dict(delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=2, cutoff=T.REACT_CUT, bond_list=h["rb"],
                  intramolecular=True, intraresidual=True)
    h["R0"] = g.reaction_add(0, 1, rate=INF, **dict(common, **(dict(new_type_1=retype, new_mass_1=1.0) if retype is not None else {})))
    h["R1"] = g.reaction_add(2, 1, rate=r1_rate, **common)
    if before_reactions is not None:
        before_reactions(g, h)
    g.reactions_enable(True)
    return g, h


def event_rows(g):
    return [(int(e["step"]), int(e["id_a"]), int(e["id_b"]), int(e["reaction"])) for e in g.get_events()]


def canon(rows):
    return [min(tuple(r), tuple(r[::-1])) for r in np.asarray(rows).tolist()]


def expected(g, h, scene, lambda0, rate, reg3=T.REG3, reg4=T.REG4, forming=None, events=None, step=None):
    """the tuples the hybrid lists must hold, their birth steps from the event log, their lambda at the current step;
    returns {"h3": (ids, birth, lam), "h4": ...} in the order of the engine's lists"""
    forming = {h["R0"], h["R1"]} if forming is None else forming
    ev = [(s, a, b) for s, a, b, r in (event_rows(g) if events is None else events) if r in forming]
    t3, s3, t4, s4 = T.spawned(scene["bonds0"], ev, g.get_state("TYPE"), reg3, reg4)
    out = {}
    for key, rows, steps in (("h3", t3, s3), ("h4", t4, s4)):
        got = g.get_list(h[key])
        birth = dict(zip(canon(rows), steps.tolist()))
        assert sorted(canon(got)) == sorted(birth), key
        b = np.array([birth[c] for c in canon(got)], dtype=np.int64)
        out[key] = (got, b, T.ramp(lambda0, rate, g.step if step is None else step, b))
    return out


def oracle_on(make_oracle, scene, g, lists, q=None):
    o = make_oracle()
    s2 = dict(spec_of(scene), pos=g.get_state("POS"), vel=g.get_state("VEL"), types=g.get_state("TYPE"), state=g.get_state("STATE"),
              mass=g.get_state("MASS"), exclusions=g.get_exclusions(), lists=[dict(l, ids=np.asarray(l["ids"], np.int64)) for l in lists])
    W.apply(s2, o, thermostat=False, reactions=False)
    o.run(0)
    return o


def plain_lists(scene, g, h, with_rb=True):
    out = [dict(BOND0, ids=scene["bonds0"]), dict(ANG0, ids=scene["angles0"]), dict(DIH0, ids=scene["dihedrals0"])]
    return out + ([dict(RBOND, ids=g.get_list(h["rb"]))] if with_rb else [])


def check(g, h, scene, prec, make_oracle, exp, ang=ANG, dih=DIH, label="", extra=None):
    """forces and energies of g against oracle-without-the-hybrid-lists + the lambda-weighted tuple terms (extra: forces and
    {handle: energy} of further terms the oracle has not, added on top).  Returns (forces, hybrid part, full-strength part)."""
    g.run(0)
    x, ty = g.get_state("POS"), g.get_state("TYPE")
    l3, l4 = dict(ang, ids=exp["h3"][0]), dict(dih, ids=exp["h4"][0])
    assert T.geometry_ok(x, scene["box"], np.concatenate([exp["h3"][0], scene["angles0"]]), np.concatenate([exp["h4"][0], scene["dihedrals0"]]))
    lists = plain_lists(scene, g, h, with_rb=extra is None or h["rb"] not in extra[1])
    o = oracle_on(make_oracle, scene, g, lists)
    ref = T.reference(x, scene["box"], ty, [l3, l4], [exp["h3"][2], exp["h4"][2]])
    full = T.reference(x, scene["box"], ty, [l3, l4], [1.0, 1.0])
    Fref = o.get_state("FORCE") + ref["force"] + (extra[0] if extra else 0.0)
    fg = g.get_state("FORCE")
    og, oo = g.observe(), o.observe()
    err = rel_err(fg, Fref)
    print("%s prec %d: %d + %d hybrid tuples, force rel err %.3e, hybrid part %.3e of the largest force" %
          (label, prec, len(exp["h3"][0]), len(exp["h4"][0]), err, np.abs(ref["force"]).max() / np.abs(Fref).max()))
    print("   list energies: hybrid triples %.12e (ref %.12e), hybrid quadruples %.12e (ref %.12e)" %
          (og["epot_list"][h["h3"]], ref["energy"][0], og["epot_list"][h["h4"]], ref["energy"][1]))
    assert np.isfinite(fg).all()
    assert err < TOL_F[prec] and TOL_F[64] == TOL_F_BONDED[64]
    for key, k in (("h3", 0), ("h4", 1)):
        assert og["list_size"][h[key]] == len(exp[key][0])
        assert og["epot_list"][h[key]] == pytest.approx(ref["energy"][k], rel=TOL_EL[prec], abs=1e-12)
    for k, key in enumerate(("bond0", "ang0", "dih0", "rb")[:len(lists)]):
        assert og["epot_list"][h[key]] == pytest.approx(oo["epot_list"][k], rel=TOL_EL[prec], abs=1e-12)
    for hh, e in (extra[1].items() if extra else ()):
        assert og["epot_list"][hh] == pytest.approx(e, rel=TOL_EL[prec], abs=1e-12)
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=TOL_ELJ[prec])
    o.close()
    return fg, ref["force"], full["force"]


def lam_equal(g, h, exp):
    return all(np.array_equal(g.list_get_lambda(h[k]), exp[k][2]) for k in ("h3", "h4"))


def id_pairs(pairs):
    return sorted(tuple(p) for p in pairs)


# ---- 1: the ramp ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_ramp(base, make_oracle, prec):
    g, h = build(base, prec, 0.0, 0.25)
    try:
        assert len(g.list_get_lambda(h["h3"])) == 0 and len(g.list_get_lambda(h["h4"])) == 0
        g.run(1)
        assert sorted((a, b) for _, a, b, _ in event_rows(g)) == id_pairs(base["r0"])       # exactly the intended pairs react
        g.reactions_enable(False)
        exp = expected(g, h, base, 0.0, 0.25)
        assert len(exp["h3"][0]) == 303 and len(exp["h4"][0]) == 173 and np.all(exp["h3"][1] == 1) and np.all(exp["h4"][1] == 1)
        # the 1-3 / 1-4 exclusion acts from the moment the tuple is inserted, at lambda = 0
        want = {tuple(p) for p in base["exclusions"].tolist()} | {(min(a, b), max(a, b)) for a, b in base["r0"]}
        want |= {(min(t[0], t[-1]), max(t[0], t[-1])) for t in exp["h3"][0].tolist() + exp["h4"][0].tolist()}
        assert [tuple(p) for p in g.get_exclusions().tolist()] == sorted(want)
        assert np.array_equal(g.list_get_lambda(h["h3"]), np.zeros(303)) and np.array_equal(g.list_get_lambda(h["h4"]), np.zeros(173))
        fg, Fh, full = check(g, h, base, prec, make_oracle, exp, label="lambda 0")
        assert np.abs(Fh).max() == 0.0 and np.abs(full).max() > 0.2 * np.abs(fg).max()      # (at full strength they would show)
        for k, want in enumerate([0.25, 0.5, 0.75, 1.0, 1.0]):
            g.run(1)
            exp = expected(g, h, base, 0.0, 0.25)
            assert np.array_equal(exp["h3"][2], np.full(303, want)) and np.array_equal(exp["h4"][2], np.full(173, want)) and lam_equal(g, h, exp), k
            if want in (0.25, 0.75, 1.0):
                fg, Fh, full = check(g, h, base, prec, make_oracle, exp, label="lambda %.2f" % want)
                if want == 0.25:
                    assert rel_err(Fh, full) > 0.4                                          # (full strength is far outside the tolerance)
    finally:
        g.close()


@pytest.mark.parametrize("prec", [64, 32])
def test_split_run_is_bit_identical(base, prec):
    out = []
    for split in ((2, 3), (5,)):
        g, h = build(base, prec, 0.0, 0.125)
        g.run(1)
        g.reactions_enable(False)
        for k in split:
            g.run(k)
        out.append((g.get_state("POS"), g.get_state("VEL"), g.list_get_lambda(h["h3"]), g.list_get_lambda(h["h4"])))
        g.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert np.abs(out[0][1]).max() > 0 and np.all(out[0][2] == 0.625)


# ---- 2: two cohorts in one list ---------------------------------------------------------------------------------------------

def two_cohorts(scene, prec, rate=0.125, wait=3, lambda0=0.0, **kw):
    """R0 at step 1, R1 opened after `wait` more steps: tuples of birth 1 and 2 + wait in one list"""
    g, h = build(scene, prec, lambda0, rate, **kw)
    g.run(1 + wait)
    g.reaction_set_rate(h["R1"], INF)
    g.run(1)
    return g, h


@pytest.mark.parametrize("prec", [64, 32])
def test_two_cohorts_in_one_list(base, make_oracle, prec):
    g, h = two_cohorts(base, prec)
    try:
        g.run(1)                                                       # step 6: cohort 1 at 5/8, cohort 2 at 1/8
        ev = event_rows(g)
        assert sorted((a, b) for s, a, b, r in ev if r == h["R0"]) == id_pairs(base["r0"]) and {s for s, _, _, r in ev if r == h["R0"]} == {1}
        assert sorted((a, b) for s, a, b, r in ev if r == h["R1"]) == id_pairs(base["r1"]) and {s for s, _, _, r in ev if r == h["R1"]} == {5}
        exp = expected(g, h, base, 0.0, 0.125)
        for key, n1, n5 in (("h3", 303, 172), ("h4", 173, 129)):
            assert sorted(set(exp[key][2].tolist())) == [0.125, 0.625] and (exp[key][2] == 0.625).sum() == n1 and (exp[key][2] == 0.125).sum() == n5
        assert lam_equal(g, h, exp)
        # an angle spawned at step 5 around a bond of step 1 (the C chains' (a, b, c)) has its own birth: its centre b then
        # holds triples of both cohorts
        old = {(min(a, b), max(a, b)) for s, a, b, r in ev if s == 1}
        late = [t for t, b in zip(exp["h3"][0].tolist(), exp["h3"][1].tolist()) if b == 5 and ((min(t[0], t[1]), max(t[0], t[1])) in old or (min(t[1], t[2]), max(t[1], t[2])) in old)]
        assert len(late) == 43
        check(g, h, base, prec, make_oracle, exp, label="two cohorts")
    finally:
        g.close()


# ---- 3: every kernel path ---------------------------------------------------------------------------------------------------

def _swap(reg, a, b):
    return [tuple(b if t == a else t for t in key) for key in reg]


REG3_RETYPED = T.REG3 + [k for k in _swap(T.REG3, 0, 4) if k not in T.REG3]
REG4_RETYPED = T.REG4 + [k for k in _swap(T.REG4, 0, 4) if k not in T.REG4]


def _by_key(reg, fun):
    """parameters per registered type tuple; a tuple and its mirror image ((1, 2, 3) and (3, 2, 1) are both registered) get the
    same ones, so that it does not matter which of the two an entry is resolved by"""
    canon_keys = sorted({min(k, k[::-1]) for k in reg})
    return [(k, fun(canon_keys.index(min(k, k[::-1])))) for k in reg]


PATHS = {
    "fused": dict(),                                                                      # full work-list kernel, fused rebuild
    "unfused": dict(opts={"fused_rebuild": 0}),                                           # k_bonded_prep of its own launch
    "no_tiles": dict(opts={"tiles": 0}),                                                  # per-particle k_bonded_hyb<.., false>
    "dd_self": dict(opts={"dd_self": 1}),
    # lists by types; R0 turns its type-0 bead into type 4, so the tuples are matched and their slots resolved with the new type
    "by_types": dict(retype=4, reg3=REG3_RETYPED, reg4=REG4_RETYPED,
                     ang=dict(arity=3, kind="ANG_COSINE", typed=_by_key(REG3_RETYPED, lambda i: [3.0 + 0.25 * i, 1.5 + 0.05 * i])),
                     dih=dict(arity=4, kind="DIH_HARMONIC", typed=_by_key(REG4_RETYPED, lambda i: [3.0 + 0.5 * i, -1.0 + 0.4 * i]))),
    "tabulated": dict(ang=dict(arity=3, kind="ANG_TABULATED", table=TAB_ANG), dih=dict(arity=4, kind="DIH_TABULATED", table=TAB_DIH)),
    "rb": dict(ang=dict(arity=3, kind="ANG_COSINE", params=[3.0, 1.7]), dih=dict(arity=4, kind="DIH_RB", params=[0.5, -0.3, 0.2, 0.1, -0.1, 0.05])),
    "dih_harmonic": dict(dih=dict(arity=4, kind="DIH_HARMONIC", params=[4.0, 175 * math.pi / 180])),
    "coul14": dict(coul14=True),                                                          # the COUL family carries the lambda code
    "hybrid_pairs": dict(hybrid_bonds=(0.0, 0.0625)),                                     # a hybrid pair list beside the hybrid tuple lists
}


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_kernel_path(base, make_oracle, path, prec):
    cfg = PATHS[path]
    kw = {k: cfg[k] for k in ("ang", "dih", "reg3", "reg4", "opts", "retype", "coul14", "hybrid_bonds") if k in cfg}
    g, h = two_cohorts(base, prec, rate=0.125, wait=1, **kw)            # births 1 and 3
    try:
        g.run(2)                                                         # step 5: lambda 1/2 and 1/4
        exp = expected(g, h, base, 0.0, 0.125, cfg.get("reg3", T.REG3), cfg.get("reg4", T.REG4))
        assert all(sorted(set(exp[k][2].tolist())) == [0.25, 0.5] for k in ("h3", "h4")) and lam_equal(g, h, exp)
        assert len(exp["h3"][0]) == 475 and len(exp["h4"][0]) == 302
        if "retype" in cfg:
            assert (g.get_state("TYPE") == 4).sum() == len(base["r0"])
        extra = None
        x = g.get_state("POS")
        if path == "coul14":
            import coulomb14_ref as C14
            p14 = c14_pairs(base)
            q = np.where(base["types"] == 3, 0.5, -0.25)
            F14, e14 = C14.terms(x, base["box"], q, p14 - 1, K14, RC14)
            assert len(p14) == 43 and np.abs(F14).max() > 1e-3 * np.abs(g.get_state("FORCE")).max() and e14 != 0.0
            assert np.array_equal(g.get_state("CHARGE"), q)
            extra = (F14, {h["c14"]: e14})
        if path == "hybrid_pairs":
            bonds = g.get_list(h["rb"])
            lamb = H.ramp(0.0, 0.0625, g.step, H.births(event_rows(g), {h["R0"], h["R1"]}, bonds))
            assert sorted(set(lamb.tolist())) == [0.125, 0.25] and np.array_equal(g.list_get_lambda(h["rb"]), lamb)
            Fb, eb = H.bond_terms(x, base["box"], bonds - 1, lamb, H.harmonic(*RBOND["params"]))
            extra = (Fb, {h["rb"]: eb})
        fg, Fh, full = check(g, h, base, prec, make_oracle, exp, ang=cfg.get("ang", ANG), dih=cfg.get("dih", DIH), label=path, extra=extra)
        assert rel_err(Fh, full) > 0.4                                   # (full strength is far outside the tolerance)
    finally:
        g.close()


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("P", [2, 3])
def test_slabs(make_gpu, make_oracle, P, prec):
    scene = T.scene(box=(14.0, 14.0, 14.0 * P))
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        _, h = build(scene, prec, 0.0, 0.125, engine=g)
        g.run(2)
        g.reaction_set_rate(h["R1"], INF)
        g.run(1)                                                          # births 1 and 3
        g.run(2)                                                          # step 5
        g.run(0)
        return dict(x=g.get_state("POS"), f=g.get_state("FORCE"), lam=[g.list_get_lambda(h[k]) for k in ("h3", "h4")],
                    lists=[g.get_list(h[k]) for k in ("h3", "h4", "rb")], h=h, ev=event_rows(g), ob=g.observe(), ty=g.get_state("TYPE"), ex=g.get_exclusions())
    out = _run_ranks(P, rank)
    for r in range(1, P):
        assert np.array_equal(out[0]["x"], out[r]["x"])
        assert all(np.array_equal(a, b) for a, b in zip(out[0]["lam"] + out[0]["lists"], out[r]["lam"] + out[r]["lists"]))   # every rank: the same lambda
    h = out[0]["h"]
    z = scene["pos"][:, 2]
    zq = z[out[0]["lists"][1] - 1]                                        # quadruples across every slab boundary, the periodic one included
    for cut in 14.0 * np.arange(1, P):
        assert (((zq - cut).min(1) < 0) & ((zq - cut).max(1) > 0) & (np.ptp(zq, axis=1) < 7.0)).sum() >= 1
    assert (np.ptp(zq, axis=1) > 7.0).sum() >= 1
    ev = [(s, a, b) for s, a, b, r in out[0]["ev"]]
    t3, s3, t4, s4 = T.spawned(scene["bonds0"], ev, out[0]["ty"], T.REG3, T.REG4)
    lams = []
    for rows, steps, got, lam in ((t3, s3, out[0]["lists"][0], out[0]["lam"][0]), (t4, s4, out[0]["lists"][1], out[0]["lam"][1])):
        birth = dict(zip(canon(rows), steps.tolist()))
        assert sorted(canon(got)) == sorted(birth)
        want = T.ramp(0.0, 0.125, 5, np.array([birth[c] for c in canon(got)]))
        assert sorted(set(want.tolist())) == [0.25, 0.5] and np.array_equal(lam, want)
        lams.append(want)
    o = make_oracle()
    lists = [dict(BOND0, ids=scene["bonds0"]), dict(ANG0, ids=scene["angles0"]), dict(DIH0, ids=scene["dihedrals0"]), dict(RBOND, ids=out[0]["lists"][2])]
    W.apply(dict(spec_of(scene), pos=out[0]["x"], exclusions=out[0]["ex"], lists=lists), o, thermostat=False, reactions=False)
    o.run(0)
    l3, l4 = dict(ANG, ids=out[0]["lists"][0]), dict(DIH, ids=out[0]["lists"][1])
    ref = T.reference(out[0]["x"], scene["box"], out[0]["ty"], [l3, l4], lams)
    full = T.reference(out[0]["x"], scene["box"], out[0]["ty"], [l3, l4], [1.0, 1.0])
    Fref = o.get_state("FORCE") + ref["force"]
    for r in range(P):
        print("rank %d of %d, prec %d: force rel err %.3e" % (r, P, prec, rel_err(out[r]["f"], Fref)))
        assert rel_err(out[r]["f"], Fref) < TOL_F[prec]
        assert out[r]["ob"]["epot_list"][h["h3"]] == pytest.approx(ref["energy"][0], rel=TOL_EL[prec])
        assert out[r]["ob"]["epot_list"][h["h4"]] == pytest.approx(ref["energy"][1], rel=TOL_EL[prec])
    assert rel_err(ref["force"], full["force"]) > 0.4


# ---- 4: lambda0 = 1 is a plain list -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_lambda0_one_is_bit_identical_to_plain_lists(base, prec):
    out = []
    for hybrid in (True, False):
        g, h = two_cohorts(base, prec, rate=0.0, wait=1, lambda0=1.0, hybrid=hybrid)
        g.run(0)
        f = g.get_state("FORCE")
        e = g.observe()["epot_list"]
        g.run(20)
        out.append((f, g.get_state("POS"), g.get_state("VEL"), e, g.list_get_lambda(h["h3"]), g.list_get_lambda(h["h4"]), g.get_list(h["h3"]), g.get_list(h["h4"])))
        g.close()
    assert np.all(out[0][4] == 1.0) and np.all(out[1][4] == 1.0) and len(out[0][4]) == 475 and len(out[0][5]) == 302
    assert np.array_equal(out[0][6], out[1][6]) and np.array_equal(out[0][7], out[1][7])
    assert np.array_equal(out[0][0], out[1][0]) and np.abs(out[0][0]).max() > 5.0
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    # (k_list_sums adds in an order that depends on the entry table, and a hybrid triple is two entries wide: equal to rounding)
    assert out[0][3] == pytest.approx(out[1][3], rel=1e-13)


# ---- 5: an entry at lambda = 0 on a near-degenerate member --------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_lambda_zero_entry_contributes_nothing_where_the_term_is_not_finite(base, make_oracle, prec):
    """Three A chains are straightened by hand before the run: n, a, b exactly collinear (the bending term divides by
    sin(theta), the dihedral's normal vanishes).  At lambda = 0 their tuples must contribute exactly nothing: every force is
    finite and equals the oracle without the hybrid lists; list_add'ed at rate 0, lambda stays 0."""
    scene = dict(base, pos=base["pos"].copy())
    box = np.asarray(scene["box"])
    moved = []
    for a, b in [p for p in scene["r0"] if scene["mol"][p[0] - 1] in (0, 4, 5)]:      # three A chains: n a | b m, ids in chain order
        n = a - 1
        assert scene["types"][n - 1] == 3 and scene["mol"][n - 1] == scene["mol"][b - 1] and (scene["mol"] == scene["mol"][b - 1]).sum() == 4
        d = scene["pos"][b - 1] - scene["pos"][a - 1]
        d -= box * np.rint(d / box)
        scene["pos"][n - 1] = scene["pos"][a - 1] - (0.8 / np.linalg.norm(d)) * d       # n - a - b on one line: theta = pi exactly up to rounding
        moved.append((n, a, b))
    g, h = build(scene, prec, 0.0, 0.0)
    try:
        g.run(1)
        g.reactions_enable(False)
        assert np.all(g.list_get_lambda(h["h3"]) == 0.0) and np.all(g.list_get_lambda(h["h4"]) == 0.0) and len(g.get_list(h["h3"])) == 303
        assert all(list(t) in g.get_list(h["h3"]).tolist() or list(t[::-1]) in g.get_list(h["h3"]).tolist() for t in moved)
        g.run(3)
        g.run(0)
        fg = g.get_state("FORCE")
        assert np.isfinite(fg).all() and np.isfinite(g.get_state("POS")).all()
        o = oracle_on(make_oracle, scene, g, plain_lists(scene, g, h))
        assert rel_err(fg, o.get_state("FORCE")) < TOL_F[prec]
        og = g.observe()
        assert og["epot_list"][h["h3"]] == 0.0 and og["epot_list"][h["h4"]] == 0.0
        assert np.all(g.pressure_tensor()["virial_list"][[h["h3"], h["h4"]]] == 0.0)
    finally:
        g.close()


# ---- 6: pressure and pressure tensor -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_pressure_and_tensor_scale_with_lambda(base, prec):
    """One shared lambda = 3/8 and kinds linear in K (harmonic angle, cosine dihedral): the hybrid lists' virial and tensor part
    equal those of plain lists with K lambda at the same configuration; tolerance of tests/test_gpu_pressure.py between paths."""
    lam = 0.375
    g, h = build(base, prec, 0.0, 0.125)
    p = None
    try:
        g.run(1)
        g.reactions_enable(False)
        g.run(3)                                                          # step 4: lambda = 3/8
        assert np.all(g.list_get_lambda(h["h3"]) == lam) and np.all(g.list_get_lambda(h["h4"]) == lam)
        x, v = g.get_state("POS"), g.get_state("VEL")
        pg, tg = g.pressure(), g.pressure_tensor()
        p = Engine(device=0, precision=prec)
        sc = dict(base, pos=x, vel=v)
        W.apply(dict(spec_of(sc), exclusions=g.get_exclusions()), p, thermostat=False, reactions=False)
        hp = {}
        for key, lst, ids in (("bond0", BOND0, base["bonds0"]), ("ang0", ANG0, base["angles0"]), ("h3", dict(ANG, params=[ANG["params"][0] * lam, ANG["params"][1]]), g.get_list(h["h3"])),
                              ("dih0", DIH0, base["dihedrals0"]), ("h4", dict(DIH, params=[DIH["params"][0] * lam] + DIH["params"][1:]), g.get_list(h["h4"])),
                              ("rb", RBOND, g.get_list(h["rb"]))):
            hp[key] = make_list(p, lst, ids)
        p.run(0)
        pp, tp = p.pressure(), p.pressure_tensor()
        for key in ("h3", "h4"):
            a, b = tg["virial_list"][h[key]], tp["virial_list"][hp[key]]
            print("prec %d %s tensor part: largest component %.3e, difference %.3e" % (prec, key, np.abs(b).max(), np.abs(a - b).max()))
            assert np.abs(b).max() > 1.0 and np.abs(a - b).max() <= TOL_P[prec] * np.abs(b).max()
            assert pg["virial_list"][h[key]] == 0.0 and pp["virial_list"][hp[key]] == 0.0      # angles alone: no scalar virial, whatever lambda
        for key in ("bond0", "ang0", "dih0", "rb"):
            assert np.abs(tg["virial_list"][h[key]] - tp["virial_list"][hp[key]]).max() <= TOL_P[prec] * np.abs(tp["virial_list"][hp[key]]).max()
        assert pg["pressure"] == pytest.approx(pp["pressure"], rel=TOL_P[prec])
    finally:
        g.close()
        if p is not None:
            p.close()


# ---- 7: dissociation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_dissociation_takes_the_tuples_and_their_births(base, make_oracle, prec):
    """Mid-ramp, with the association closed, a dissociation reaction breaks about half of the 0 - 1 bonds (one Philox draw per
    bond, p = 1/2); later the association is open again and the broken pairs bond anew: their tuples start at lambda0."""
    rate = 0.0625

    def add_dissociation(g, h):
        h["dz"] = g.dissociation_add(0, 1, -1, -1, 1, 2, 1, 3, diss_rate=0.0, cutoff=0.0, bond_list=h["rb"])
    g, h = build(base, prec, 0.0, rate, before_reactions=add_dissociation)
    try:
        dz = h["dz"]
        g.run(2)
        g.reaction_set_rate(h["R1"], INF)
        g.run(1)                                                          # births 1 (R0) and 3 (R1)
        g.reaction_set_rate(h["R1"], 0.0)
        g.run(1)                                                          # step 4
        before = {k: [tuple(t) for t in g.get_list(h[k]).tolist()] for k in ("h3", "h4")}
        exp0 = expected(g, h, base, 0.0, rate)
        g.reaction_set_rate(h["R0"], 0.0)
        g.reaction_set_rate(dz, 0.5 / base["dt"])                         # p = diss_rate * dt * interval = 1/2
        g.run(1)                                                          # step 5: bonds break, none forms
        g.reaction_set_rate(dz, 0.0)
        ev = event_rows(g)
        broken = sorted((min(a, b), max(a, b)) for s, a, b, r in ev if r == dz)
        assert {s for s, _, _, r in ev if r == dz} == {5} and 50 < len(broken) < 125
        assert set(broken) <= {(min(a, b), max(a, b)) for a, b in base["r0"]}
        gone = set(broken)
        for key in ("h3", "h4"):
            left = [t for t in before[key] if not any((min(t[k], t[k + 1]), max(t[k], t[k + 1])) in gone for k in range(len(t) - 1))]
            got = [tuple(t) for t in g.get_list(h[key]).tolist()]
            assert got == left and 0 < len(left) < len(before[key])                          # order of the survivors kept
            keep = [k for k, t in enumerate(before[key]) if t in set(left)]
            want = T.ramp(0.0, rate, 5, exp0[key][1][keep])                                  # the survivors' own births, one step on
            assert np.array_equal(g.list_get_lambda(h[key]), want) and sorted(set(exp0[key][1][keep].tolist())) == [1, 3]
        # reference: the surviving tuples with their births
        exp = {key: (g.get_list(h[key]), None, g.list_get_lambda(h[key])) for key in ("h3", "h4")}
        check(g, h, base, prec, make_oracle, exp, label="after the break")
        g.reaction_set_rate(h["R0"], INF)
        g.run(1)                                                          # step 6: the broken pairs bond again
        g.run(2)                                                          # step 8
        assert sorted(tuple(p) for p in g.get_list(h["rb"]).tolist()) == id_pairs(base["r0"] + base["r1"])
        # births: the last bond-forming event of the pair that spawned the tuple; restated by replaying the log in two parts
        again = [(s, a, b) for s, a, b, r in event_rows(g) if r in (h["R0"], h["R1"])]
        for key, n in (("h3", 475), ("h4", 302)):
            lam = g.list_get_lambda(h[key])
            rows = g.get_list(h[key]).tolist()
            assert len(rows) == n and sorted(set(lam.tolist())) == [2 * rate, 5 * rate, 7 * rate]    # a tuple spawned again starts at lambda0
            last = {}
            for s, a, b in again:
                last[(min(a, b), max(a, b))] = s
            for t, l in zip(rows, lam.tolist()):
                # a tuple is as old as the youngest bond among its consecutive pairs that a reaction made
                born = max(last.get((min(t[k], t[k + 1]), max(t[k], t[k + 1])), 0) for k in range(len(t) - 1))
                assert l == rate * (8 - born), (t, l, born)
        exp = {key: (g.get_list(h[key]), None, g.list_get_lambda(h[key])) for key in ("h3", "h4")}
        check(g, h, base, prec, make_oracle, exp, label="bonded again")
    finally:
        g.close()


# ---- 8: checkpoint ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_checkpoint_mid_ramp_continues_bit_for_bit(base, prec):
    g, h = two_cohorts(base, prec, rate=0.0625, wait=1)                  # births 1 and 3
    g2 = p = None
    try:
        g.run(2)                                                          # step 5: mid-ramp
        blob = g.checkpoint_save()
        g2, h2 = build(base, prec, 0.0, 0.0625)
        g2.reaction_set_rate(h2["R1"], INF)
        g2.checkpoint_load(blob)
        assert all(np.array_equal(g.list_get_lambda(h[k]), g2.list_get_lambda(h2[k])) for k in ("h3", "h4"))
        assert sorted(set(g2.list_get_lambda(h2["h3"]).tolist())) == [0.125, 0.25]
        for e in (g, g2):
            e.run(7)
        assert np.array_equal(g.get_state("POS"), g2.get_state("POS")) and np.array_equal(g.get_state("VEL"), g2.get_state("VEL"))
        assert np.array_equal(g.get_state("FORCE"), g2.get_state("FORCE"))
        assert all(np.array_equal(g.list_get_lambda(h[k]), g2.list_get_lambda(h2[k])) for k in ("h3", "h4"))
        assert sorted(set(g2.list_get_lambda(h2["h4"]).tolist())) == [0.5625, 0.6875]
        p, hp = build(base, prec, hybrid=False)                          # set up without the hybrid flag: the fingerprint differs
        p.reaction_set_rate(hp["R1"], INF)
        with pytest.raises(ChemError) as ex:
            p.checkpoint_load(blob)
        assert ex.value.code == _capi.EINVAL and "hybrid" in str(ex.value)
    finally:
        for e in (g, g2, p):
            if e is not None:
                e.close()


# ---- 9: refusals through the C ABI --------------------------------------------------------------------------------------------

def test_set_hybrid_tuples_refusals(base, make_gpu):
    g = make_gpu(64)
    W.apply(spec_of(base), g, thermostat=False, reactions=False)
    pair = make_list(g, BOND0)
    full3 = make_list(g, ANG0, base["angles0"])
    e3, e4 = make_list(g, ANG), make_list(g, dict(arity=4, kind="DIH_TABULATED", table=TAB_DIH))
    typed = make_list(g, dict(arity=3, kind="ANG_COSINE", typed=[((3, 0, 1), [3.0, 1.5])]))
    with pytest.raises(ChemError, match="chem_list_set_hybrid") as ex:
        g.list_set_hybrid_tuples(pair, 0.0, 0.1)                         # arity 2: the message points to the other call
    assert ex.value.code == _capi.EINVAL
    for args, code in (((e3, -0.1, 0.1), _capi.EINVAL), ((e3, 1.5, 0.1), _capi.EINVAL), ((e4, 0.5, -1.0), _capi.EINVAL), ((e4, float("nan"), 0.1), _capi.EINVAL),
                       ((e3, 0.5, float("inf")), _capi.EINVAL), ((e3, 0.5, float("nan")), _capi.EINVAL), ((full3, 0.0, 0.1), _capi.ESTATE), ((99, 0.0, 0.1), _capi.EINVAL),
                       ((-1, 0.0, 0.1), _capi.EINVAL)):
        with pytest.raises(ChemError) as ex:
            g.list_set_hybrid_tuples(*args)
        assert ex.value.code == code, args
    for hh in (e3, e4):                                                   # chem_list_set_hybrid stays a pair-list call
        with pytest.raises(ChemError) as ex:
            g.list_set_hybrid(hh, 0.0, 0.1)
        assert ex.value.code == _capi.EINVAL
    for hh in (e3, e4, typed):
        g.list_set_hybrid_tuples(hh, 0.0, 0.0)
        g.list_set_hybrid_tuples(hh, 0.5, 0.03125)                       # again on an empty list: allowed
        assert len(g.list_get_lambda(hh)) == 0
    # list_add at step 0, then a run: the entries' birth is the step of the call
    g.list_add(e3, base["angles0"][:5])
    g.run(4)
    g.list_add(e3, base["angles0"][5:8])
    g.run(8)
    assert np.array_equal(g.list_get_lambda(e3), np.array([0.5 + 12 / 32] * 5 + [0.5 + 8 / 32] * 3))
    assert np.array_equal(g.list_get_lambda(full3), np.ones(len(base["angles0"])))
    with pytest.raises(ChemError) as ex:
        g.list_set_hybrid_tuples(e3, 0.0, 0.1)                           # no longer empty
    assert ex.value.code == _capi.ESTATE


# ---- 10: the espressopp shim, end to end ----------------------------------------------------------------------------------------

def test_shim_end_to_end(base):
    """The system assembled from the shim's objects the way the driver assembles it with --t_hybrid_angle 8 --t_hybrid_dihedral 8
    (plain dynamic lists for the tuples of the start, empty hybrid Types lists with the same potentials that the topology manager
    spawns into, registered with rate 1/8, res_ftl_0 / res_fql_0 monitored) against the same run assembled by hand on the engine."""
    from chemlab_amd import espp
    box = tuple(base["box"])
    prev = espp._factory[0]
    ang_typed = [(k, ANG["params"]) for k in T.REG3]
    dih_typed = [(k, DIH["params"]) for k in T.REG4]
    try:
        espp.set_engine_factory(lambda: Engine(device=0, precision=64))
        system = espp.System()
        system.rng = espp.esutil.RNG(4)
        system.skin = T.SCENE_SKIN
        system.bc = espp.bc.OrthorhombicBC(system.rng, box)
        system.storage = espp.storage.DomainDecomposition(system, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), T.SCENE_RC, T.SCENE_SKIN))
        integrator = espp.integrator.VelocityVerlet(system)
        integrator.dt = base["dt"]
        plist = [[int(i + 1), int(base["types"][i]), espp.Real3D(*base["pos"][i]), 1.0] for i in range(base["n"])]
        system.storage.addParticles(plist, "id", "type", "pos", "mass")
        system.storage.decompose()
        excl = espp.DynamicExcludeList(integrator, [tuple(p) for p in base["exclusions"].tolist()])
        vl = espp.VerletList(system, cutoff=T.SCENE_RC, exclusionlist=excl)
        lj = espp.interaction.VerletListLennardJones(vl)
        for t1, t2, eps, sig, rc in LJ:
            lj.setPotential(type1=t1, type2=t2, potential=espp.interaction.LennardJones(eps, sig, rc))
        system.addInteraction(lj, "lj")
        fpl0 = espp.FixedPairList(system.storage)
        fpl0.addBonds([tuple(p) for p in base["bonds0"].tolist()])
        system.addInteraction(espp.interaction.FixedPairListHarmonic(system, fpl0, espp.interaction.Harmonic(*BOND0["params"])), "bonds")
        ftl0 = espp.FixedTripleList(system.storage)
        ftl0.addTriples([tuple(p) for p in base["angles0"].tolist()])
        system.addInteraction(espp.interaction.FixedTripleListAngularHarmonic(system, ftl0, espp.interaction.AngularHarmonic(*ANG0["params"])), "angle_dynamic")
        ftl = espp.FixedTripleListLambda(system.storage, 0.0)
        ia = espp.interaction.FixedTripleListTypesLambdaAngularHarmonic(system, ftl)
        for k, p in ang_typed:
            ia.setPotential(*(k + (espp.interaction.AngularHarmonic(*p),)))
        system.addInteraction(ia, "angle_hybrid")
        fql0 = espp.FixedQuadrupleList(system.storage)
        fql0.addQuadruples([tuple(p) for p in base["dihedrals0"].tolist()])
        system.addInteraction(espp.interaction.FixedQuadrupleListDihedralHarmonic(system, fql0, espp.interaction.DihedralHarmonic(*DIH0["params"])), "dihedral_dynamic")
        fql = espp.FixedQuadrupleListLambda(system.storage, 0.0)
        iq = espp.interaction.FixedQuadrupleListTypesLambdaDihedralHarmonicNCos(system, fql)
        for k, p in dih_typed:
            iq.setPotential(*(k + (espp.interaction.DihedralHarmonicNCos(K=p[0], phi0=p[1], multiplicity=int(p[2])),)))
        system.addInteraction(iq, "dihedral_hybrid")
        fpl = espp.FixedPairList(system.storage)
        system.addInteraction(espp.interaction.FixedPairListHarmonic(system, fpl, espp.interaction.Harmonic(*RBOND["params"])), "fpl_0")
        ext = espp.integrator.FixedListDynamicResolution(system)
        ext.register_triple_list(ftl, 1.0 / 8)
        ext.register_quadruple_list(fql, 1.0 / 8)
        integrator.addExtension(ext)
        tm = espp.integrator.TopologyManager(system)
        for k in T.REG3:
            tm.register_triplet(ftl, *k)
        for k in T.REG4:
            tm.register_quadruplet(fql, *k)
        for lst, obs in ((ftl0, excl.observe_triple), (ftl, excl.observe_triple), (fql0, excl.observe_quadruple), (fql, excl.observe_quadruple)):
            obs(lst)
        ar = espp.integrator.ChemicalReaction(system, vl, system.storage, tm, 1)
        r = espp.integrator.Reaction(type_1=0, type_2=1, delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=2,
                                     rate=INF, fpl=fpl, cutoff=T.REACT_CUT)
        r.intramolecular = r.intraresidual = True
        ar.nearest_mode = True
        ar.add_reaction(r)
        integrator.addExtension(ar)
        r3, r4 = espp.analysis.ResolutionFixedTripleList(system, ftl), espp.analysis.ResolutionFixedQuadrupleList(system, fql)
        mon = espp.analysis.SystemMonitor(system, integrator, None)
        mon.add_observable("res_ftl_0", r3)
        mon.add_observable("res_fql_0", r4)
        mon.add_observable("angle_hybrid", espp.analysis.PotentialEnergy(system, ia))
        mon.add_observable("dihedral_hybrid", espp.analysis.PotentialEnergy(system, iq))
        assert r3.compute() == 0.0 and r4.compute() == 0.0               # empty lists
        eng = system.engine
        # by hand: typed hybrid lists with the same potentials (lists 2 and 4 of build()), R0 alone
        g, h = build(base, 64, 0.0, 1.0 / 8, ang=dict(arity=3, kind="ANG_HARMONIC", typed=ang_typed), dih=dict(arity=4, kind="DIH_NCOS", typed=dih_typed))
        rows = []
        for want in (0.0, 0.125, 0.25, 0.375):
            integrator.run(1)
            g.run(1)
            assert r3.compute() == want and r4.compute() == want and ftl.getAllLambda() == [want] * 303 and fql.getAllLambda() == [want] * 173
            mon.perform_action()
            names, row = mon.last
            assert names == ["step", "time", "res_ftl_0", "res_fql_0", "angle_hybrid", "dihedral_hybrid"] and row[2] == want and row[3] == want
            og = g.observe()
            assert row[4] == pytest.approx(og["epot_list"][h["h3"]], rel=TOL_EL[64], abs=1e-12) and row[5] == pytest.approx(og["epot_list"][h["h4"]], rel=TOL_EL[64], abs=1e-12)
            rows.append(row)
        assert rows[0][4] == 0.0 and rows[-1][4] > 1.0 and rows[-1][5] > 1.0
        assert sorted(ftl.getAllTriples()) == sorted(tuple(t) for t in g.get_list(h["h3"]).tolist()) and len(ftl0.getAllTriples()) == len(base["angles0"])
        # (the two set-ups rebuild their neighbour lists at different steps: equal to rounding, not bit for bit)
        assert rel_err(eng.get_state("POS"), g.get_state("POS")) < 1e-12 and rel_err(eng.get_state("FORCE"), g.get_state("FORCE")) < TOL_F[64]
        assert [tuple(p) for p in eng.get_exclusions().tolist()] == [tuple(p) for p in g.get_exclusions().tolist()]
        eng.close()
        g.close()
    finally:
        espp.set_engine_factory(prev)


# ---- 11: the driver, end to end ---------------------------------------------------------------------------------------------------

ANG_TYPES = {(0, 0, 0): (10.0, 120.0), (0, 0, 1): (10.0, 120.0), (0, 0, 2): (8.0, 115.0), (1, 0, 0): (10.0, 120.0), (2, 0, 0): (8.0, 115.0)}   # K = k / 2, theta0 in degrees
DIH_TYPES = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2), (1, 0, 0, 0), (2, 0, 0, 0)]                                                            # all K 2, phi0 20 degrees, n 3


def by_hand(prec, particles, n_hyb):
    """The engine calls of the driver's run on the staged fixture, written out: tests/golden/chain_growth_catalytic (types A, B,
    D = 0, 1, 2; LJ 1, 1 between A-A, B-B, B-D, D-D; Langevin; four reactions, two of them virtual) with the angle and dihedral
    types of tests/golden/hybrid_tuples/bonded_types.top, reaction interval 5 and rate 100 (stage_driver), --t_hybrid_angle and
    --t_hybrid_dihedral = n_hyb.  particles: the arguments of set_particles as the readers produced them.  Yields the engine
    after every 5 steps (the driver's integrator step), 12 times; the first value is the dict of handles."""
    g = Engine(device=0, precision=prec)
    g.set_box([12.111984] * 3)
    g.set_dt(0.005)
    g.set_particles(*particles[0], **particles[1])
    g.set_cutoff(2.5, 0.3)
    h = dict(rb=g.list_create(2, "HARMONIC", False))
    g.list_set_params(h["rb"], [30.0, 0.97])
    g.set_option("count_intra_inter", 1)
    for a, b in ((0, 0), (1, 1), (1, 2), (2, 2)):
        g.nb_lj(a, b, 1.0, 1.0, 2.5, True)

    h["ad"] = g.list_create(3, "ANG_HARMONIC", True)
    for k, (K, th) in ANG_TYPES.items():
        g.list_set_params(h["ad"], [K, th * math.pi / 180], types=k)
    h["dd"] = g.list_create(4, "DIH_NCOS", True)
    for k in DIH_TYPES:
        g.list_set_params(h["dd"], [2.0, 20.0 * math.pi / 180, 3.0], types=k)
    g.thermostat_langevin(0.5, 5.0, 12345)
    g.thermostat_langevin_types([])
    h["ah"] = g.list_create(3, "ANG_HARMONIC", True)
    g.list_set_hybrid_tuples(h["ah"], 0.0, 1.0 / n_hyb)
    for k, (K, th) in ANG_TYPES.items():
        g.list_set_params(h["ah"], [K, th * math.pi / 180], types=k)
    h["dh"] = g.list_create(4, "DIH_NCOS", True)
    g.list_set_hybrid_tuples(h["dh"], 0.0, 1.0 / n_hyb)
    for k in DIH_TYPES:
        g.list_set_params(h["dh"], [2.0, 20.0 * math.pi / 180, 3.0], types=k)
    for k in ANG_TYPES:
        g.topology_register(h["ah"], list(k))
    for k in DIH_TYPES:
        g.topology_register(h["dh"], list(k))
    yield g, h
    for chunk in range(12):
        if chunk == 2:                                    # --start_ar=10
            g.reaction_init(5, True, 0, 12345)
            rx = dict(min_cutoff=0.0, intramolecular=False, intraresidual=False, active=True)
            g.reaction_add(0, 1, 2, 0, 1, 2, 1, 2, 100.0, 1.2, bond_list=-1, is_virtual=True, new_type_2=2, new_mass_2=1.0, new_q_2=0.0, **rx)      # A(1,2) + B(1,2) -> A(2):D(0)
            g.reaction_add(0, 0, 1, 1, 3, 4, 1, 2, 100.0, 1.2, bond_list=h["rb"], is_virtual=False, **rx)                                            # A(3,4) + A(1,2) -> A(1):A(1)
            g.reaction_add(0, 0, 1, 1, 2, 3, 1, 2, 100.0, 1.2, bond_list=h["rb"], is_virtual=False, **rx)                                            # A(2,3) + A(1,2) -> A(1):A(1)
            g.reaction_add(0, 2, -2, 0, 3, 4, 1, 2, 100.0, 1.2, bond_list=-1, is_virtual=True, new_type_2=1, new_mass_2=1.0, new_q_2=0.0, **rx)     # A(3,4) + D(1,2) -> A(-2):B(0)
            g.reactions_enable(True)
        g.run(5)
        yield g, h


def stage_driver(tmp_path):
    """the fixture of tests/test_host_hybrid_tuples.py (chain_growth_catalytic with angle and dihedral types spliced in), with a
    reaction step every 5 MD steps and rates that make every candidate react, so that chains of three and four beads -- angles
    and dihedrals to spawn -- exist after a few dozen steps"""
    from test_host_hybrid_tuples import stage
    d = stage(tmp_path)
    cfg = open(str(d / "reaction.cfg")).read()
    assert cfg.count("interval: 500") == 1 and cfg.count("rate: 1.0") == 4
    open(str(d / "reaction.cfg"), "w").write(cfg.replace("interval: 500", "interval: 5").replace("rate: 1.0", "rate: 100.0"))
    return d


@pytest.mark.parametrize("prec", [64, 32])
def test_driver_end_to_end(tmp_path, monkeypatch, prec):
    """start_simulation.main on the staged fixture with --t_hybrid_angle 8 --t_hybrid_dihedral 8 on the HIP engine, against the
    same run assembled by hand from engine calls (by_hand; it takes the particle arrays the driver's readers produced, everything
    else is written out there): events, lists, lambdas, the energy file's columns, positions and forces; and against what the
    event log says must have been spawned, with which birth steps."""
    from chemlab_amd import espp, start_simulation
    kept = []

    class Keep(Engine):
        def set_particles(self, *a, **k):
            kept.append((a, k))
            return Engine.set_particles(self, *a, **k)
    monkeypatch.chdir(stage_driver(tmp_path))
    prev = espp._factory[0]
    espp.set_engine_factory(lambda: Keep(device=0, precision=prec))
    try:
        res = start_simulation.main(["@params", "--run=60", "--start_ar=10", "--t_hybrid_angle=8", "--t_hybrid_dihedral=8"], quiet=True)
    finally:
        espp.set_engine_factory(prev)
    e = res["system"].engine
    assert len(kept) == 1 and e.step == 60
    lists = dict(ad=res["angles"]["angle_dynamic"][0], ah=res["angles"]["angle_hybrid"][0], dd=res["dihedrals"]["dihedral_dynamic"][0],
                 dh=res["dihedrals"]["dihedral_hybrid"][0], rb=res["chem_fpls"][0][1])
    run = by_hand(prec, kept[0], 8)
    g, h = next(run)
    rows_hand = []
    try:
        for g, _ in run:
            ob = g.observe()
            lam3, lam4 = g.list_get_lambda(h["ah"]), g.list_get_lambda(h["dh"])
            rows_hand.append((g.step, ob["epot_list"][h["ah"]], ob["epot_list"][h["dh"]], float(lam3.mean()) if len(lam3) else 0.0, float(lam4.mean()) if len(lam4) else 0.0,
                              ob["list_size"][h["rb"]]))
        # the same events, the same lists in the same order, the same lambdas
        ev = event_rows(e)
        assert ev == event_rows(g) and len(ev) > 1000
        for key in ("rb", "ad", "ah", "dd", "dh"):
            assert np.array_equal(e.get_list(lists[key].handle), g.get_list(h[key])), key
        assert len(e.get_list(lists["ad"].handle)) == 0 and len(e.get_list(lists["dd"].handle)) == 0      # nothing of the start: all that exists was spawned
        t3, t4 = g.get_list(h["ah"]), g.get_list(h["dh"])
        assert len(t3) > 50 and len(t4) > 20
        assert lists["ah"].getAllLambda() == g.list_get_lambda(h["ah"]).tolist() and lists["dh"].getAllLambda() == g.list_get_lambda(h["dh"]).tolist()
        # what the event log says: the tuples around the bonds of reactions 1 and 2 (0 and 3 are virtual), born with the later bond
        bonds = [(s, a, b) for s, a, b, r in ev if r in (1, 2)]
        s3, b3, s4, b4 = T.spawned(np.zeros((0, 2), np.int64), bonds, e.get_state("TYPE"), list(ANG_TYPES), DIH_TYPES)
        for got, rows, births, lam in ((t3, s3, b3, g.list_get_lambda(h["ah"])), (t4, s4, b4, g.list_get_lambda(h["dh"]))):
            birth = dict(zip(canon(rows), births.tolist()))
            assert sorted(canon(got)) == sorted(birth)
            want = T.ramp(0.0, 0.125, 60, np.array([birth[c] for c in canon(got)]))
            assert np.array_equal(lam, want) and {0.0, 0.625, 1.0} <= set(want.tolist())                 # born at 60, at 55, and saturated
        # the spawned tuples' 1-3 / 1-4 pairs and the bonds are excluded, in the driver's run as by hand
        ex = {tuple(p) for p in e.get_exclusions().tolist()}
        assert ex == {tuple(p) for p in g.get_exclusions().tolist()}
        assert {(min(t[0], t[-1]), max(t[0], t[-1])) for t in t3.tolist() + t4.tolist()} <= ex
        # positions and forces
        e.run(0); g.run(0)
        tol_x, tol_f = (1e-9, 1e-8) if prec == 64 else (1e-5, 10 * TOL_F[32])
        print("prec %d: driver against by hand, positions %.3e, forces %.3e" % (prec, rel_err(e.get_state("POS_UNFOLDED"), g.get_state("POS_UNFOLDED")), rel_err(e.get_state("FORCE"), g.get_state("FORCE"))))
        assert rel_err(e.get_state("POS_UNFOLDED"), g.get_state("POS_UNFOLDED")) < tol_x and rel_err(e.get_state("FORCE"), g.get_state("FORCE")) < tol_f
        # the hybrid lists' energies against the reference, every entry with its own lambda
        x, ty = e.get_state("POS"), e.get_state("TYPE")
        ref = T.reference(x, [12.111984] * 3, ty, [dict(arity=3, kind="ANG_HARMONIC", typed=[(k, [K, th * math.pi / 180]) for k, (K, th) in ANG_TYPES.items()], ids=t3),
                                                  dict(arity=4, kind="DIH_NCOS", typed=[(k, [2.0, 20.0 * math.pi / 180, 3.0]) for k in DIH_TYPES], ids=t4)],
                          [g.list_get_lambda(h["ah"]), g.list_get_lambda(h["dh"])])
        ob = e.observe()
        assert ob["epot_list"][lists["ah"].handle] == pytest.approx(ref["energy"][0], rel=TOL_EL[prec]) and ob["epot_list"][lists["dh"].handle] == pytest.approx(ref["energy"][1], rel=TOL_EL[prec])
        # the energy file: its columns, and every row against the by-hand run at the same step (six digits are written)
        table = [l.strip().split(",") for l in open("sim0_energy_12345.csv")]
        head = table[0]
        assert head[-5:] == ["angle_hybrid", "dihedral_hybrid", "count_0", "res_ftl_0", "res_fql_0"] and "angle_dynamic" in head and "dihedral_dynamic" in head
        assert len(table) == 13
        for row, hand in zip(table[1:], rows_hand):
            r = dict(zip(head, row))
            assert int(r["step"]) == hand[0] and float(r["count_0"]) == hand[5]
            assert float(r["angle_hybrid"]) == pytest.approx(hand[1], rel=1e-4, abs=1e-6) and float(r["dihedral_hybrid"]) == pytest.approx(hand[2], rel=1e-4, abs=1e-6)
            assert float(r["res_ftl_0"]) == pytest.approx(hand[3], rel=1e-5) and float(r["res_fql_0"]) == pytest.approx(hand[4], rel=1e-5)
            assert float(r["angle_dynamic"]) == 0.0 and float(r["dihedral_dynamic"]) == 0.0
        assert 0.0 < rows_hand[-1][3] < 1.0 and 0.0 < rows_hand[-1][4] < 1.0                                # mid-ramp at the end
    finally:
        g.close()
        e.close()
