"""Per-particle resolution lambda on the HIP path (chem_nb_resolution: k_pair_tiles MODE 5, k_pair_force_res; chem_resolution_rate,
chem_set_resolution, chem_reaction_set_resolution).  Rule set: include/chem_mi355.h.

The CPU oracle has no lambda, so the rule set is restated in numpy (tests/dynres_ref.py, which imports nothing from the
product) and everything is compared with a brute-force sum over all pairs.

Shapes are those of tests/test_gpu_spline_tables.py: rc = 1.5, skin = 0.3, jittered lattice of spacing 0.75.  (a) 9.0^3: five
cells per axis, tiles.  (b) (9.0, 10.8, 12.6).  (c) 5.4^3: three cells per axis, k_pair_force_res.  (slab) (9.0, 9.0, 18.0) on
two in-process ranks.

System: three types drawn uniformly; 0-0 LJ (cutoff 1.3) marked, 1-1 table marked (linear, or the natural cubic spline where a
test says so), 0-1 LJ UNMARKED (the mask), 0-2 LJ (cutoff 1.4) marked with a cap where a test sets one, 1-2 and 2-2 nothing.
lambda per particle: 0 with weight 0.2, 1 with weight 0.4, otherwise uniform in (0, 1).

Every force test first asserts on the CPU (guard) that the scaled reference differs from the unscaled one by more than 1e-2
of the largest force, that some marked pair has both lambdas strictly inside (0, 1), that some marked pair with w == 0 sits
where its unscaled force would exceed the largest force a marked pair applies -- so that evaluating it would show --, and
that, for the fp32 comparisons, no pair that carries a term lies within 2e-6 of its cutoff (no cutoff flip is allowed in
fp32; the seeds below were chosen on the CPU for that).

Tolerances are the project's: fp64 forces TOL[64] = 1e-10 of the largest force, fp32 pair forces TOL_MELT32 = 2e-5 with no
cutoff flip, energies and virials 1e-11 (fp64) / 1e-5 (fp32)."""
import numpy as np
import pytest

import dynres_ref as D
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks
from test_gpu_spline_tables import BOXES, DT, RC, SKIN, table_11

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_MELT32}
TOL_E = {64: 1e-11, 32: 1e-5}
LJ00, LJ01, LJ02 = (1.0, 0.5, 1.3), (1.0, 0.5, RC), (0.8, 0.6, 1.4)
MARKED = ((0, 0), (1, 1), (0, 2))
# fp32 decides a cutoff like fp64 unless the pair lies within rounding of it: the shell helpers.force_error_without_cutoff_flips looks at
GAP32 = 2e-6
SEED = {"a": 2, "b": 1, "c": 1, "slab": 1}


def system(shape, seed=None, kT=0.3, dt=DT, vel=True):
    box = np.array(BOXES[shape])
    rng = np.random.default_rng(SEED[shape] if seed is None else seed)
    k = np.floor(box / 0.75 + 1e-9).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3)
    pos = g * 0.75 - 0.1 + rng.uniform(-0.1, 0.1, g.shape)
    n = len(pos)
    types_ = rng.integers(0, 3, n).astype(np.int32)
    u = rng.random(n)
    lam = np.where(u < 0.2, 0.0, np.where(u < 0.6, 1.0, rng.uniform(0.02, 0.98, n)))
    v = rng.normal(0.0, np.sqrt(kT), (n, 3))
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=dt, ids=np.arange(1, n + 1), types=types_, lam=lam,
                pos=pos, vel=v if vel else np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), kT=kT, gamma=0.0, seed=1, rebuild_criterion=1)
    return W.snap_to_grid(spec)


def pair_spec(spec, itype=1, cap=0.0, resolution=True):
    """the non-bonded matrix of the module docstring as W.apply takes it"""
    out = dict(spec, lj=[(0, 0) + LJ00, (0, 1) + LJ01, (0, 2) + LJ02], tables=[(1, 1) + table_11() + (RC, itype)])
    if resolution:
        out["resolution"] = [(0, 0, 0.0), (1, 1, 0.0), (0, 2, cap)]
    else:
        out.pop("lam", None)
    return out


def matrix(itype=1):
    return {(0, 0): S.lj(*LJ00), (0, 1): S.lj(*LJ01), (0, 2): S.lj(*LJ02), (1, 1): ("tab", S.Table(*table_11(), itype), RC)}


def marked(cap=0.0):
    return {(0, 0): 0.0, (1, 1): 0.0, (0, 2): cap}


def guard(pos, box, types_, lam, itype=1, cap=0.0, excluded=(), prec=32, dead_pairs=True):
    """the reference of this configuration, after the assertions of the module docstring (dead_pairs = False: a configuration
    in the middle of a ramp on the LJ types, where no strongly repelling pair has w == 0 any more; the static tests hold that guard)"""
    ref = D.total(pos, box, types_, lam, matrix(itype), marked(cap), excluded)
    plain = D.total(pos, box, types_, np.ones(len(lam)), matrix(itype), marked(0.0), excluded)
    part = np.abs(ref["F"] - plain["F"]).max() / np.abs(plain["F"]).max()
    p = ref["pairs"]
    li, lj = np.asarray(lam)[p["i"]], np.asarray(lam)[p["j"]]
    both_inside = p["marked"] & (li > 0) & (li < 1) & (lj > 0) & (lj < 1)
    mag = np.sqrt(p["r2"])
    dead, alive = p["marked"] & (p["w"] == 0.0), p["marked"] & (p["w"] != 0.0)
    gap = D.gap_to_cutoff(pos, box, types_, lam, matrix(itype), marked(cap), excluded)
    print("scaling moves %.3e of the largest force; %d pairs with both lambdas inside (0, 1); largest unscaled force of a w = 0 pair %.3e, "
          "largest applied marked force %.3e; nearest pair with a term %.3e from its cutoff" %
          (part, both_inside.sum(), (np.abs(p["ff"]) * mag)[dead].max() if dead.any() else 0.0, (np.abs(p["fs"]) * mag)[alive].max(), gap))
    assert part > 1e-2
    assert both_inside.any()
    assert not dead_pairs or (np.abs(p["ff"]) * mag)[dead].max() > (np.abs(p["fs"]) * mag)[alive].max()
    assert prec == 64 or gap > GAP32
    return ref


def compare(fg, ob, spec, x, prec, ref, itype=1):
    if prec == 64:
        err, flips = rel_err(fg, ref["F"]), 0
    else:
        s = dict(pair_spec(spec, itype, resolution=False), pos=x)
        s["tables"] = [t[:7] for t in s["tables"]]
        err, flips = force_error_without_cutoff_flips(s, fg, ref["F"], TOL_F[32], max_flips=0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    print("prec %d: force rel err %.3e flips %d, virial_nb %.3e epot_lj %.3e epot_tab %.3e" %
          (prec, err, flips, rel(ob["virial_nb"], ref["w_nb"]), rel(ob["epot_lj"], ref["e_lj"]), rel(ob["epot_tab"], ref["e_tab"])))
    assert err < TOL_F[prec] and flips == 0
    assert ob["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[prec])
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec]) and ob["epot_tab"] == pytest.approx(ref["e_tab"], rel=TOL_E[prec])


def check(g, spec, prec, ref, itype=1):
    """forces, virial and the two energies at the engine's current positions"""
    g.run(0)
    compare(g.get_state("FORCE"), g.observe(), spec, g.get_state("POS"), prec, ref, itype)


# ---- 1: forces, energies and virial at step 0 --------------------------------------------------------------------------------

_REF = {}


def static_ref(shape, itype=1):
    """computed once, shared by both precisions"""
    if (shape, itype) not in _REF:
        spec = system(shape)
        _REF[(shape, itype)] = (spec, guard(spec["pos"], spec["box"], spec["types"], spec["lam"], itype))
    return _REF[(shape, itype)]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape,itype", [("a", 1), ("a", 3), ("b", 1), ("c", 1), ("c", 3)])
def test_static_forces_energies_and_virial(make_gpu, shape, itype, prec):
    spec, ref = static_ref(shape, itype)
    g = make_gpu(prec)
    W.apply(pair_spec(spec, itype), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref, itype)
    assert np.array_equal(g.get_state("LAMBDA"), spec["lam"])


def two_ranks(make_gpu, spec, body):
    P = 2
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        return body(g)
    return _run_ranks(P, rank)


def test_static_forces_on_two_slabs(make_gpu):
    spec, ref = static_ref("slab")

    def body(g):
        W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
        g.run(0)
        return dict(f=g.get_state("FORCE"), ob=g.observe(), x=g.get_state("POS"), lam=g.get_state("LAMBDA"))
    for out in two_ranks(make_gpu, spec, body):
        compare(out["f"], out["ob"], spec, out["x"], 64, ref)
        assert np.array_equal(out["lam"], spec["lam"])


# ---- 2: the cap ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_cap_on_the_02_pairs(make_gpu, shape, prec):
    """max_force on 0-2 = the median magnitude of the reference's uncapped 0-2 pair forces: about half of them are capped.
    The energy is uncapped."""
    spec, free = static_ref(shape)
    p = free["pairs"]
    is02 = (p["cap"] == 0.0) & p["marked"] & (p["w"] != 0.0) & (np.minimum(spec["types"][p["i"]], spec["types"][p["j"]]) == 0) & \
           (np.maximum(spec["types"][p["i"]], spec["types"][p["j"]]) == 2)
    cap = float(np.median((np.abs(p["fs"]) * np.sqrt(p["r2"]))[is02]))
    ref = guard(spec["pos"], spec["box"], spec["types"], spec["lam"], cap=cap)
    share = ref["pairs"]["capped"][is02].mean()
    print("cap %.4f: %.2f of the %d 0-2 pairs capped" % (cap, share, is02.sum()))
    assert 0.25 <= share <= 0.75
    assert rel_err(ref["F"], free["F"]) > 1e-2                   # the cap is far from negligible
    assert ref["e_lj"] == free["e_lj"]
    g = make_gpu(prec)
    W.apply(pair_spec(spec, cap=cap), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref)


# ---- 3: the ramp ---------------------------------------------------------------------------------------------------------------

def ramp_model(spec, l0, steps):
    """lambda of every particle after `steps` steps: type 0 from l0 at 1/16 per step, the others as drawn"""
    return np.array([D.lam(l0, 0, 1 / 16, steps) if t == 0 else l for t, l in zip(spec["types"], spec["lam"])])


def ramp_spec(spec, l0):
    lam = np.where(spec["types"] == 0, l0, spec["lam"])
    return dict(pair_spec(dict(spec, lam=lam)), res_rates=[(0, 1 / 16)])


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("l0", [0.0, 0.5])
def test_ramp(make_gpu, l0, prec):
    spec = system("a")
    one, two = make_gpu(prec), make_gpu(prec)
    W.apply(ramp_spec(spec, l0), one, thermostat=False, reactions=False)
    W.apply(ramp_spec(spec, l0), two, thermostat=False, reactions=False)
    assert np.array_equal(one.get_state("LAMBDA"), ramp_model(spec, l0, 0))
    one.run(40)
    two.run(15)
    assert np.array_equal(two.get_state("LAMBDA"), ramp_model(spec, l0, 15))
    assert ((two.get_state("LAMBDA") > 0) & (two.get_state("LAMBDA") < 1) & (spec["types"] == 0)).any() == (l0 == 0.0)
    two.run(25)
    want = ramp_model(spec, l0, 40)
    assert np.array_equal(one.get_state("LAMBDA"), want) and np.array_equal(two.get_state("LAMBDA"), want)
    for g in (one, two):
        x = g.get_state("POS")
        assert np.abs(x - spec["pos"]).max() > 1e-3
        check(g, spec, prec, guard(x, spec["box"], spec["types"], want, prec=prec))


def test_ramp_midway_forces(make_gpu):
    """the forces while the ramp is under way: 9 steps from 0, lambda = 9/16 on every type-0 particle"""
    spec = system("a")
    g = make_gpu(64)
    W.apply(ramp_spec(spec, 0.0), g, thermostat=False, reactions=False)
    g.run(9)
    want = ramp_model(spec, 0.0, 9)
    assert np.array_equal(g.get_state("LAMBDA"), want) and (want == 9 / 16).any()
    fg, x = g.get_state("FORCE"), g.get_state("POS")                  # the forces the run left behind: those current at step 9
    ref = guard(x, spec["box"], spec["types"], want, prec=64)
    assert rel_err(fg, ref["F"]) < TOL_F[64]
    late = D.total(x, spec["box"], spec["types"], ramp_model(spec, 0.0, 10), matrix(), marked())
    assert rel_err(late["F"], ref["F"]) > 1e-3                        # one step's lambda off would show
    check(g, spec, 64, ref)


def test_ramp_on_two_slabs(make_gpu):
    spec = system("slab")

    def body(g):
        W.apply(ramp_spec(spec, 0.0), g, thermostat=False, reactions=False)
        g.run(15)
        mid = g.get_state("LAMBDA")
        g.run(25)
        g.run(0)
        return dict(mid=mid, lam=g.get_state("LAMBDA"), x=g.get_state("POS"), f=g.get_state("FORCE"), ob=g.observe())
    out = two_ranks(make_gpu, spec, body)
    assert np.array_equal(out[0]["x"], out[1]["x"])
    want = ramp_model(spec, 0.0, 40)
    ref = guard(out[0]["x"], spec["box"], spec["types"], want, prec=64)
    for o in out:
        assert np.array_equal(o["mid"], ramp_model(spec, 0.0, 15)) and np.array_equal(o["lam"], want)
        compare(o["f"], o["ob"], spec, o["x"], 64, ref)


# ---- 4: completion ------------------------------------------------------------------------------------------------------------

NEW_MASS, NEW_Q = 2.5, 0.5


def completion_system():
    spec = system("a")
    chosen = np.nonzero(spec["types"] == 2)[0][[3, 10, 17, 40, 77]]
    lam = np.where(spec["types"] == 2, 1.0, spec["lam"])         # the rate acts on every type-2 particle with lambda < 1: only the chosen
    lam[chosen] = 0.0
    full = dict(pair_spec(dict(spec, lam=lam)), res_rates=[dict(type_id=2, alpha=1 / 8, new_type=1, new_mass=NEW_MASS, new_q=NEW_Q)])
    return spec, chosen, lam, full


@pytest.mark.parametrize("prec", [64, 32])
def test_completion_changes_the_properties_when_lambda_reaches_one(make_gpu, prec):
    spec, chosen, lam, full = completion_system()
    assert D.s_full(0.0, 0, 1 / 8) == 8
    g, single = make_gpu(prec), make_gpu(prec)
    W.apply(full, g, thermostat=False, reactions=False)
    W.apply(full, single, thermostat=False, reactions=False)
    g.run(7)
    lam7 = lam.copy(); lam7[chosen] = 7 / 8
    assert np.array_equal(g.get_state("TYPE"), spec["types"]) and np.array_equal(g.get_state("LAMBDA"), lam7)
    assert np.array_equal(g.get_state("MASS"), spec["mass"])
    g.run(1)
    ty, lam8, mass, q = spec["types"].copy(), lam.copy(), spec["mass"].copy(), np.zeros(len(lam))
    ty[chosen], lam8[chosen], mass[chosen], q[chosen] = 1, 1.0, NEW_MASS, NEW_Q
    assert g.step == 8
    assert np.array_equal(g.get_state("TYPE"), ty) and np.array_equal(g.get_state("LAMBDA"), lam8)
    assert np.array_equal(g.get_state("MASS"), mass) and np.array_equal(g.get_state("CHARGE"), q)
    # the forces current at s_full are those of type 1's potentials (1-1 table, 0-1 LJ unmarked; no 0-2 LJ any more)
    x, fg = g.get_state("POS"), g.get_state("FORCE")
    ref = guard(x, spec["box"], ty, lam8, prec=prec)
    old = D.total(x, spec["box"], spec["types"], lam8, matrix(), marked())
    assert rel_err(old["F"], ref["F"]) > 1e-3
    if prec == 64:
        assert rel_err(fg, ref["F"]) < TOL_F[64]
    check(g, dict(spec, types=ty), prec, ref)
    # a single run over the completion step: the same types and the same lambda, and it goes on from there
    single.run(12)
    g.run(4)
    assert np.array_equal(single.get_state("TYPE"), ty) and np.array_equal(single.get_state("LAMBDA"), lam8)
    assert np.array_equal(single.get_state("MASS"), mass)
    assert np.array_equal(g.get_state("TYPE"), ty) and np.array_equal(g.get_state("LAMBDA"), lam8)
    if prec == 64:
        assert np.abs(single.get_state("POS") - g.get_state("POS")).max() < 1e-9


# ---- 5: a dissociation reaction drives it ------------------------------------------------------------------------------------

BOND_K, BOND_R0 = 40.0, 0.7


L1, L2 = 0.0, 0.25                                              # lambda the two roles get on the break: different, so that a swap shows


def dissociation_system():
    """Harmonic dimers of one type-0 and one type-2 particle (lambda 1, so that they are still of those types at the event);
    everybody else keeps the drawn lambda and ramps at 1/8 per step like the broken pairs will"""
    spec = dict(system("a", dt=1e-4, vel=False))
    pos, box, ty = spec["pos"], np.asarray(spec["box"]), spec["types"]
    iu = np.triu_indices(len(pos), 1)
    d = pos[iu[0]] - pos[iu[1]]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(1))
    hit = np.nonzero((r < 0.8) & (((ty[iu[0]] == 0) & (ty[iu[1]] == 2)) | ((ty[iu[0]] == 2) & (ty[iu[1]] == 0))))[0]
    bonds, used = [], set()
    for k in hit:
        a, b = int(iu[0][k]), int(iu[1][k])
        if a in used or b in used:
            continue
        bonds.append((a, b) if ty[a] == 0 else (b, a)); used.update((a, b))
    bonds = bonds[:40]
    assert len(bonds) == 40 and r[hit].min() > 0.35
    lam = spec["lam"].copy()
    lam[[i for p in bonds for i in p]] = 1.0
    spec["lam"] = lam
    return spec, bonds


def dissociation_model(spec, bonds, upto):
    """types and stamps step by step: the event at step 2 stamps (L1, L2), then whatever is complete at a step changes"""
    m = D.Stamps(spec["types"].tolist())
    for i, l in enumerate(spec["lam"]):
        m.set_lambda(i, l, 0)
    m.set_rate(0, 1 / 8, 0, 1)
    m.set_rate(2, 1 / 8, 0, 1)
    changed = set()
    for s in range(1, upto + 1):
        if s == 2:
            for a, b in bonds:
                m.set_lambda(a, L1, 2); m.set_lambda(b, L2, 2)
        changed.update(m.complete(s))
    ty = np.array(m.types, dtype=np.int32)
    mass = np.where(np.isin(np.arange(len(ty)), sorted(changed)), 1.5, 1.0)
    return ty, np.array([m.lam(i, upto) for i in range(len(ty))]), mass


def dissociation_engine(make_gpu, spec, bonds, prec):
    ids = [(a + 1, b + 1) for a, b in bonds]
    g = make_gpu(prec)
    h = W.apply(dict(pair_spec(spec, cap=50.0), exclusions=ids, lists=[dict(arity=2, kind="HARMONIC", params=[BOND_K, BOND_R0], ids=ids)],
                     res_rates=[dict(type_id=0, alpha=1 / 8, new_type=1, new_mass=1.5, new_q=0.0), dict(type_id=2, alpha=1 / 8, new_type=1, new_mass=1.5, new_q=0.0)]),
                g, thermostat=False, reactions=False)
    g.reaction_init(2, nearest=True, seed=4)
    rx = g.dissociation_add(type_1=0, type_2=2, delta_1=0, delta_2=0, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1,
                            diss_rate=0.0, cutoff=0.3, bond_list=h[0], unexclude=True, new_type_1=-1, new_type_2=-1)
    g.reaction_set_resolution(rx, 1, L1)
    g.reaction_set_resolution(rx, "type_2", L2)
    g.reactions_enable(True)
    return g, h


def same_state(g, spec, bonds, step):
    ty, lam, mass = dissociation_model(spec, bonds, step)
    assert g.step == step
    assert np.array_equal(g.get_state("TYPE"), ty) and np.array_equal(g.get_state("LAMBDA"), lam) and np.array_equal(g.get_state("MASS"), mass)
    return ty, lam


@pytest.mark.parametrize("prec", [64, 32])
def test_dissociation_sets_lambda_and_the_ramp_changes_the_types(make_gpu, prec):
    """The dissociation's distance rule alone fires (diss_rate 0, cutoff 0.3 below every dimer's length) at the first reaction
    step (interval 2).  Role 1 gets lambda 0, role 2 lambda 0.25, both keep their type; rate 1/8 on both old types with the
    change to type 1: role 2 changes 6 steps after the event, role 1 after 8.  A second context crosses the event and every
    completion step in ONE run(12): the same types, masses and lambda, the same positions."""
    spec, bonds = dissociation_system()
    a_, b_ = np.array([p[0] for p in bonds]), np.array([p[1] for p in bonds])
    g, h = dissociation_engine(make_gpu, spec, bonds, prec)
    single, _ = dissociation_engine(make_gpu, spec, bonds, prec)
    g.run(1)
    assert len(g.get_events()) == 0
    same_state(g, spec, bonds, 1)
    g.run(1)
    ev = g.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev) == sorted(bonds) and set(ev["step"].tolist()) == {2}
    ty, lam = same_state(g, spec, bonds, 2)
    assert (lam[a_] == L1).all() and (lam[b_] == L2).all() and (ty[a_] == 0).all() and (ty[b_] == 2).all()
    assert len(g.get_list(h[0])) == 0
    g.run(3)                                                      # in between: 3/8 and 0.25 + 3/8, the pairs interact again (scaled, capped)
    ty, lam = same_state(g, spec, bonds, 5)
    assert (lam[a_] == 3 / 8).all() and (lam[b_] == 5 / 8).all() and (ty[a_] == 0).all() and (ty[b_] == 2).all()
    x = g.get_state("POS")
    ref = guard(x, spec["box"], ty, lam, cap=50.0, prec=prec, dead_pairs=False)
    still_excluded = D.total(x, spec["box"], ty, lam, matrix(), marked(50.0), excluded=bonds)
    assert rel_err(still_excluded["F"], ref["F"]) > 1e-3         # the broken pairs do act through the 0-2 potential
    check(g, dict(spec, types=ty), prec, ref)
    g.run(3)                                                      # role 2: 0.25 + 6/8 = 1 at step 8
    ty, lam = same_state(g, spec, bonds, 8)
    assert (ty[b_] == 1).all() and (lam[b_] == 1.0).all() and (ty[a_] == 0).all() and (lam[a_] == 6 / 8).all()
    g.run(2)                                                      # role 1: 8/8 at step 10
    ty, lam = same_state(g, spec, bonds, 10)
    assert (ty[a_] == 1).all() and (lam[spec["types"] != 1] == 1.0).all()      # (type 1 has no rate: its drawn lambdas stay)
    assert not (ty[spec["lam"] < 1.0] == 0).any() and not (ty[spec["lam"] < 1.0] == 2).any()      # whatever ramped has changed; lambda = 1 from the start: untouched
    check(g, dict(spec, types=ty), prec, guard(g.get_state("POS"), spec["box"], ty, lam, cap=50.0, prec=prec, dead_pairs=False))
    g.run(2)
    single.run(12)                                                # the event at step 2 and its completion steps lie inside one call
    same_state(single, spec, bonds, 12)
    same_state(g, spec, bonds, 12)
    ev1 = single.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev1) == sorted(bonds) and set(ev1["step"].tolist()) == {2}
    dx = np.abs(single.get_state("POS") - g.get_state("POS")).max()
    print("single run against stepped runs: max |dx| %.3e" % dx)
    assert dx < (1e-9 if prec == 64 else 1e-5)


def test_an_association_reaction_sets_lambda_on_its_two_roles(make_gpu):
    """a virtual 0 + 2 reaction at an infinite rate (the isolated close pairs of tests/test_gpu_coulomb.py) with lambda 0 on
    role 1 and 0.5 on role 2; no rate, so nothing else moves"""
    from test_gpu_coulomb import REACT_CUT, reacting_pairs
    spec = system("a", dt=1e-5, vel=False)
    pairs = reacting_pairs(spec)
    assert 3 <= len(pairs) <= 60
    g = make_gpu(64)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.reaction_init(1, nearest=True, seed=4)
    r = g.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=1e30, cutoff=REACT_CUT, is_virtual=True, intramolecular=True, intraresidual=True)
    g.reaction_set_resolution(r, 1, 0.0)
    g.reaction_set_resolution(r, 2, 0.5)
    g.reactions_enable(True)
    g.run(3)                                                      # the event is at step 1, inside the call
    ev = g.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev) == sorted(pairs) and set(ev["step"].tolist()) == {1}
    lam = spec["lam"].copy()
    for a, b in pairs:
        lam[a], lam[b] = 0.0, 0.5
    assert np.array_equal(g.get_state("LAMBDA"), lam) and np.array_equal(g.get_state("TYPE"), spec["types"])
    g.reactions_enable(False)
    check(g, spec, 64, guard(g.get_state("POS"), spec["box"], spec["types"], lam, prec=64))


# ---- 6: inert ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_a_context_without_resolution_is_untouched(make_gpu, shape, prec):
    """no resolution call at all against nb_resolution(on = 0) on every pair and set_resolution(ids, 1.0): forces and a short
    trajectory bit for bit, the same launch counts in the timers, and no lambda but 1"""
    spec = system(shape)
    plain, g = make_gpu(prec), make_gpu(prec)
    W.apply(pair_spec(spec, resolution=False), plain, thermostat=False, reactions=False)
    W.apply(pair_spec(spec, resolution=False), g, thermostat=False, reactions=False)
    for a, b in MARKED:
        g.nb_resolution(a, b, False, 0.0)
    g.set_resolution(spec["ids"], 1.0)
    g.run(0); plain.run(0)
    assert np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    og, op = g.observe(), plain.observe()
    assert og["epot_lj"] == op["epot_lj"] and og["epot_tab"] == op["epot_tab"] and og["virial_nb"] == op["virial_nb"]
    assert np.array_equal(g.get_state("LAMBDA"), np.ones(spec["n"]))
    # the scaled forces are another matter: marking the pairs with lambda drawn does change them
    g.set_resolution(spec["ids"], spec["lam"])
    for a, b in MARKED:
        g.nb_resolution(a, b, True, 0.0)
    g.run(0)
    assert rel_err(g.get_state("FORCE"), plain.get_state("FORCE")) > 1e-2
    # unmarking brings the old kernels back, whatever lambda the particles have: bit-identical once more, and along a trajectory
    for a, b in MARKED:
        g.nb_resolution(a, b, False, 0.0)
    plain.set_option("tiles", 1)                                    # (both contexts build their lists again)
    for e in (plain, g):
        e.set_option("time_pair_kernel", 1)
        e.run(0)
    assert np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    g.run(20); plain.run(20)
    assert np.array_equal(g.get_state("POS"), plain.get_state("POS")) and np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    # The guard of existing behaviour is the bit-identical forces and trajectory above.  The timers expose launch counts, no
    # kernel names, so they cannot tell k_pair_tiles_res from k_pair_tiles: the counts only show that nothing was launched extra.
    tg, tp = g.timers(), plain.timers()
    assert tg.keys() == tp.keys()
    for k in ("pair_kernel_launches", "bonded_kernel_launches", "integrate_kernel_launches", "steps"):
        assert tg[k] == tp[k] or k == "steps", k
    assert tg["pair_kernel_launches"] > 0


# ---- 7: refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu):
    spec = system("a")
    g = make_gpu(64)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.run(0)
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        with pytest.raises(ChemError) as ei:
            g.set_resolution([1, 2], [0.5, bad])
        assert ei.value.code == _capi.EINVAL
        with pytest.raises(ChemError) as ei:
            g.modify_particle(1, "LAMBDA", bad)
        assert ei.value.code == _capi.EINVAL
    assert np.array_equal(g.get_state("LAMBDA"), spec["lam"])      # a refused call sets nothing
    with pytest.raises(ChemError) as ei:
        g.set_resolution([spec["n"] + 5], [0.5])
    assert ei.value.code == _capi.EINVAL
    g.modify_particle(1, "LAMBDA", 0.125)
    assert g.get_state("LAMBDA")[0] == 0.125
    # reactions: role and index
    h = g.list_create(2, "HARMONIC")
    g.list_set_params(h, [BOND_K, BOND_R0])
    g.reaction_init(5, nearest=True, seed=1)
    r = g.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=0.0, cutoff=0.5, bond_list=h)
    g.reaction_set_resolution(r, 1, 0.0)
    g.reaction_set_resolution(r, 1, -1.0)                           # removes the rule again
    for role in (0, 3):
        with pytest.raises(ChemError, match="role") as ei:
            g.reaction_set_resolution(r, role, 0.0)
        assert ei.value.code == _capi.EINVAL
    for idx in (r + 1, -1, 99):
        with pytest.raises(ChemError, match="unknown reaction index") as ei:
            g.reaction_set_resolution(idx, 1, 0.0)
        assert ei.value.code == _capi.EINVAL
    with pytest.raises(ChemError) as ei:
        g.reaction_set_resolution(r, 1, 1.5)
    assert ei.value.code == _capi.EINVAL
    # a type pair without a potential has nothing to scale: EINVAL (documented in the header); unmarking it is a no-op
    with pytest.raises(ChemError, match=r"type pair \(1,2\) carries no") as ei:
        g.nb_resolution(1, 2, True, 0.0)
    assert ei.value.code == _capi.EINVAL
    g.nb_resolution(1, 2, False, 0.0)
    with pytest.raises(ChemError) as ei:
        g.nb_resolution(0, 16, True, 0.0)
    assert ei.value.code == _capi.EINVAL
    # the build limits of the mode, as for the Coulomb term
    for opt, bad, good in (("tpp", 2, 0), ("pair_block", 256, 512)):
        g.set_option(opt, bad)
        with pytest.raises(ChemError, match=opt) as ei:
            g.run(0)
        assert ei.value.code == _capi.EINVAL
        g.set_option(opt, good)
        g.run(0)
    # the Coulomb combination: refused at the next evaluation, naming the marked pair
    g.nb_coulomb(1, 2, 1.5, 1.2)
    with pytest.raises(ChemError, match=r"resolution-scaled type pair \(0,0\)") as ei:
        g.run(0)
    assert ei.value.code == _capi.ENOTIMPL
    g.nb_coulomb(1, 2, 0.0, 1.2)
    g.run(0)
    # a reaction rule and the decomposed path
    g2 = make_gpu(64)
    W.apply(pair_spec(spec), g2, thermostat=False, reactions=False)
    h2 = g2.list_create(2, "HARMONIC")
    g2.reaction_init(5, nearest=True, seed=1)
    r2 = g2.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=0.0, cutoff=0.5, bond_list=h2)
    g2.reaction_set_resolution(r2, 2, 0.0)
    with pytest.raises(ChemError, match="reaction_set_resolution") as ei:
        g2.comm_init_local(2, 0, 4712)
    assert ei.value.code == _capi.ENOTIMPL
