"""Truncated Coulomb pair forces on the HIP path (chem_nb_coulomb: k_pair_tiles MODE 4, k_pair_force COUL, the by-tag
charge array).  Rule set: include/chem_mi355.h.

The CPU oracle has no Coulomb term, so the rule set is restated in numpy (tests/coulomb_ref.py, which imports nothing from
the product) and everything is compared with a brute-force sum over all pairs: LJ / table part from tests/spline_ref.py,
Coulomb part from coulomb_ref.

Shapes are those of tests/test_gpu_spline_tables.py: rc = 1.5, skin = 0.3, jittered lattice of spacing 0.75 whose first
layer lies 0.1 behind the low faces.  (a) 9.0^3, 12^3 particles: five cells per axis, tiles.  (b) (9.0, 10.8, 12.6).
(c) 5.4^3, 7^3 particles: three cells per axis, k_pair_force.  (slab) (9.0, 9.0, 18.0) on two in-process ranks.

System: three types drawn uniformly; charges from {-1, -0.5, 0, 0.5, 1} with weights (1, 1, 6, 1, 1) / 10, not neutral
overall; 0-0 under LJ with cutoff 1.3 (below rc_qq = 1.5, above rc_qq = 1.2), 1-1 under a table (linear, or the natural
cubic spline where a test says so: MODE 4 then covers kind 3), 0-1 under LJ WITHOUT the Coulomb term (mask), 0-2 and 1-2
with no LJ or table but with Coulomb (list activity), 2-2 with nothing at all.  Prefactor k = 1.5 (0.5 where a test
integrates, see KQ_MOTION).

Every force test first asserts on the CPU (guard) that the Coulomb part of the reference exceeds 1e-2 of the largest
force -- none can pass with the term missing -- and that no pair lies within 1e-4 of rc_qq, where the unshifted force is
discontinuous.  "Pair" there means a pair that carries a non-zero term (registered type pair, not excluded,
q_i q_j != 0): a pair without one has no discontinuity, and among ALL pairs of these boxes 7 are expected inside that
shell (N/2 * 4 pi r^2 rho * 2e-4 at r = 1.2), so no seed could meet the condition on them.  That is also why most
particles are neutral: 0.8 pairs with a term are expected in the shell, and the seeds below are such that there is none.

Tolerances are the project's: fp64 forces TOL[64] = 1e-10 of the largest force, fp32 pair forces TOL_MELT32 = 2e-5 with no
cutoff flip allowed, fp32 forces with bonds TOL_STIFF32 = 5e-5, energies and virials 1e-11 (fp64) / 1e-5 (fp32).
Measured on an MI355X when the path was built, static configurations: fp32 forces 4.1e-7 .. 3.1e-6 of the largest force
with no flip (with the dimers' bonds 1.6e-6), fp32 Coulomb energy 4.6e-8 .. 1.3e-6, its virial up to 2.4e-6, virial_nb
up to 5.4e-8, epot_lj / epot_tab up to 1.4e-7; fp64 forces up to 3.3e-14, energies and virials up to 3.3e-15.
After 200 steps with the seeds below the nearest charged pair lay 3.05e-4 (single domain, both precisions) and 1.92e-4
(two slabs) from rc_qq, with 9 and 8 list builds; forces there: fp32 5.9e-6, fp64 7.3e-15, two slabs 1.7e-14."""
import numpy as np
import pytest

import coulomb_ref as Q
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_parity import TOL, TOL_MELT32, TOL_STIFF32, _HUB, _run_ranks
from test_gpu_spline_tables import BOXES, DT, RC, SKIN, table_11

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_MELT32}
TOL_FB = {64: TOL[64], 32: TOL_STIFF32}
TOL_E = {64: 1e-11, 32: 1e-5}
KQ = 1.5
# The tests that integrate use a weaker term: the Coulomb-only pairs (0-2, 1-2) have no repulsive core, and with k = 1.5 two
# opposite charges that meet are thrown apart at speeds at which a particle crosses more than one slab layer between two
# list builds, which the decomposed path refuses ("particle migration error").
KQ_MOTION = 0.5
LJ00, LJ01 = (1.0, 0.5, 1.3), (1.0, 0.5, RC)
MASK = [(0, 0), (1, 1), (0, 2), (1, 2)]
CHARGES, WEIGHTS = (-1.0, -0.5, 0.0, 0.5, 1.0), (0.1, 0.1, 0.6, 0.1, 0.1)
# seeds with no charged, registered pair within 1e-4 of either rc_qq (SEED_MOTION: after the 200 steps of the tests that integrate)
SEED = {"a": 15, "b": 1, "c": 1, "slab": 1}
SEED_MOTION = {64: 3, 32: 3, "slab": 4}


def system(shape, seed=None, kT=1.0, dt=DT, vel=True):
    box = np.array(BOXES[shape])
    rng = np.random.default_rng(SEED[shape] if seed is None else seed)
    k = np.floor(box / 0.75 + 1e-9).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3)
    pos = g * 0.75 - 0.1 + rng.uniform(-0.1, 0.1, g.shape)
    n = len(pos)
    types_ = rng.integers(0, 3, n).astype(np.int32)
    q = rng.choice(CHARGES, n, p=WEIGHTS)
    v = rng.normal(0.0, np.sqrt(kT), (n, 3))
    assert abs(q.sum()) > 0.25                                   # not neutral overall
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=dt, ids=np.arange(1, n + 1), types=types_, q=q,
                pos=pos, vel=v if vel else np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), kT=kT, gamma=0.0, seed=1, rebuild_criterion=1)
    return W.snap_to_grid(spec)


def pair_spec(spec, rcq, itype=1, coulomb=True, k=KQ):
    """the non-bonded matrix of the module docstring as W.apply takes it"""
    out = dict(spec, lj=[(0, 0) + LJ00, (0, 1) + LJ01], tables=[(1, 1) + table_11() + (RC, itype)])
    if coulomb:
        out["coulomb"] = [(a, b, k, rcq) for a, b in MASK]
    return out


def matrix(itype=1):
    return {(0, 0): S.lj(*LJ00), (0, 1): S.lj(*LJ01), (1, 1): ("tab", S.Table(*table_11(), itype), RC)}


def term_gap(pos, box, types_, q, rcq, excluded=()):
    """smallest | r - rc_qq | over the pairs that carry a non-zero Coulomb term"""
    live = np.nonzero(np.asarray(q) != 0.0)[0]
    idx = {int(t): k for k, t in enumerate(live)}
    ex = [(idx[a], idx[b]) for a, b in excluded if a in idx and b in idx]
    gap = np.inf
    ty = np.asarray(types_)[live]
    for t1, t2 in MASK:                                           # one type pair at a time: the others' pairs do not count
        sel = np.nonzero((ty == t1) | (ty == t2))[0]
        sub = {int(s): k for k, s in enumerate(sel)}
        exs = [(sub[a], sub[b]) for a, b in ex if a in sub and b in sub]
        p, tt = np.asarray(pos)[live][sel], ty[sel]
        if len(p) < 2:
            continue
        iu = np.triu_indices(len(p), 1)
        d = p[iu[0]] - p[iu[1]]
        d -= np.asarray(box) * np.rint(d / np.asarray(box))
        ok = ((tt[iu[0]] == t1) & (tt[iu[1]] == t2)) | ((tt[iu[0]] == t2) & (tt[iu[1]] == t1))
        for a, b in exs:
            ok &= ~((iu[0] == min(a, b)) & (iu[1] == max(a, b)))
        if ok.any():
            gap = min(gap, np.abs(np.sqrt((d * d).sum(1))[ok] - rcq).min())
    return gap


def guard(pos, box, types_, q, rcq, itype=1, excluded=(), k=KQ):
    """the reference of this configuration; asserts that the Coulomb part is far from negligible and that no pair with a
    term sits at the cutoff"""
    ref = Q.total(pos, box, types_, q, matrix(itype), k, rcq, set(MASK), excluded)
    part, gap = np.abs(ref["Fq"]).max() / np.abs(ref["F"]).max(), term_gap(pos, box, types_, q, rcq, excluded)
    print("Coulomb part %.3e of the largest force, nearest charged pair %.3e from rc_qq" % (part, gap))
    assert part > 1e-2
    assert gap > 1e-4
    return ref


def check(g, spec, prec, ref, rcq, itype=1, tol_f=None, extra_f=None):
    """forces, Coulomb energy and virial, virial_nb, and the LJ / table energies that keep their meaning"""
    tol_f = TOL_F if tol_f is None else tol_f
    g.run(0)
    F = ref["F"] if extra_f is None else ref["F"] + extra_f
    fg, ob, (eq, wq) = g.get_state("FORCE"), g.observe(), g.get_coulomb()
    if prec == 64:
        err, flips = rel_err(fg, F), 0
    else:
        s = dict(pair_spec(spec, rcq, itype, coulomb=False), pos=g.get_state("POS"))
        s["tables"] = [t[:7] for t in s["tables"]]
        err, flips = force_error_without_cutoff_flips(s, fg, F, tol_f[32], max_flips=0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    print("prec %d rc_qq %.1f: force rel err %.3e flips %d, e_q %.3e w_q %.3e virial_nb %.3e epot_lj %.3e epot_tab %.3e" %
          (prec, rcq, err, flips, rel(eq, ref["e_q"]), rel(wq, ref["w_q"]), rel(ob["virial_nb"], ref["w_nb"]), rel(ob["epot_lj"], ref["e_lj"]), rel(ob["epot_tab"], ref["e_tab"])))
    assert err < tol_f[prec] and flips == 0
    assert eq == pytest.approx(ref["e_q"], rel=TOL_E[prec]) and wq == pytest.approx(ref["w_q"], rel=TOL_E[prec])
    assert ob["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[prec])
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec]) and ob["epot_tab"] == pytest.approx(ref["e_tab"], rel=TOL_E[prec])


# ---- 1: forces, energy and virials at step 0 -----------------------------------------------------------------------------------

_REF = {}


def static_ref(shape, rcq):
    """computed once, shared by both precisions"""
    if (shape, rcq) not in _REF:
        spec = system(shape)
        _REF[(shape, rcq)] = (spec, guard(spec["pos"], spec["box"], spec["types"], spec["q"], rcq))
    return _REF[(shape, rcq)]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("rcq", [1.2, 1.5])
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_static_forces_energy_and_virials(make_gpu, shape, rcq, prec):
    spec, ref = static_ref(shape, rcq)
    g = make_gpu(prec)
    W.apply(pair_spec(spec, rcq), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref, rcq)
    assert np.array_equal(g.get_state("CHARGE"), spec["q"])


# ---- 2: exclusions ----------------------------------------------------------------------------------------------------------

def close_pairs(spec, rmax, count, seed=8, disjoint=False):
    """`count` random pairs closer than rmax, as 0-based index pairs (disjoint: no particle twice)"""
    pos, box = spec["pos"], np.asarray(spec["box"])
    iu = np.triu_indices(len(pos), 1)
    d = pos[iu[0]] - pos[iu[1]]
    d -= box * np.rint(d / box)
    near = np.nonzero((d * d).sum(1) < rmax * rmax)[0]
    near = near[np.random.default_rng(seed).permutation(len(near))]
    out, used = [], set()
    for k in near:
        a, b = int(iu[0][k]), int(iu[1][k])
        if disjoint and (a in used or b in used):
            continue
        out.append((a, b)); used.update((a, b))
        if len(out) == count:
            break
    assert len(out) == count
    return out


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_excluded_pairs_contribute_nothing(make_gpu, shape, prec):
    """300 random close pairs excluded; the 1-1 table is a natural cubic spline here (MODE 4 / COUL evaluate kind 3)"""
    spec, rcq, itype = system(shape), 1.2, 3
    ex = close_pairs(spec, 0.8, 300)
    ref = guard(spec["pos"], spec["box"], spec["types"], spec["q"], rcq, itype, excluded=ex)
    full = Q.coulomb_sums(spec["pos"], spec["box"], spec["types"], spec["q"], KQ, rcq, set(MASK))[0]
    assert rel_err(full, ref["Fq"]) > 1e-2                       # the excluded pairs did carry a visible part of the term
    g = make_gpu(prec)
    W.apply(dict(pair_spec(spec, rcq, itype), exclusions=[(a + 1, b + 1) for a, b in ex]), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref, rcq, itype)


# ---- 3: harmonic dimers: the configuration that would otherwise run its bonds inline -------------------------------------------

BOND_K, BOND_R0 = 40.0, 0.7


@pytest.mark.parametrize("prec", [64, 32])
def test_dimers_whose_bonds_are_the_exclusions(make_gpu, prec):
    spec, rcq = system("a"), 1.5
    bonds = close_pairs(spec, 0.8, 400, seed=9, disjoint=True)
    ref = guard(spec["pos"], spec["box"], spec["types"], spec["q"], rcq, excluded=bonds)
    Fb, eb = S.bond_terms(spec["pos"], np.asarray(spec["box"]), bonds, lambda r: (BOND_K * (r - BOND_R0) ** 2, -2.0 * BOND_K * (r - BOND_R0)))
    ids = [(a + 1, b + 1) for a, b in bonds]
    g = make_gpu(prec)
    h = W.apply(dict(pair_spec(spec, rcq), exclusions=ids, lists=[dict(arity=2, kind="HARMONIC", params=[BOND_K, BOND_R0], ids=ids)]),
                g, thermostat=False, reactions=False)
    check(g, spec, prec, ref, rcq, tol_f=TOL_FB, extra_f=Fb)
    assert g.observe()["epot_list"][h[0]] == pytest.approx(eb, rel=TOL_E[prec])


# ---- 4: after motion and list rebuilds ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_after_motion_and_rebuilds(make_gpu, prec):
    spec, rcq = system("a", seed=SEED_MOTION[prec], kT=0.3), 1.2
    g = make_gpu(prec)
    W.apply(pair_spec(spec, rcq, k=KQ_MOTION), g, thermostat=False, reactions=False)
    g.run(200)
    tm = g.timers()
    print("rebuilds", tm["rebuilds"], "list rebuilds", tm["list_rebuilds"])
    assert tm["list_rebuilds"] >= 2
    x = g.get_state("POS")
    ref = guard(x, spec["box"], spec["types"], spec["q"], rcq, k=KQ_MOTION)
    check(g, spec, prec, ref, rcq)


def test_after_motion_on_two_slabs(make_gpu):
    spec, rcq, P = system("slab", seed=SEED_MOTION["slab"], kT=0.3), 1.2, 2
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        W.apply(pair_spec(spec, rcq, k=KQ_MOTION), g, thermostat=False, reactions=False)
        g.run(200)
        reb = g.timers()["list_rebuilds"]
        g.run(0)
        return dict(x=g.get_state("POS"), f=g.get_state("FORCE"), ob=g.observe(), qq=g.get_coulomb(), reb=reb, q=g.get_state("CHARGE"))
    out = _run_ranks(P, rank)
    assert np.array_equal(out[0]["x"], out[1]["x"])
    ref = guard(out[0]["x"], spec["box"], spec["types"], spec["q"], rcq, k=KQ_MOTION)
    for r in range(P):
        print("rank %d: rebuilds %d, force rel err %.3e" % (r, out[r]["reb"], rel_err(out[r]["f"], ref["F"])))
        assert out[r]["reb"] >= 2
        assert rel_err(out[r]["f"], ref["F"]) < TOL_F[64]
        assert out[r]["qq"][0] == pytest.approx(ref["e_q"], rel=TOL_E[64]) and out[r]["qq"][1] == pytest.approx(ref["w_q"], rel=TOL_E[64])
        assert out[r]["ob"]["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[64])
        assert np.array_equal(out[r]["q"], spec["q"])


# ---- 5: charge changes -------------------------------------------------------------------------------------------------------

REACT_CUT = 0.6


def reacting_pairs(spec):
    """type-0 / type-2 pairs closer than REACT_CUT in which neither particle has another such partner: with an infinite rate
    exactly these react; (index of the type-0 particle, index of the type-2 particle)"""
    pos, box, ty = spec["pos"], np.asarray(spec["box"]), spec["types"]
    iu = np.triu_indices(len(pos), 1)
    d = pos[iu[0]] - pos[iu[1]]
    d -= box * np.rint(d / box)
    r = np.sqrt((d * d).sum(1))
    hit = np.nonzero((r < REACT_CUT) & (((ty[iu[0]] == 0) & (ty[iu[1]] == 2)) | ((ty[iu[0]] == 2) & (ty[iu[1]] == 0))))[0]
    assert np.abs(r[hit] - REACT_CUT).min() > 1e-4
    members = np.concatenate([iu[0][hit], iu[1][hit]])
    assert len(set(members.tolist())) == len(members)            # isolated candidate pairs: nothing to resolve
    return [(int(a), int(b)) if ty[a] == 0 else (int(b), int(a)) for a, b in zip(iu[0][hit], iu[1][hit])]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_charges_change_through_a_reaction_and_modify_particle(make_gpu, shape, prec):
    """A virtual reaction 0 + 2 -> 1 + 2 with new_q 0.75 / -0.25 at an infinite rate, one step of 1e-5 from rest (the
    particles move by ~1e-9), then chem_modify_particle(CHARGE) on three particles.  After each: the read-back of
    CHEM_STATE_CHARGE equals the host rule and the forces are the reference's with the new charges and types."""
    spec, rcq = system(shape, dt=1e-5, vel=False), 1.2
    pairs = reacting_pairs(spec)
    print("reacting pairs:", len(pairs))
    assert 3 <= len(pairs) <= 60
    g = make_gpu(prec)
    W.apply(pair_spec(spec, rcq), g, thermostat=False, reactions=False)
    g.reaction_init(1, nearest=True, seed=4)
    g.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=1e30, cutoff=REACT_CUT, is_virtual=True, intramolecular=True, intraresidual=True,
                   new_type_1=1, new_type_2=2, new_mass_1=1.0, new_mass_2=1.0, new_q_1=0.75, new_q_2=-0.25)
    g.reactions_enable(True)
    g.run(0)
    assert np.array_equal(g.get_state("CHARGE"), spec["q"])
    g.run(1)
    ev = g.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev) == sorted(pairs)
    q, ty = spec["q"].copy(), spec["types"].copy()
    for a, b in pairs:                                           # the host rule: the reaction names a new type for both roles
        q[a], q[b], ty[a] = 0.75, -0.25, 1
    assert np.array_equal(g.get_state("CHARGE"), q) and np.array_equal(g.get_state("TYPE"), ty)
    g.reactions_enable(False)
    x = g.get_state("POS")
    assert np.abs(x - spec["pos"]).max() < 1e-6
    ref = guard(x, spec["box"], ty, q, rcq)
    assert rel_err(ref["F"], Q.total(x, spec["box"], ty, spec["q"], matrix(), KQ, rcq, set(MASK))["F"]) > 1e-3      # the old charges are far off
    check(g, dict(spec, types=ty), prec, ref, rcq)
    # modifyParticle: a neutral particle gets a charge, a charged one loses it, one flips its sign
    neutral, charged = np.nonzero(q == 0.0)[0], np.nonzero(q != 0.0)[0]
    for i, v in ((int(neutral[5]), -1.0), (int(charged[7]), 0.0), (int(charged[11]), -q[charged[11]])):
        g.modify_particle(i + 1, "CHARGE", v)
        q[i] = v
    assert np.array_equal(g.get_state("CHARGE"), q)
    ref2 = guard(x, spec["box"], ty, q, rcq)
    assert rel_err(ref2["F"], ref["F"]) > 1e-3
    check(g, dict(spec, types=ty), prec, ref2, rcq)


def test_shim_storage_reads_and_modifies_the_charge(make_gpu):
    """storage.getParticle(pid).q is the particle's charge and storage.modifyParticle(pid, 'q', v) changes it"""
    import types
    from chemlab_amd import espp
    spec = system("c")
    g = make_gpu(64)
    W.apply(pair_spec(spec, 1.2), g, thermostat=False, reactions=False)
    g.run(0)
    storage = types.SimpleNamespace(system=types.SimpleNamespace(engine=g), _ids=spec["ids"])
    pid = int(np.nonzero(spec["q"] != 0.0)[0][3]) + 1
    assert espp.storage.DomainDecomposition.getParticle(storage, pid).q == spec["q"][pid - 1]
    espp.storage.DomainDecomposition.modifyParticle(storage, pid, "q", 0.25)
    assert espp.storage.DomainDecomposition.getParticle(storage, pid).q == 0.25
    assert g.get_state("CHARGE")[pid - 1] == 0.25


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu):
    spec = system("a")
    g = make_gpu(64)
    W.apply(pair_spec(spec, 1.2), g, thermostat=False, reactions=False)
    with pytest.raises(ChemError, match="share one") as ei:         # a second (prefactor, rc)
        g.nb_coulomb(2, 2, KQ, 1.0)
    assert ei.value.code == _capi.ENOTIMPL
    with pytest.raises(ChemError, match="share one") as ei:
        g.nb_coulomb(2, 2, 2.0 * KQ, 1.2)
    assert ei.value.code == _capi.ENOTIMPL
    g.run(0)
    for opt, bad, good in (("tpp", 2, 0), ("pair_block", 256, 512)):
        g.set_option(opt, bad)
        with pytest.raises(ChemError, match=opt) as ei:
            g.run(0)
        assert ei.value.code == _capi.EINVAL
        g.set_option(opt, good)
        g.run(0)
    g2 = make_gpu(64)                                               # rc_qq beyond the list cutoff: refused at run(), naming the type pair
    W.apply(pair_spec(spec, 1.6), g2, thermostat=False, reactions=False)
    with pytest.raises(ChemError, match=r"type pair \(0,0\).*max_cutoff") as ei:
        g2.run(0)
    assert ei.value.code == _capi.EINVAL


# ---- 7: removing the registration --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_removed_registration_is_bit_identical_to_none(make_gpu, shape, prec):
    """prefactor = 0 on every pair brings back the forces of a context that never registered the term, bit for bit (both
    contexts have built their lists twice: the second context through a geometry option that changes nothing)"""
    spec = system(shape)
    g, plain = make_gpu(prec), make_gpu(prec)
    W.apply(pair_spec(spec, 1.2), g, thermostat=False, reactions=False)
    W.apply(pair_spec(spec, 1.2, coulomb=False), plain, thermostat=False, reactions=False)
    g.run(0); plain.run(0)
    assert rel_err(g.get_state("FORCE"), plain.get_state("FORCE")) > 1e-2
    for a, b in MASK:
        g.nb_coulomb(a, b, 0.0, 1.2)
    plain.set_option("tiles", 1)
    g.run(0); plain.run(0)
    assert np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    assert g.get_coulomb() == (0.0, 0.0)
    og, op = g.observe(), plain.observe()
    assert og["epot_lj"] == op["epot_lj"] and og["epot_tab"] == op["epot_tab"] and og["virial_nb"] == op["virial_nb"]
    g.run(5); plain.run(5)
    assert np.array_equal(g.get_state("POS"), plain.get_state("POS"))
