"""1-4 Coulomb pair lists on the HIP path (CHEM_POT_COULOMB_BOND: k_bonded_work_q, k_bonded_q, the by-tag charge array kept
alive by the list).  Rule set: include/chem_mi355.h.

The CPU oracle has no Coulomb term.  Reference: the oracle on the same configuration WITHOUT the Coulomb list plus the
per-entry terms of tests/coulomb14_ref.py (numpy, imports nothing from the product); where chem_nb_coulomb is on as well, the
brute-force tests/coulomb_ref.py total plus the bonds and 1-4 LJ pairs from tests/spline_ref.py bond_terms.

System: the jittered lattice of tests/test_gpu_coulomb.py (spacing 0.75, jitter +-0.1, first layer 0.1 behind the low faces,
rc 1.5, skin 0.3, its non-bonded matrix) cut into 2x2x1 blocks of four sites, each block a tetramer: harmonic bonds 1-2, 2-3,
3-4 (K 40, r0 0.75), exclusions 1-2, 1-3, 1-4, an LJ 1-4 list (eps 0.5, sigma 0.5, cutoff 1.5) and a Coulomb 1-4 list on
(1, 4).  Alternate blocks are ordered (0,0),(1,0),(1,1),(0,1) (1-4 distance ~0.75) and (0,0),(1,0),(0,1),(1,1) (~1.06);
rc_14 = 0.9 lies between.  Charges from {-1, -0.5, 0, 0.417, 0.5, 1}, a quarter neutral; 0.417 is not an fp32 value.
Shapes: (a) 9.0^3, 1728 particles, 432 tetramers: tiles, k_bonded_work_q.  (c) 5.4^3, 343 particles, 63 tetramers + 91
monomers: k_pair_force, k_bonded_q.  (slab) (9, 9, 18), 3456 particles on two in-process ranks, blocks in the x-z plane so
that 1-4 pairs cross the slab border.  k = 20 (5 where a test integrates).

Every force test first asserts on the CPU (guard14): at least a quarter of the pairs with q_i q_j != 0 inside rc_14 and a
quarter outside; none within 1e-4 of rc_14; a listed pair through a periodic face; the 1-4 Coulomb part above 1e-2 of the
largest force -- no test can pass with the term missing.  Seeds: SEED below (gaps on the CPU: a 4.6e-3, c 1.7e-2, slab
2.3e-3).

Tolerances are the project's: forces TOL[64] = 1e-10 / TOL_STIFF32 = 5e-5 of the largest force, list energy 1e-11 / 1e-5.
Measured on an MI355X when the path was built: static configurations (all tests but the two below), forces fp64 up to
7.2e-16, fp32 up to 4.4e-07 of the largest force, list energy fp64 up to 1.5e-14, fp32 up to 5.4e-8; after 200 steps (9 list
builds) forces fp64 8.7e-15, fp32 4.1e-6; two slabs against one domain (10 list builds): identical to the bit at step 0 and
after 200 steps; the reaction of the charge test gave 147 (a) and 38 (c) events."""
import numpy as np
import pytest

import coulomb14_ref as C14
import coulomb_ref as Q
import hybrid_ref as H
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from test_gpu_coulomb import KQ, MASK, matrix, pair_spec
from test_gpu_parity import TOL, TOL_STIFF32, _HUB, _run_ranks
from test_gpu_spline_tables import BOXES, DT, RC, SKIN

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_STIFF32}
TOL_E = {64: 1e-11, 32: 1e-5}
K14, RC14 = 20.0, 0.9
K14_MOTION = 5.0            # weak enough that no particle crosses a slab layer between two list builds
BOND_K, BOND_R0 = 40.0, 0.75
LJ14 = (0.5, 0.5, 1.5)
RCQ = 1.2
REACT_CUT = 0.7             # enough 0 + 2 pairs of different tetramers react in the small shape too that 1-4 entries feel it
CHARGES, WEIGHTS = (-1.0, -0.5, 0.0, 0.417, 0.5, 1.0), (0.15, 0.15, 0.25, 0.15, 0.15, 0.15)
SEED = {"a": 1, "c": 2, "slab": 5}
SEED_MOTION = {64: 3, 32: 3, "slab": 5}
ORDERS = (((0, 0), (1, 0), (1, 1), (0, 1)), ((0, 0), (1, 0), (0, 1), (1, 1)))


# ---- the system ------------------------------------------------------------------------------------------------------------

def system14(shape, seed=None, kT=1.0, dt=DT, vel=True):
    """spec WITHOUT the Coulomb list (what the oracle gets) with the non-bonded matrix of test_gpu_coulomb (no Coulomb term);
    spec["tet"]: the tetramers as rows of four 0-based indices, spec["p14"]: their (1, 4) pairs"""
    box = np.array(BOXES[shape])
    rng = np.random.default_rng(SEED[shape] if seed is None else seed)
    k = np.floor(box / 0.75 + 1e-9).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3)
    index = np.arange(len(g)).reshape(k)
    pos = g * 0.75 - 0.1 + rng.uniform(-0.1, 0.1, g.shape)
    n = len(pos)
    types_ = rng.integers(0, 3, n).astype(np.int32)
    q = rng.choice(CHARGES, n, p=WEIGHTS)
    v = rng.normal(0.0, np.sqrt(kT), (n, 3))
    u, w = (0, 2) if shape == "slab" else (0, 1)                  # the block's plane
    t = 3 - u - w
    tet = []
    for lt in range(k[t]):
        for bu in range(k[u] // 2):
            for bw in range(k[w] // 2):
                row = []
                for du, dw in ORDERS[(bu + bw + lt) % 2]:
                    c = [0, 0, 0]
                    c[u], c[w], c[t] = 2 * bu + du, 2 * bw + dw, lt
                    row.append(int(index[tuple(c)]))
                tet.append(row)
    tet = np.array(tet, dtype=np.int64)
    bonds = np.concatenate([tet[:, [0, 1]], tet[:, [1, 2]], tet[:, [2, 3]]])
    p14 = tet[:, [0, 3]]
    excl = np.concatenate([bonds, tet[:, [0, 2]], p14])
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=dt, ids=np.arange(1, n + 1), types=types_, q=q,
                pos=pos, vel=v if vel else np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), kT=kT, gamma=0.0, seed=1, rebuild_criterion=1,
                lists=[dict(arity=2, kind="HARMONIC", params=[BOND_K, BOND_R0], ids=bonds + 1),
                       dict(arity=2, kind="LJ_BOND", params=list(LJ14), ids=p14 + 1)],
                exclusions=excl + 1)
    spec = pair_spec(W.snap_to_grid(spec), RCQ, coulomb=False)
    spec.update(tet=tet, p14=p14, bonds=bonds, excl=excl)
    return spec


def add_c14(g, spec, k=K14, rc=RC14, typed=None, hybrid=None, pairs=None):
    h = g.list_create(2, "COULOMB_BOND", typed is not None)
    if typed is None:
        g.list_set_params(h, [k, rc])
    else:
        for tt, p in typed.items():
            g.list_set_params(h, list(p), types=tt)
    if hybrid is not None:
        g.list_set_hybrid(h, *hybrid)
    g.list_add(h, (spec["p14"] if pairs is None else np.asarray(pairs)) + 1)
    return h


def build(make_gpu, spec, prec, coulomb_nb=False, **kw):
    g = make_gpu(prec)
    s = dict(spec, coulomb=[(a, b, KQ, RCQ) for a, b in MASK]) if coulomb_nb else spec
    W.apply(s, g, thermostat=False, reactions=False)
    return g, add_c14(g, spec, **kw)


def oracle_forces(make_oracle, spec, **over):
    """forces of the oracle on `spec` (no Coulomb list, no Coulomb term) with pos / types / lists / exclusions replaced"""
    o = make_oracle()
    s = dict(spec, **over)
    s.pop("coulomb", None)
    W.apply(s, o, thermostat=False, reactions=False)
    o.run(0)
    F = o.get_state("FORCE")
    o.close()
    return F


def lj14_fun(eps, sig, rc):
    def fun(r):
        s6, c6 = (sig / r) ** 6, (sig / rc) ** 6
        inside = r <= rc
        return np.where(inside, 4.0 * eps * ((s6 * s6 - s6) - (c6 * c6 - c6)), 0.0), np.where(inside, 24.0 * eps * (2.0 * s6 * s6 - s6) / r, 0.0)
    return fun


def harmonic_fun(r):
    return BOND_K * (r - BOND_R0) ** 2, -2.0 * BOND_K * (r - BOND_R0)


def guard14(pos, box, q, pairs, Fref, F14, rc14=RC14, label=""):
    """the conditions of the module docstring on this configuration"""
    box = np.asarray(box)
    b, d, r = C14.distances(pos, box, pairs)
    live = C14.live(q, pairs)
    n_in, n_out = int((r[live] <= rc14).sum()), int((r[live] > rc14).sum())
    gap = np.abs(r[live] - rc14).min()
    raw = np.asarray(pos)[b[:, 0]] - np.asarray(pos)[b[:, 1]]
    faces = int((np.abs(raw) > 0.5 * box).any(1).sum())
    part = np.abs(F14).max() / np.abs(Fref).max()
    print("%s 1-4 Coulomb: %d live pairs in, %d out of %d; nearest %.3e from rc_14; %d through a face; part %.3e of the largest force"
          % (label, n_in, n_out, len(b), gap, faces, part))
    assert 4 * n_in >= live.sum() and 4 * n_out >= live.sum()
    assert gap > 1e-4
    assert faces >= 1
    assert part > 1e-2


def stored(q, prec):
    """the charges as the build holds them: the by-tag array has the build's real type"""
    return np.asarray(q, np.float32).astype(np.float64) if prec == 32 else np.asarray(q, np.float64)


def check14(g, h, prec, Fref, e14, label=""):
    g.run(0)
    err = rel_err(g.get_state("FORCE"), Fref)
    el = g.observe()["epot_list"][h]
    print("%s prec %d: force rel err %.3e, list energy rel err %.3e" % (label, prec, err, abs(el - e14) / max(abs(e14), 1e-300)))
    assert err < TOL_F[prec]
    assert el == pytest.approx(e14, rel=TOL_E[prec], abs=1e-12)


_REF = {}


def static_ref(make_oracle, shape):
    """computed once per shape, shared and left unchanged: spec, oracle forces, 1-4 Coulomb forces and energy"""
    if shape not in _REF:
        spec = system14(shape, vel=False)
        Fo = oracle_forces(make_oracle, spec)
        F14, e14 = C14.terms(spec["pos"], spec["box"], spec["q"], spec["p14"], K14, RC14)
        guard14(spec["pos"], spec["box"], spec["q"], spec["p14"], Fo + F14, F14, label=shape)
        for a in (Fo, F14):
            a.setflags(write=False)
        _REF[shape] = (spec, Fo, F14, e14)
    return _REF[shape]


def test_shapes():
    for shape, n, ntet in (("a", 1728, 432), ("c", 343, 63), ("slab", 3456, 864)):
        spec = system14(shape)
        assert spec["n"] == n and len(spec["tet"]) == ntet and len(set(spec["tet"].ravel().tolist())) == 4 * ntet
        assert abs((spec["q"] == 0.0).mean() - 0.25) < 0.08 and float(np.float32(0.417)) != 0.417


# ---- 1: static forces and list energy --------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_static_forces_and_list_energy(make_gpu, make_oracle, shape, prec):
    spec, Fo, F14, e14 = static_ref(make_oracle, shape)
    g, h = build(make_gpu, spec, prec)
    check14(g, h, prec, Fo + F14, e14, shape)
    assert np.array_equal(g.get_state("CHARGE"), stored(spec["q"], prec))
    assert g.get_coulomb() == (0.0, 0.0)                                    # chem_get_coulomb keeps meaning the non-bonded term
    # the pair kernel runs in the mode it has without any Coulomb term: the MODE 4 restriction of the options does not apply
    for opt, value in (("tpp", 2), ("pair_block", 256)):
        g.set_option(opt, value)
        check14(g, h, prec, Fo + F14, e14, "%s %s=%d" % (shape, opt, value))


# ---- 2: together with the non-bonded term, and after its removal -------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_with_the_non_bonded_term_and_after_its_removal(make_gpu, shape, prec):
    spec = system14(shape, vel=False)
    x, box, ty, q = spec["pos"], np.asarray(spec["box"]), spec["types"], spec["q"].copy()
    Fb = S.bond_terms(x, box, spec["bonds"], harmonic_fun)[0] + S.bond_terms(x, box, spec["p14"], lj14_fun(*LJ14))[0]

    def reference(q, coulomb):
        ref = Q.total(x, box, ty, q, matrix(), KQ, RCQ, set(MASK), [tuple(p) for p in spec["excl"].tolist()])
        F14, e14 = C14.terms(x, box, q, spec["p14"], K14, RC14)
        Fnb = ref["F"] if coulomb else ref["F"] - ref["Fq"]
        guard14(x, box, q, spec["p14"], Fnb + Fb + F14, F14, label=shape)
        return Fnb + Fb + F14, e14, ref
    g, h = build(make_gpu, spec, prec, coulomb_nb=True)
    F, e14, ref = reference(q, True)
    assert np.abs(ref["Fq"]).max() > 1e-2 * np.abs(F).max()
    check14(g, h, prec, F, e14, shape + " MODE 4")
    assert g.get_coulomb()[0] == pytest.approx(ref["e_q"], rel=TOL_E[prec])
    # a charge changes, then the non-bonded term goes: the 1-4 term is still there and the charges survive
    inside = C14.live(q, spec["p14"]) & (C14.distances(x, box, spec["p14"])[2] <= RC14)
    i = int(spec["p14"][np.nonzero(inside)[0][3], 0])
    g.modify_particle(i + 1, "CHARGE", -q[i])
    q[i] = -q[i]
    for a, b in MASK:
        g.nb_coulomb(a, b, 0.0, RCQ)
    F2, e2, _ = reference(q, False)
    check14(g, h, prec, F2, e2, shape + " term removed")
    assert np.array_equal(g.get_state("CHARGE"), stored(q, prec)) and g.get_coulomb() == (0.0, 0.0)
    assert abs(e2 - e14) > 1e-3 * abs(e14)


# ---- 3: by types -----------------------------------------------------------------------------------------------------------

TYPED = {(0, 0): (20.0, 0.9), (2, 1): (12.0, 1.2)}


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_types_list_follows_the_current_types(make_gpu, make_oracle, shape, prec):
    spec, Fo, _, _ = static_ref(make_oracle, shape)
    ty, p14, q = spec["types"].copy(), spec["p14"], spec["q"]

    def reference(ty, Fo):
        F14, e14 = C14.terms(spec["pos"], spec["box"], q, p14, types=ty, typed=TYPED)
        kk, rr = C14.entry_params(p14, 0, 1, ty, TYPED)
        _, _, r = C14.distances(spec["pos"], spec["box"], p14)
        sel = C14.live(q, p14) & (kk != 0)
        assert sel.sum() >= 4 and np.abs(r[sel] - rr[sel]).min() > 1e-4 and len(set(kk[sel].tolist())) == 2
        assert np.abs(F14).max() > 1e-2 * np.abs(Fo + F14).max()
        return F14, e14, kk != 0
    g, h = build(make_gpu, spec, prec, typed=TYPED)
    F14, e14, had = reference(ty, Fo)
    check14(g, h, prec, Fo + F14, e14, shape + " typed")
    # entries move between "has parameters" and "has none": type 0 -> 2 on members of (0, 0) entries, 1 -> 2 on members of (1, 1)
    t0, t1 = ty[p14[:, 0]], ty[p14[:, 1]]
    lose = p14[np.nonzero((t0 == 0) & (t1 == 0))[0][:5], 0]
    gain = p14[np.nonzero((t0 == 1) & (t1 == 1))[0][:5], 1]
    for i in np.concatenate([lose, gain]).tolist():
        g.modify_particle(i + 1, "TYPE", 2)
        ty[i] = 2
    Fo2 = oracle_forces(make_oracle, spec, types=ty)
    F14b, e14b, has = reference(ty, Fo2)
    assert (had & ~has).sum() >= 3 and (~had & has).sum() >= 3
    check14(g, h, prec, Fo2 + F14b, e14b, shape + " typed, types changed")


# ---- 4: charge changes act at the next evaluation ----------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_charge_changes_act_at_the_next_evaluation(make_gpu, make_oracle, shape, prec):
    """chem_modify_particle(CHARGE) on 20 members of live entries with no list build in between, then a virtual reaction
    0 + 2 -> 1 + 2 with new_q 0.75 / -0.25 at an infinite rate (one step of 1e-5 from rest).  After each: forces and list
    energy are the reference's with the new charges."""
    spec = system14(shape, dt=1e-5, vel=False)
    x, box, p14, q, ty = spec["pos"], spec["box"], spec["p14"], spec["q"].copy(), spec["types"].copy()
    Fo = oracle_forces(make_oracle, spec)
    g, h = build(make_gpu, spec, prec)
    g.reaction_init(1, nearest=True, seed=4)
    g.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=1e30, cutoff=REACT_CUT, is_virtual=True, intramolecular=True, intraresidual=True,
                   new_type_1=1, new_type_2=2, new_mass_1=1.0, new_mass_2=1.0, new_q_1=0.75, new_q_2=-0.25)
    F14, e14 = C14.terms(x, box, q, p14, K14, RC14)
    guard14(x, box, q, p14, Fo + F14, F14, label=shape)
    check14(g, h, prec, Fo + F14, e14, shape)
    builds = g.timers()["list_rebuilds"]
    members = p14[np.nonzero(C14.live(q, p14))[0][:20], 0]
    for n_, i in enumerate(members.tolist()):
        v = (0.0, -q[i], 0.417 if q[i] != 0.417 else 1.0)[n_ % 3]
        g.modify_particle(i + 1, "CHARGE", v)
        q[i] = v
    F14b, e14b = C14.terms(x, box, q, p14, K14, RC14)
    assert rel_err(F14b, F14) > 1e-2
    check14(g, h, prec, Fo + F14b, e14b, shape + " modify_particle")
    assert g.timers()["list_rebuilds"] == builds and np.array_equal(g.get_state("CHARGE"), stored(q, prec))
    # the reaction
    g.reactions_enable(True)
    g.run(1)
    g.reactions_enable(False)
    ev = [(int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in g.get_events()]
    print("reaction events:", len(ev))
    assert len(ev) >= 5
    for a, b in ev:                                              # the host rule: the reaction names a new type for both roles
        a, b = (a, b) if ty[a] == 0 else (b, a)
        assert ty[a] == 0 and ty[b] == 2
        q[a], q[b], ty[a] = 0.75, -0.25, 1
    assert np.array_equal(g.get_state("CHARGE"), stored(q, prec)) and np.array_equal(g.get_state("TYPE"), ty)
    x2 = g.get_state("POS")
    assert np.abs(x2 - x).max() < 1e-6
    Fo2 = oracle_forces(make_oracle, spec, pos=x2, types=ty)
    F14c, e14c = C14.terms(x2, box, q, p14, K14, RC14)
    guard14(x2, box, q, p14, Fo2 + F14c, F14c, label=shape + " reacted")
    assert rel_err(F14c, C14.terms(x2, box, spec["q"], p14, K14, RC14)[0]) > 1e-3       # the charges of the start are far off
    assert np.abs(F14c - F14b).max() > 1e-3 * np.abs(F14c).max()
    check14(g, h, prec, Fo2 + F14c, e14c, shape + " reaction")


# ---- 5: after motion and list builds -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_after_motion_and_list_builds(make_gpu, make_oracle, prec):
    spec = system14("a", seed=SEED_MOTION[prec], kT=0.3)
    g, h = build(make_gpu, spec, prec, k=K14_MOTION)
    g.run(200)
    builds = g.timers()["list_rebuilds"]
    print("list builds", builds)
    assert builds >= 5
    x = g.get_state("POS")
    Fo = oracle_forces(make_oracle, spec, pos=x, vel=g.get_state("VEL"))
    F14, e14 = C14.terms(x, spec["box"], spec["q"], spec["p14"], K14_MOTION, RC14)
    guard14(x, spec["box"], spec["q"], spec["p14"], Fo + F14, F14, label="after 200 steps")
    check14(g, h, prec, Fo + F14, e14, "after 200 steps")
    # a split run is the same run
    g2, _ = build(make_gpu, spec, prec, k=K14_MOTION)
    g2.run(120); g2.run(80)
    assert np.array_equal(g2.get_state("POS"), x) and np.array_equal(g2.get_state("VEL"), g.get_state("VEL"))


# ---- 6: two slabs ------------------------------------------------------------------------------------------------------------

def test_two_slabs_equal_one_domain(make_gpu, make_oracle):
    spec, P = system14("slab", seed=SEED_MOTION["slab"], kT=0.3), 2
    x0, box, p14, q = spec["pos"], np.asarray(spec["box"]), spec["p14"], spec["q"]
    Fo = oracle_forces(make_oracle, spec)
    F14, e14 = C14.terms(x0, box, q, p14, K14_MOTION, RC14)
    guard14(x0, box, q, p14, Fo + F14, F14, label="slab")
    z = x0[:, 2] - np.floor(x0[:, 2] / box[2]) * box[2]
    owner = (z >= 0.5 * box[2]).astype(int)
    crossing = int((owner[p14[:, 0]] != owner[p14[:, 1]]).sum())
    print("listed pairs with members on different ranks:", crossing)
    assert crossing >= 10

    def one(g):
        W.apply(spec, g, thermostat=False, reactions=False)
        h = add_c14(g, spec, k=K14_MOTION)
        g.run(0)
        out = dict(f0=g.get_state("FORCE"), e0=g.observe()["epot_list"][h])
        g.run(200)
        out["builds"] = g.timers()["list_rebuilds"]
        g.run(0)
        out.update(x=g.get_state("POS"), f=g.get_state("FORCE"), e=g.observe()["epot_list"][h], q=g.get_state("CHARGE"))
        return out
    single = one(make_gpu(64))
    assert rel_err(single["f0"], Fo + F14) < TOL[64] and single["e0"] == pytest.approx(e14, rel=TOL_E[64])
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        engs[r].comm_init_local(P, r, hub)
        return one(engs[r])
    out = _run_ranks(P, rank)
    for r in range(P):
        e0, e1 = rel_err(out[r]["f0"], single["f0"]), rel_err(out[r]["f"], single["f"])
        print("rank %d: %d list builds; forces against one domain: step 0 %.3e, after 200 steps %.3e" % (r, out[r]["builds"], e0, e1))
        assert out[r]["builds"] >= 2
        assert e0 < TOL[64] and e1 < TOL[64]
        assert out[r]["e0"] == pytest.approx(single["e0"], rel=TOL_E[64]) and out[r]["e"] == pytest.approx(single["e"], rel=TOL_E[64])
        assert np.array_equal(out[r]["q"], q)                      # (fp64 build)
    # ... and the one domain after its 200 steps is right
    x = single["x"]
    Fo2 = oracle_forces(make_oracle, spec, pos=x)
    F14b, e14b = C14.terms(x, box, q, p14, K14_MOTION, RC14)
    guard14(x, box, q, p14, Fo2 + F14b, F14b, label="slab shape after 200 steps")
    assert rel_err(single["f"], Fo2 + F14b) < TOL[64] and single["e"] == pytest.approx(e14b, rel=TOL_E[64])


# ---- 7: hybrid lists ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_next_to_a_hybrid_list_and_as_a_hybrid_list(make_gpu, make_oracle, shape, prec):
    spec, Fo, F14, e14 = static_ref(make_oracle, shape)
    x, box = spec["pos"], spec["box"]
    # (i) the harmonic bonds in a hybrid list at lambda = 0.25 beside the plain Coulomb list
    rest = dict(spec, lists=spec["lists"][1:])
    Fo_rest = oracle_forces(make_oracle, rest)
    g = make_gpu(prec)
    W.apply(rest, g, thermostat=False, reactions=False)
    hh = g.list_create(2, "HARMONIC")
    g.list_set_params(hh, [BOND_K, BOND_R0])
    g.list_set_hybrid(hh, 0.25, 0.0)
    g.list_add(hh, spec["bonds"] + 1)
    h = add_c14(g, spec)
    lam = g.list_get_lambda(hh)
    assert np.array_equal(lam, np.full(len(spec["bonds"]), 0.25))
    Fh, eh = H.bond_terms(x, box, g.get_list(hh) - 1, lam, H.harmonic(BOND_K, BOND_R0))
    assert rel_err(Fo_rest + Fh, Fo) > 1e-2
    check14(g, h, prec, Fo_rest + Fh + F14, e14, shape + " beside a hybrid list")
    assert g.observe()["epot_list"][hh] == pytest.approx(eh, rel=TOL_E[prec])
    # (ii) the Coulomb list itself hybrid: lambda from chem_list_get_lambda
    g2, h2 = build(make_gpu, dict(spec, vel=np.zeros_like(x), dt=1e-5), prec, hybrid=(0.5, 0.125))
    assert np.array_equal(g2.list_get_lambda(h2), np.full(len(spec["p14"]), 0.5))
    g2.run(2)
    lam2 = g2.list_get_lambda(h2)
    assert np.array_equal(lam2, np.full(len(spec["p14"]), 0.75))
    x2 = g2.get_state("POS")
    Fo2 = oracle_forces(make_oracle, spec, pos=x2)
    F14l, e14l = C14.terms(x2, box, spec["q"], g2.get_list(h2) - 1, K14, RC14, lam=lam2)
    full = C14.terms(x2, box, spec["q"], spec["p14"], K14, RC14)[0]
    guard14(x2, box, spec["q"], spec["p14"], Fo2 + F14l, F14l, label=shape + " hybrid")
    assert rel_err(F14l, full) > 0.2
    check14(g2, h2, prec, Fo2 + F14l, e14l, shape + " hybrid Coulomb list")


# ---- 8: a system whose bonds would run inline ---------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_bonds_that_qualify_for_inline_evaluation(make_gpu, make_oracle, prec):
    """one harmonic parameter set, exclusions = bonds (the chain-growth shape of tests/test_gpu_round3.py) and a Coulomb list on
    the next-nearest pairs (1, 3), (2, 4): right forces, and the bonded kernel runs (sampled by the kernel timers), which it
    does not for the same system without the list"""
    base, _, _, _ = static_ref(make_oracle, "a")
    tet = base["tet"]
    nn = np.concatenate([tet[:, [0, 2]], tet[:, [1, 3]]])
    spec = dict(base, lists=base["lists"][:1], exclusions=base["bonds"] + 1, dt=1e-4, vel=np.zeros_like(base["pos"]))
    Fo = oracle_forces(make_oracle, spec)
    F14, e14 = C14.terms(spec["pos"], spec["box"], spec["q"], nn, K14, RC14)      # (0.75 in one block order, 1.06 in the other)
    guard14(spec["pos"], spec["box"], spec["q"], nn, Fo + F14, F14, label="next-nearest")
    launches = {}
    for with_list in (False, True):
        g = make_gpu(prec)
        g.set_option("time_pair_kernel", 1)
        W.apply(spec, g, thermostat=False, reactions=False)
        h = add_c14(g, spec, pairs=nn) if with_list else None
        if with_list:
            check14(g, h, prec, Fo + F14, e14, "inline-shaped system")
        else:
            g.run(0)
            assert rel_err(g.get_state("FORCE"), Fo) < TOL_F[prec]
        g.run(9)
        launches[with_list] = g.timers()["bonded_kernel_launches"]
    print("bonded kernel launches sampled in 9 steps: without the list %d, with it %d" % (launches[False], launches[True]))
    assert launches[False] == 0 and launches[True] >= 1


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu, make_oracle):
    spec, Fo, _, _ = static_ref(make_oracle, "c")
    g = make_gpu(64)
    W.apply(spec, g, thermostat=False, reactions=False)
    for arity in (3, 4):
        with pytest.raises(ChemError) as ei:
            g.list_create(arity, "COULOMB_BOND")
        assert ei.value.code == _capi.ENOTIMPL
    h = g.list_create(2, "COULOMB_BOND")
    for bad in ([K14], [K14, RC14, 1.0], [K14, 0.0], [K14, -0.9], [float("nan"), RC14], [K14, float("inf")], [float("inf"), RC14]):
        with pytest.raises(ChemError, match="1-4 Coulomb") as ei:
            g.list_set_params(h, bad)
        assert ei.value.code == _capi.EINVAL
    ht = g.list_create(2, "COULOMB_BOND", True)
    with pytest.raises(ChemError, match="1-4 Coulomb") as ei:
        g.list_set_params(ht, [K14, 0.0], types=(0, 1))
    assert ei.value.code == _capi.EINVAL
    # prefactor 0 is a list that does nothing
    g.list_set_params(h, [0.0, RC14])
    g.list_add(h, spec["p14"] + 1)
    g.run(0)
    assert rel_err(g.get_state("FORCE"), Fo) < TOL[64]
    ob = g.observe()
    assert ob["epot_list"][h] == 0.0 and ob["list_size"][h] == len(spec["p14"])
