"""Capped pair potentials on the HIP path (chem_nb_cap: k_pair_tiles_cap / k_pair_tiles_rescap, k_pair_force_cap /
k_pair_force_rescap).  Rule set: include/chem_mi355.h.

The CPU oracle has no cap radius, so the rule set is restated in numpy (tests/capped_ref.py, which imports nothing from the
product) and everything is compared with a brute-force sum over all pairs.

Shapes and system are those of tests/test_gpu_resolution.py: rc = 1.5, skin = 0.3, jittered lattice of spacing 0.75; (a) 9.0^3,
tiles; (b) (9.0, 10.8, 12.6); (c) 5.4^3, the per-cell k_pair_force_cap; (slab) (9.0, 9.0, 18.0) on two in-process ranks.  Three
types drawn uniformly; 0-0 LJ (cutoff 1.3) capped at 0.7, 1-1 table capped at 0.8 (linear, or the natural cubic spline where a
test says so), 0-1 LJ uncapped, 0-2 LJ (cutoff 1.4) uncapped -- or resolution-marked with a max_force in the mixed test --,
1-2 and 2-2 nothing.

Every force test first asserts on the CPU (guard) that each capped type pair has at least 10 pairs inside its cap radius, that
the capped reference differs from the uncapped one by more than 1e-2 of the largest force, and, for the fp32 comparisons, that
no pair that carries a term lies within 2e-6 of its CUTOFF (force and energy are continuous at the cap radius, so nothing of
the kind is needed there).

Tolerances are the project's: fp64 forces TOL[64] = 1e-10 of the largest force, fp32 pair forces TOL_MELT32 = 2e-5 with no
cutoff flip, energies and virials 1e-11 (fp64) / 1e-5 (fp32)."""
import numpy as np
import pytest

import capped_ref as C
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError, Engine
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_coulomb import REACT_CUT, reacting_pairs
from test_gpu_parity import TOL, TOL_MELT32
from test_gpu_resolution import GAP32, LJ00, LJ01, LJ02, system, two_ranks
from test_gpu_spline_tables import BOXES, RC, SKIN, table_11

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_MELT32}
TOL_E = {64: 1e-11, 32: 1e-5}
CAP00, CAP11 = 0.7, 0.8
CAPS = {(0, 0): CAP00, (1, 1): CAP11}
FMAX02 = 4.0                      # max_force of the marked 0-2 pairs in the mixed test


def pair_spec(spec, itype=1, caps=True, resolution=False):
    """the non-bonded matrix of the module docstring as W.apply takes it"""
    out = dict(spec, lj=[(0, 0) + LJ00, (0, 1) + LJ01, (0, 2) + LJ02], tables=[(1, 1) + table_11() + (RC, itype)])
    if caps:
        out["caps"] = [(a, b, c) for (a, b), c in CAPS.items()]
    if resolution:
        out["resolution"] = [(0, 2, FMAX02)]
    else:
        out.pop("lam", None)
    return out


def matrix(itype=1):
    return {(0, 0): S.lj(*LJ00), (0, 1): S.lj(*LJ01), (0, 2): S.lj(*LJ02), (1, 1): ("tab", S.Table(*table_11(), itype), RC)}


def guard(pos, box, types_, itype=1, lam=None, excluded=(), prec=32):
    """the reference of this configuration, after the assertions of the module docstring; lam: the mixed test (0-2 marked)"""
    marked = {(0, 2): FMAX02} if lam is not None else None
    ref = C.total(pos, box, types_, matrix(itype), CAPS, lam, marked, excluded)
    plain = C.total(pos, box, types_, matrix(itype), {}, lam, marked, excluded)
    part = np.abs(ref["F"] - plain["F"]).max() / np.abs(plain["F"]).max()
    p = ref["pairs"]
    ty = np.asarray(types_)
    inside = {k: int((p["inside"].astype(bool) & (ty[p["i"]] == k[0]) & (ty[p["j"]] == k[1])).sum()) for k in CAPS}
    gap = C.gap_to_cutoff(pos, box, types_, matrix(itype), lam, marked, excluded)
    print("pairs inside their cap radius %r; the caps move %.3e of the largest force; nearest pair with a term %.3e from its cutoff" % (inside, part, gap))
    assert min(inside.values()) >= 10
    assert part > 1e-2
    assert prec == 64 or gap > GAP32
    if lam is not None:             # the scaling shows as well
        unscaled = C.total(pos, box, types_, matrix(itype), CAPS, excluded=excluded)
        assert rel_err(ref["F"], unscaled["F"]) > 1e-2
    return ref


def compare(fg, ob, spec, x, prec, ref, itype=1):
    if prec == 64:
        err, flips = rel_err(fg, ref["F"]), 0
    else:
        s = dict(pair_spec(spec, itype, caps=False), pos=x)
        s["tables"] = [t[:7] for t in s["tables"]]
        err, flips = force_error_without_cutoff_flips(s, fg, ref["F"], TOL_F[32], max_flips=0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    print("prec %d: force rel err %.3e flips %d, virial_nb %.3e epot_lj %.3e epot_tab %.3e" %
          (prec, err, flips, rel(ob["virial_nb"], ref["w_nb"]), rel(ob["epot_lj"], ref["e_lj"]), rel(ob["epot_tab"], ref["e_tab"])))
    assert np.isfinite(fg).all()
    assert err < TOL_F[prec] and flips == 0
    assert ob["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[prec])
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec]) and ob["epot_tab"] == pytest.approx(ref["e_tab"], rel=TOL_E[prec])


def check(g, spec, prec, ref, itype=1):
    """forces, virial and the two energies at the engine's current positions"""
    g.run(0)
    compare(g.get_state("FORCE"), g.observe(), spec, g.get_state("POS"), prec, ref, itype)


# ---- 1: forces, energies and virial at step 0 --------------------------------------------------------------------------------

_REF = {}


def static_ref(shape, itype=1, mixed=False):
    """computed once, shared by both precisions"""
    key = (shape, itype, mixed)
    if key not in _REF:
        spec = system(shape)
        _REF[key] = (spec, guard(spec["pos"], spec["box"], spec["types"], itype, lam=spec["lam"] if mixed else None))
    return _REF[key]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape,itype", [("a", 1), ("a", 3), ("b", 1), ("c", 1), ("c", 3)])
def test_static_forces_energies_and_virial(make_gpu, shape, itype, prec):
    spec, ref = static_ref(shape, itype)
    g = make_gpu(prec)
    W.apply(pair_spec(spec, itype), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref, itype)


# ---- 2: two particles, known answers -----------------------------------------------------------------------------------------

def lj_f(r, eps, sig):
    s6 = (sig / r) ** 6
    return 24.0 * eps * (2.0 * s6 * s6 - s6) / r


def two_body_system(shape):
    """eight far-apart pairs in one context: for the LJ (type 0) and the table (type 1) pair, r = c/2, c, c (1 + 1e-3) and 0;
    particle 2k sits on a site of a lattice of spacing about 3 (box a) or 2.7 (box c), its partner at r along a skew direction"""
    box = np.array(BOXES[shape])
    u = np.array([1.0, 2.0, -2.0]) / 3.0
    site = np.stack(np.meshgrid(*[np.arange(int(np.floor(b / 2.7 + 1e-9))) * (b / int(np.floor(b / 2.7 + 1e-9))) for b in box], indexing="ij"), -1).reshape(-1, 3) + 0.4
    pos, ty, want = [], [], []
    for t, c in ((0, CAP00), (1, CAP11)):
        for r in (0.5 * c, c, c * (1.0 + 1e-3), 0.0):
            k = len(pos) // 2
            pos += [site[k], site[k] - r * u]
            ty += [t, t]
            want.append((t, c, r))
    n = len(pos)
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=1e-3, ids=np.arange(1, n + 1), types=np.array(ty, np.int32), pos=np.array(pos),
                vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32),
                kT=0.0, gamma=0.0, seed=1, rebuild_criterion=1)
    return W.snap_to_grid(spec), want, u


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_two_particle_known_answers(make_gpu, shape, prec):
    spec, want, u = two_body_system(shape)
    assert len(spec["pos"]) == 16
    x, box = spec["pos"], np.asarray(spec["box"])
    ref = C.total(x, box, spec["types"], matrix(), CAPS)
    assert len(ref["pairs"]["i"]) == 8                               # the eight pairs and nothing else
    tab = S.Table(*table_11(), 1)
    g = make_gpu(prec)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.run(0)
    f, ob = g.get_state("FORCE"), g.observe()
    assert np.isfinite(f).all()
    tol = 1e-10 if prec == 64 else 2e-5
    for k, (t, c, r) in enumerate(want):
        fc = lj_f(c, *LJ00[:2]) if t == 0 else float(tab(c)[1])
        fi, fj = f[2 * k], f[2 * k + 1]
        print("type %d r/c %.4f: |F| %.9e  f(c) %.9e" % (t, r / c, np.linalg.norm(fi), fc))
        if r == 0.0:
            assert np.array_equal(fi, np.zeros(3)) and np.array_equal(fj, np.zeros(3))        # exactly zero, and finite
            continue
        assert np.abs(fi + fj).max() <= tol * abs(fc)
        assert np.abs(fi - ref["F"][2 * k]).max() <= tol * abs(fc)
        if r < c:                                                     # magnitude f(c), direction r_ij, whatever r is
            assert np.abs(fi - fc * u).max() <= (1e-7 if prec == 64 else 2e-5) * abs(fc)      # (fp64: the snapped r_ij is 1e-9 off u)
        else:                                                         # just above (or, snapped, on) the cap radius: the potential's own force, continuous with f(c)
            assert abs(np.linalg.norm(fi) - abs(fc)) < 0.05 * abs(fc)
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec]) and ob["epot_tab"] == pytest.approx(ref["e_tab"], rel=TOL_E[prec])
    assert ob["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[prec])
    # U(c) at r = 0 and r = c/2: three pairs of either kind sit on the plateau or next to it
    assert ref["pairs"]["inside"].sum() >= 4


# ---- 3, 4: motion and rebuilds -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_forces_after_motion_and_rebuilds(make_gpu, shape, prec):
    """200 NVE steps (energy conservation is not expected: inside a cap the energy does not integrate the force), then the
    forces at the engine's final positions against the reference"""
    spec = system(shape)
    g = make_gpu(prec)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.run(200)
    x = g.get_state("POS")
    assert g.timers()["rebuilds"] >= 2 and np.abs(x - spec["pos"]).max() > 0.1
    check(g, spec, prec, guard(x, spec["box"], spec["types"], prec=prec))


def test_forces_after_motion_on_two_slabs(make_gpu):
    spec = system("slab")

    def body(g):
        W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
        g.run(200)
        g.run(0)
        return dict(x=g.get_state("POS"), f=g.get_state("FORCE"), ob=g.observe(), rebuilds=g.timers()["rebuilds"])
    out = two_ranks(make_gpu, spec, body)
    assert np.array_equal(out[0]["x"], out[1]["x"]) and np.abs(out[0]["x"] - spec["pos"]).max() > 0.1
    ref = guard(out[0]["x"], spec["box"], spec["types"], prec=64)
    for o in out:
        assert o["rebuilds"] >= 2
        compare(o["f"], o["ob"], spec, o["x"], 64, ref)


# ---- 5: caps and resolution in one context -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_caps_and_resolution_in_one_context(make_gpu, shape, prec):
    """0-2 resolution-marked with max_force, 0-0 and 1-1 capped, lambda drawn as in tests/test_gpu_resolution.py"""
    spec, ref = static_ref(shape, mixed=True)
    assert ((ref["pairs"]["fmax"] > 0) & (np.abs(ref["pairs"]["w"] * ref["pairs"]["ff"]) * np.sqrt(ref["pairs"]["r2"]) > FMAX02)).any()      # max_force acts
    g = make_gpu(prec)
    W.apply(pair_spec(spec, resolution=True), g, thermostat=False, reactions=False)
    check(g, spec, prec, ref)
    assert np.array_equal(g.get_state("LAMBDA"), spec["lam"])


# ---- 6: type changes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_type_changes_move_pairs_between_capped_and_uncapped(make_gpu, shape, prec):
    """A virtual reaction 0 + 2 -> 0 + 0 at an infinite rate, one step of 1e-5 from rest (the particles move by ~1e-9): type 2
    (no cap anywhere) becomes type 0 (0-0 capped).  Then chem_modify_particle(TYPE) on a handful: 0 -> 1, 1 -> 0, 2 -> 1.
    After each the forces are the reference's on the new types."""
    spec = system(shape, dt=1e-5, vel=False)
    pairs = reacting_pairs(spec)
    print("reacting pairs:", len(pairs))
    assert 3 <= len(pairs) <= 60
    g = make_gpu(prec)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.reaction_init(1, nearest=True, seed=4)
    g.reaction_add(0, 2, 1, 1, 0, 1, 0, 1, rate=1e30, cutoff=REACT_CUT, is_virtual=True, intramolecular=True, intraresidual=True,
                   new_type_1=0, new_type_2=0, new_mass_1=1.0, new_mass_2=1.0)
    g.reactions_enable(True)
    g.run(1)
    ev = g.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev) == sorted(pairs)
    ty = spec["types"].copy()
    for a, b in pairs:
        ty[b] = 0
    assert np.array_equal(g.get_state("TYPE"), ty)
    g.reactions_enable(False)
    x = g.get_state("POS")
    assert np.abs(x - spec["pos"]).max() < 1e-6
    ref = guard(x, spec["box"], ty, prec=prec)
    assert rel_err(ref["F"], C.total(x, spec["box"], spec["types"], matrix(), CAPS)["F"]) > 1e-3      # the old types are far off
    check(g, dict(spec, types=ty), prec, ref)
    for t_old, t_new in ((0, 1), (1, 0), (2, 1)):
        for i in np.nonzero(spec["types"] == t_old)[0][[2, 9, 21]]:
            if ty[i] == t_old:
                g.modify_particle(int(i) + 1, "TYPE", t_new)
                ty[i] = t_new
    assert np.array_equal(g.get_state("TYPE"), ty)
    ref2 = guard(x, spec["box"], ty, prec=prec)
    assert rel_err(ref2["F"], ref["F"]) > 1e-3
    check(g, dict(spec, types=ty), prec, ref2)


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(make_gpu):
    spec = system("a")
    g = make_gpu(64)
    W.apply(pair_spec(spec, caps=False), g, thermostat=False, reactions=False)
    g.run(0)
    before = g.get_state("FORCE")

    def refused(code, match, call):
        with pytest.raises(ChemError, match=match) as ei:
            call()
        assert ei.value.code == code
    refused(_capi.EINVAL, r"type pair \(1,2\) carries no", lambda: g.nb_cap(1, 2, 0.5))
    g.nb_cap(1, 2, 0.0)                                             # removing what is not there is a no-op
    refused(_capi.EINVAL, "type out of range", lambda: g.nb_cap(0, 16, 0.5))
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(_capi.EINVAL, "finite", lambda: g.nb_cap(0, 0, bad))
    for bad in (LJ00[2], LJ00[2] + 0.1):                            # caprad >= rc of that potential (0-0: 1.3)
        refused(_capi.EINVAL, r"\(0,0\) must lie inside its cutoff", lambda: g.nb_cap(0, 0, bad))
    refused(_capi.EINVAL, r"\(1,1\) must lie inside its cutoff", lambda: g.nb_cap(1, 1, RC))
    g.run(0)
    assert np.array_equal(g.get_state("FORCE"), before)            # a refused call sets nothing
    # capped and resolution-marked on one type pair, in either order
    g.nb_resolution(0, 2, True, 0.0)
    refused(_capi.EINVAL, r"\(0,2\) is resolution-marked", lambda: g.nb_cap(0, 2, 0.7))
    refused(_capi.EINVAL, r"\(2,0\) is resolution-marked", lambda: g.nb_cap(2, 0, 0.7))
    g.nb_resolution(0, 2, False, 0.0)
    g.nb_cap(0, 2, 0.7)
    refused(_capi.EINVAL, r"\(0,2\) is capped", lambda: g.nb_resolution(0, 2, True, 0.0))
    refused(_capi.EINVAL, r"\(2,0\) is capped", lambda: g.nb_resolution(2, 0, True, 5.0))
    g.nb_cap(0, 2, 0.0)
    # the build limits of the mode, as for the Coulomb term
    g.nb_cap(0, 0, CAP00)
    g.run(0)
    for opt, bad, good in (("tpp", 2, 0), ("pair_block", 256, 512)):
        g.set_option(opt, bad)
        refused(_capi.EINVAL, opt, lambda: g.run(0))
        g.set_option(opt, good)
        g.run(0)
    # a re-sent potential whose cutoff no longer exceeds the radius: refused at the next run, naming the pair
    g.nb_lj(0, 0, LJ00[0], LJ00[1], 0.65)
    refused(_capi.EINVAL, r"capped type pair \(0,0\)", lambda: g.run(0))
    g.nb_lj(0, 0, *LJ00)
    g.run(0)
    # the Coulomb combination: refused at the next evaluation, naming the capped pair
    g.nb_coulomb(1, 2, 1.5, 1.2)
    refused(_capi.ENOTIMPL, r"capped type pair \(0,0\) next to a registered Coulomb pair", lambda: g.run(0))
    g.nb_coulomb(1, 2, 0.0, 1.2)
    g.run(0)


# ---- 8: removal ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_caps_set_and_removed_leave_nothing_behind(make_gpu, shape, prec):
    """caps set and removed against a context that never had them: forces, energies and a short trajectory bit for bit;
    and a potential that is sent again keeps its cap"""
    spec = system(shape)
    plain, g = make_gpu(prec), make_gpu(prec)
    W.apply(pair_spec(spec, caps=False), plain, thermostat=False, reactions=False)
    W.apply(pair_spec(spec), g, thermostat=False, reactions=False)
    g.run(0); plain.run(0)
    capped = g.get_state("FORCE")
    assert rel_err(capped, plain.get_state("FORCE")) > 1e-2
    # the potentials sent again: the caps stay
    g.nb_lj(0, 0, *LJ00)
    g.nb_table(1, 1, *table_11(), RC)
    g.run(0)
    assert np.array_equal(g.get_state("FORCE"), capped)
    for (a, b) in CAPS:
        g.nb_cap(a, b, 0.0)
    plain.set_option("tiles", 1)                                    # (both contexts build their lists again)
    g.run(0); plain.run(0)
    assert np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    og, op = g.observe(), plain.observe()
    assert og["epot_lj"] == op["epot_lj"] and og["epot_tab"] == op["epot_tab"] and og["virial_nb"] == op["virial_nb"]
    g.run(20); plain.run(20)
    assert np.array_equal(g.get_state("POS"), plain.get_state("POS")) and np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))


# ---- 9: the shim ---------------------------------------------------------------------------------------------------------------

def test_the_shim_sends_the_caps_and_reports_the_shared_energies(tmp_path):
    """VerletListTabulatedCapped.computeEnergy() = the reference's tabulated energy; a VerletListLennardJonesCapped next to a
    plain VerletListLennardJones reports the one LJ accumulator both feed"""
    from chemlab_amd import espp
    spec, ref = static_ref("a")
    r0, dr, e, f = table_11()
    np.savetxt(tmp_path / "table_1_1.pot", np.stack([r0 + dr * np.arange(len(e)), e, f], 1), fmt="%.17g")
    prev = espp._factory[0]
    espp.set_engine_factory(lambda: Engine(device=0, precision=64))
    try:
        sysm = espp.System()
    finally:
        espp.set_engine_factory(prev)
    try:
        sysm.rng = espp.esutil.RNG(1)
        sysm.skin = SKIN
        box = tuple(spec["box"])
        sysm.bc = espp.bc.OrthorhombicBC(sysm.rng, box)
        sysm.storage = espp.storage.DomainDecomposition(sysm, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), RC, SKIN))
        integrator = espp.integrator.VelocityVerlet(sysm)
        integrator.dt = 0.002
        plist = [[i + 1, int(spec["types"][i]), espp.Real3D(*spec["pos"][i]), espp.Real3D(0.0, 0.0, 0.0), 1.0, 0] for i in range(spec["n"])]
        sysm.storage.addParticles(plist, "id", "type", "pos", "v", "mass", "state")
        sysm.storage.decompose()
        vl = espp.VerletList(sysm, cutoff=RC, exclusionlist=espp.DynamicExcludeList(integrator, []))
        lj = espp.interaction.VerletListLennardJones(vl)
        lj.setPotential(type1=0, type2=1, potential=espp.interaction.LennardJones(epsilon=LJ01[0], sigma=LJ01[1], cutoff=LJ01[2]))
        lj.setPotential(type1=0, type2=2, potential=espp.interaction.LennardJones(epsilon=LJ02[0], sigma=LJ02[1], cutoff=LJ02[2]))
        sysm.addInteraction(lj, "lj")
        ljc = espp.interaction.VerletListLennardJonesCapped(vl)
        ljc.setPotential(type1=0, type2=0, potential=espp.interaction.LennardJonesCapped(epsilon=LJ00[0], sigma=LJ00[1], cutoff=LJ00[2], caprad=CAP00))
        sysm.addInteraction(ljc, "lj_cap")
        tc = espp.interaction.VerletListTabulatedCapped(vl)
        tc.setPotential(type1=1, type2=1, potential=espp.interaction.TabulatedCapped(itype=1, filename=str(tmp_path / "table_1_1.pot"), cutoff=RC, caprad=CAP11))
        sysm.addInteraction(tc, "lj-tab_cap")
        assert tc.getPotential(1, 1).caprad == CAP11
        integrator.run(0)
        assert tc.computeEnergy() == pytest.approx(ref["e_tab"], rel=1e-11)
        assert ljc.computeEnergy() == pytest.approx(ref["e_lj"], rel=1e-11)
        assert espp.analysis.PotentialEnergy(sysm, lj).compute() == ljc.computeEnergy()
        assert espp.analysis.PotentialEnergy(sysm, tc).compute() == tc.computeEnergy()
        assert rel_err(sysm.engine.get_state("FORCE"), ref["F"]) < TOL[64]
    finally:
        sysm.engine.close()
