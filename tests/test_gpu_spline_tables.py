"""Spline kinds of the tabulated potentials on the HIP path: Tabulated itype 2 (Akima) and 3 (natural cubic spline) as pair
tables (chem_nb_table_interp: k_pair_tiles MODE 3, k_pair_force CUBIC) and as bonded tables (chem_table_create_interp:
btab_lookup in k_bonded_work / k_bonded).  Rule set: include/chem_mi355.h.

The CPU oracle interpolates linearly only, so the rule set is restated in numpy (tests/spline_ref.py, which imports nothing
from the product) and forces and energies are compared with a brute-force sum over all pairs plus bonds, angles and
dihedrals evaluated from the splines.  Every test first asserts that the linear and the spline reference of its own
configuration differ by more than 1e-3 of the largest force: none of them can pass on a linear evaluation.

Shapes: pair tables use rc = 1.5, skin = 0.3, so one cell is 1.8 and five cells per axis the smallest grid the LDS tiles
take.  (a) box 9.0^3, 12^3 particles on a jittered lattice (spacing 0.75, jitter 0.1) whose first layer lies 0.1 behind the
low faces: pairs cross every periodic boundary.  (b) box (9.0, 10.8, 12.6): 5 x 6 x 7 cells.  (c) box 5.4^3, 7^3 particles:
three cells per axis, no tiles, k_pair_force.  The table is synthetic_table(nrow=34, dr=0.05): on that grid the kinds are
percent apart.

Tolerances are the project's: fp64 forces 1e-10 of the largest force, energies 1e-11, trajectory 1e-9 (test_gpu_parity TOL,
test_gpu_dissociation); fp32 pair forces TOL_MELT32 = 2e-5 with no cutoff flip allowed (the tables' force is zero at rc and
the LJ pairs of these configurations do not sit on their cutoff), fp32 bonded forces TOL_STIFF32 = 5e-5, fp32 energies 1e-5.
Measured on an MI355X when the path was built: fp32 pair forces 1.4e-6 .. 7.9e-6 of the largest force with no flip (the
linear kind on the same configuration: 4.5e-6), fp32 table energies 7e-8, fp32 bonded forces up to 1.0e-6; fp64 1.5e-14."""
import numpy as np
import pytest

import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError, Engine
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_parity import TOL, TOL_MELT32, TOL_STIFF32, _HUB, _run_ranks

pytestmark = pytest.mark.gpu

RC, SKIN, DT = 1.5, 0.3, 0.002
TOL_F = {64: TOL[64], 32: TOL_MELT32}
TOL_FB = {64: TOL[64], 32: TOL_STIFF32}
TOL_E = {64: 1e-11, 32: 1e-5}
LJ01 = (1.0, 0.5, RC)                     # type pair 0-1: eps, sigma, cutoff
BOXES = {"a": (9.0, 9.0, 9.0), "b": (9.0, 10.8, 12.6), "c": (5.4, 5.4, 5.4), "slab": (9.0, 9.0, 18.0)}


# ---- tables and systems --------------------------------------------------------------------------------------------------

def table_00():
    return W.synthetic_table(nrow=34, dr=0.05, rc=RC)


def table_11():
    """a second table with another r0: rows at r = 0.1 + 0.05 k, k < 30; same family as synthetic_table, other parameters"""
    r0, dr, eps, sigma = 0.1, 0.05, 1.5, 0.7
    r = r0 + dr * np.arange(30)
    x = r / sigma
    e = eps * (np.exp(-4.0 * (x - 1.0)) - 2.0 * np.exp(-2.0 * (x - 1.0)))
    f = eps * (2.0 / sigma) * (2.0 * np.exp(-4.0 * (x - 1.0)) - 2.0 * np.exp(-2.0 * (x - 1.0)))
    sw = np.where(r < RC, (1.0 - (r / RC) ** 2) ** 2, 0.0)
    dsw = np.where(r < RC, -4.0 * r / RC ** 2 * (1.0 - (r / RC) ** 2), 0.0)
    return r0, dr, e * sw, f * sw - e * dsw


def linear_tables():
    """columns y = a + b r on the grids of table_00 and table_11"""
    r0a, dra, _, _ = table_00()
    r0b, drb, _, _ = table_11()
    ra, rb = r0a + dra * np.arange(34), r0b + drb * np.arange(30)
    return (r0a, dra, 3.0 - 1.5 * ra, 4.0 - 2.0 * ra), (r0b, drb, 1.0 - 0.5 * rb, 2.5 - 1.25 * rb)


def melt(shape, seed=3, kT=1.0):
    box = np.array(BOXES[shape])
    rng = np.random.default_rng(seed)
    k = np.floor(box / 0.75 + 1e-9).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3)
    pos = g * 0.75 - 0.1 + rng.uniform(-0.1, 0.1, g.shape)
    n = len(pos)
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, n + 1), types=rng.integers(0, 2, n).astype(np.int32),
                pos=pos, vel=rng.normal(0.0, np.sqrt(kT), (n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), kT=kT, gamma=0.0, seed=1, rebuild_criterion=1)
    return W.snap_to_grid(spec)


def matrix(t00, t11, itype):
    """reference matrix: 0-0 and 1-1 under tables of kind `itype` (None: no entry), 0-1 under LJ"""
    m = {(0, 1): S.lj(*LJ01)}
    if t00 is not None:
        m[(0, 0)] = ("tab", S.Table(*t00, itype), RC)
    if t11 is not None:
        m[(1, 1)] = ("tab", S.Table(*t11, itype), RC)
    return m


def send_pairs(g, t00, t11, itype):
    g.nb_lj(0, 1, *LJ01, True)
    g.nb_table(0, 0, *t00, RC, itype=itype)
    g.nb_table(1, 1, *t11, RC, itype=itype)


def setup(g, spec):
    W.apply(spec, g, thermostat=False, reactions=False)


def guard(pos, box, types, mat_spline, mat_linear, **kw):
    """the reference of this configuration; asserts that the linear kind is far from it"""
    F, elj, etab = S.pair_sums(pos, box, types, mat_spline, **kw)
    Fl, _, _ = S.pair_sums(pos, box, types, mat_linear, **kw)
    assert rel_err(Fl, F) > 1e-3
    return F, elj, etab


def check_pairs(g, spec, prec, F, elj, etab, tables=()):
    g.run(0)
    fg, ob = g.get_state("FORCE"), g.observe()
    if prec == 64:
        err, flips = rel_err(fg, F), 0
    else:
        s = dict(spec, pos=g.get_state("POS"), lj=[(0, 1) + LJ01], tables=list(tables))
        err, flips = force_error_without_cutoff_flips(s, fg, F, TOL_F[32], max_flips=0)
    print("prec %d: force rel err %.3e, flips %d, epot_tab %.3e, epot_lj %.3e" %
          (prec, err, flips, abs(ob["epot_tab"] - etab) / max(abs(etab), 1e-300), abs(ob["epot_lj"] - elj) / max(abs(elj), 1e-300)))
    assert err < TOL_F[prec] and flips == 0
    assert ob["epot_tab"] == pytest.approx(etab, rel=TOL_E[prec])
    assert ob["epot_lj"] == pytest.approx(elj, rel=TOL_E[prec])


# ---- 6: static forces and energies ----------------------------------------------------------------------------------------

_REF = {}


def static_ref(shape, itype):
    """numpy reference of a static configuration: computed once, shared by both precisions"""
    if (shape, itype) not in _REF:
        spec = melt(shape)
        _REF[(shape, itype)] = (spec, guard(spec["pos"], spec["box"], spec["types"], matrix(table_00(), table_11(), itype),
                                            matrix(table_00(), table_11(), 1)))
    return _REF[(shape, itype)]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("itype", [2, 3])
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_static_forces_and_energies(make_gpu, shape, itype, prec):
    spec, (F, elj, etab) = static_ref(shape, itype)
    g = make_gpu(prec)
    setup(g, spec)
    send_pairs(g, table_00(), table_11(), itype)
    check_pairs(g, spec, prec, F, elj, etab, tables=[(0, 0) + table_00() + (RC,), (1, 1) + table_11() + (RC,)])


def test_refused_arguments(make_gpu):
    g = make_gpu(64)
    r0, dr, e, f = table_00()
    for itype in (2, 3):
        with pytest.raises(ChemError) as ei:
            g.nb_table(0, 0, r0, dr, e[:3], f[:3], RC, itype=itype)
        assert ei.value.code == _capi.EINVAL
        with pytest.raises(ChemError) as ei:
            g.table_create(r0, dr, e[:3], f[:3], itype=itype)
        assert ei.value.code == _capi.EINVAL
    for itype in (0, 4):
        with pytest.raises(ChemError) as ei:
            g.nb_table(0, 0, r0, dr, e, f, RC, itype=itype)
        assert ei.value.code == _capi.EINVAL
        with pytest.raises(ChemError) as ei:
            g.table_create(r0, dr, e, f, itype=itype)
        assert ei.value.code == _capi.EINVAL
    assert g.table_create(r0, dr, e[:4], f[:4], itype=2) == 0 and g.table_create(r0, dr, e[:2], f[:2]) == 1


# ---- 7: after motion and list rebuilds ------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("itype", [2, 3])
def test_after_motion_and_rebuilds(make_gpu, itype, prec):
    spec = melt("a")
    g = make_gpu(prec)
    setup(g, spec)
    send_pairs(g, table_00(), table_11(), itype)
    g.run(60)
    print("rebuilds", g.timers()["rebuilds"])
    assert g.timers()["rebuilds"] >= 2
    x = g.get_state("POS")
    F, elj, etab = guard(x, spec["box"], spec["types"], matrix(table_00(), table_11(), itype), matrix(table_00(), table_11(), 1))
    check_pairs(g, spec, prec, F, elj, etab, tables=[(0, 0) + table_00() + (RC,), (1, 1) + table_11() + (RC,)])


def test_after_motion_on_two_slabs(make_gpu):
    """the in-process decomposed path (two ranks, one thread each, box 9 x 9 x 18): the same kernels behind the halo exchange"""
    spec, itype, P = melt("slab"), 2, 2
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        setup(g, spec)
        send_pairs(g, table_00(), table_11(), itype)
        g.run(60)
        reb = g.timers()["rebuilds"]
        g.run(0)
        return dict(x=g.get_state("POS"), f=g.get_state("FORCE"), ob=g.observe(), reb=reb)
    out = _run_ranks(P, rank)
    assert np.array_equal(out[0]["x"], out[1]["x"])
    F, elj, etab = guard(out[0]["x"], spec["box"], spec["types"], matrix(table_00(), table_11(), itype), matrix(table_00(), table_11(), 1))
    for r in range(P):
        assert out[r]["reb"] >= 2
        assert rel_err(out[r]["f"], F) < TOL_F[64]
        assert out[r]["ob"]["epot_tab"] == pytest.approx(etab, rel=TOL_E[64])
        assert out[r]["ob"]["epot_lj"] == pytest.approx(elj, rel=TOL_E[64])


# ---- 8: the kind of a type pair swapped between runs --------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
def test_kind_swap_between_runs(make_gpu, prec):
    """0-0: (Akima, no step) -> linear -> Akima -> cubic spline -> LJ with run(5) in between; 0-1 is LJ and 1-1 a linear
    table throughout.  The linear leg is compared bit for bit with a context that never saw a spline table."""
    spec = melt("a")
    t00, t11 = table_00(), table_11()
    lj00 = (0.8, 0.55, RC)

    def base(g):
        setup(g, spec)
        g.nb_lj(0, 1, *LJ01, True)
        g.nb_table(1, 1, *t11, RC)
    g, plain = make_gpu(prec), make_gpu(prec)
    base(g); base(plain)
    g.nb_table(0, 0, *t00, RC, itype=2)
    g.run(0)                                                 # the CUBIC instantiations ran in this context
    f_akima0 = g.get_state("FORCE")
    plain.nb_table(0, 0, *t00, RC)
    plain.run(0)                                             # (the same history of list builds, linear tables only)
    for e in (g, plain):
        e.nb_table(0, 0, *t00, RC)
        e.run(5)
    assert np.array_equal(g.get_state("POS"), plain.get_state("POS")) and np.array_equal(g.get_state("VEL"), plain.get_state("VEL"))
    g.run(0); plain.run(0)
    assert np.array_equal(g.get_state("FORCE"), plain.get_state("FORCE"))
    assert g.observe()["epot_tab"] == plain.observe()["epot_tab"]
    assert rel_err(f_akima0, S.pair_sums(spec["pos"], spec["box"], spec["types"], {(0, 0): ("tab", S.Table(*t00, 2), RC), (0, 1): S.lj(*LJ01), (1, 1): ("tab", S.Table(*t11, 1), RC)})[0]) < TOL_F[prec]

    def ref(kind):
        m = {(0, 1): S.lj(*LJ01), (1, 1): ("tab", S.Table(*t11, 1), RC)}
        m[(0, 0)] = S.lj(*lj00) if kind == "lj" else ("tab", S.Table(*t00, kind), RC)
        return S.pair_sums(g.get_state("POS"), spec["box"], spec["types"], m)
    legs = [1, 2, 3, "lj"]
    for k, kind in enumerate(legs):
        if k:                                                 # (the linear leg has run above)
            if kind == "lj":
                g.nb_lj(0, 0, *lj00, True)
            else:
                g.nb_table(0, 0, *t00, RC, itype=kind)
            g.run(5)
        F, elj, etab = ref(kind)
        others = [ref(o)[0] for o in legs if o != kind]
        assert min(rel_err(Fo, F) for Fo in others) > 1e-3    # every other kind is far from the one in force
        tabs = [(1, 1) + t11 + (RC,)] + ([] if kind == "lj" else [(0, 0) + t00 + (RC,)])
        s = dict(spec, lj=[(0, 1) + LJ01] + ([(0, 0) + lj00] if kind == "lj" else []))
        g.run(0)
        fg, ob = g.get_state("FORCE"), g.observe()
        if prec == 64:
            err, flips = rel_err(fg, F), 0
        else:
            err, flips = force_error_without_cutoff_flips(dict(s, pos=g.get_state("POS"), tables=tabs), fg, F, TOL_F[32], max_flips=0)
        print("leg %s prec %d: force rel err %.3e flips %d" % (kind, prec, err, flips))
        assert err < TOL_F[prec] and flips == 0
        assert ob["epot_tab"] == pytest.approx(etab, rel=TOL_E[prec]) and ob["epot_lj"] == pytest.approx(elj, rel=TOL_E[prec])


# ---- 9: bonded tables --------------------------------------------------------------------------------------------------------

BOND_LEN = (0.55, 0.62, 0.9, 1.1, 1.36, 1.45)       # the table spans [0.6, 1.38]: both clamps run


def bond_table():
    r = 0.6 + 0.06 * np.arange(14)                   # (a coarse grid under a wavy column: the kinds are percent apart)
    return 0.6, 0.06, 30.0 * (r - 0.95) ** 2 + 2.0 * np.sin(20.0 * r), -60.0 * (r - 0.95) - 40.0 * np.cos(20.0 * r)


def angle_table():
    th = np.linspace(0.0, np.pi, 40)
    return 0.0, np.pi / 39.0, 5.0 * (th - 2.0) ** 2 + np.cos(5.0 * th), -10.0 * (th - 2.0) + 5.0 * np.sin(5.0 * th)


def dihedral_table():
    ph = np.linspace(-np.pi, np.pi, 73)
    return -np.pi, 2.0 * np.pi / 72.0, 2.0 * (1.0 + np.cos(3.0 * ph)) + 0.7 * np.sin(5.0 * ph) + 0.3 * ph, 6.0 * np.sin(3.0 * ph) - 3.5 * np.cos(5.0 * ph) - 0.3


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def molecules(box, nside, ntri, nchain, seed=11, dmin=0.4):
    """ntri bent trimers a(0)-b(1)-c(0) and nchain four-bead chains (type 1) on a jittered lattice whose first layer lies
    0.15 behind the low faces; bond lengths from BOND_LEN in turn, chain torsions spread over [-3.13, 3.13].  Orientations
    are drawn again until no particle of another molecule is closer than dmin (the LJ pairs stay off their wall)."""
    rng = np.random.default_rng(seed)
    g = np.arange(nside)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * (box / nside) - 0.15 + rng.uniform(-0.05, 0.05, (nside ** 3, 3))
    sites = sites[rng.permutation(len(sites))][:ntri + nchain]
    pos, types, b_ab, b_cb, angles, b_chain, quads = [], [], [], [], [], [], []

    def place(draw):
        for _ in range(1000):
            p = draw()
            if pos:
                d = np.array(pos)[None, :, :] - p[:, None, :]
                d -= box * np.rint(d / box)
                if (d * d).sum(2).min() < dmin * dmin:
                    continue
            return p
        raise AssertionError("no room for a molecule")

    def trimer(k):
        d1 = rng.choice([-1.0, 1.0], 3) / np.sqrt(3.0)
        d2 = d1.copy(); d2[rng.integers(3)] *= -1.0
        d2 = d2 + rng.uniform(-0.3, 0.3, 3); d2 /= np.linalg.norm(d2)
        return np.array([sites[k] - BOND_LEN[k % 6] * d1, sites[k], sites[k] + BOND_LEN[(k // 6) % 6] * d2])
    for k in range(ntri):
        i0 = len(pos) + 1
        pos += list(place(lambda: trimer(k))); types += [0, 1, 0]
        b_ab.append((i0, i0 + 1) if k % 3 else (i0 + 1, i0)); b_cb.append((i0 + 2, i0 + 1)); angles.append((i0, i0 + 1, i0 + 2))
    l, al = 0.5, 1.9
    for k, phi in enumerate(np.linspace(-3.13, 3.13, nchain)):
        p = np.array([[l * np.sin(al), 0.0, -l * np.cos(al)], [0.0, 0.0, 0.0], [0.0, 0.0, l],
                      [l * np.sin(al) * np.cos(phi), l * np.sin(al) * np.sin(phi), l + l * np.cos(al - np.pi / 2.0)]])
        i0 = len(pos) + 1
        pos += list(place(lambda: p @ rotation(rng).T + sites[ntri + k])); types += [1, 1, 1, 1]
        b_chain += [(i0, i0 + 1), (i0 + 1, i0 + 2), (i0 + 2, i0 + 3)]; quads.append((i0, i0 + 1, i0 + 2, i0 + 3))
    return np.array(pos), np.array(types, np.int32), [np.array(x, np.int64) for x in (b_ab, b_cb, b_chain, angles, quads)]


K_CHAIN, R_CHAIN = 40.0, 0.5
LJB = (1.0, 0.3)


def bonded_pair_part(pos, box, types, lists, rc_lj):
    excl = np.concatenate([np.asarray(x) - 1 for x in lists[:3]])
    F, elj, _ = S.pair_sums(pos, np.array([box] * 3), types, {(a, b): S.lj(*LJB, rc_lj) for a in range(2) for b in range(a, 2)}, excluded=[tuple(e) for e in excl])
    return F, elj


def bonded_terms(pos, box, lists, kinds):
    """(forces, energy) of the lists [ab, cb, chain, angle, dihedral] with tables of kinds (bond ab, bond cb, angle, dihedral)"""
    L = np.array([box] * 3)
    b_ab, b_cb, b_chain, angles, quads = [np.asarray(x) - 1 for x in lists]
    return [S.bond_terms(pos, L, b_ab, S.Table(*bond_table(), kinds[0])), S.bond_terms(pos, L, b_cb, S.Table(*bond_table(), kinds[1])),
            S.bond_terms(pos, L, b_chain, lambda r: (K_CHAIN * (r - R_CHAIN) ** 2, -2.0 * K_CHAIN * (r - R_CHAIN))),
            S.angle_terms(pos, L, angles, S.Table(*angle_table(), kinds[2])), S.dihedral_terms(pos, L, quads, S.Table(*dihedral_table(), kinds[3]))]


def bonded_spec(box, nside, ntri, nchain, rc_lj, kT=1.0):
    pos, types, lists = molecules(box, nside, ntri, nchain)
    n = len(pos)
    rng = np.random.default_rng(2)
    spec = dict(n=n, box=[box] * 3, rc=rc_lj, skin=SKIN, dt=1e-3, ids=np.arange(1, n + 1), types=types, pos=pos,
                vel=rng.normal(0.0, np.sqrt(kT), (n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32),
                lj=[(a, b) + LJB + (rc_lj,) for a in range(2) for b in range(a, 2)], kT=kT, gamma=0.0, seed=1, rebuild_criterion=1,
                exclusions=np.concatenate(lists[:3]))
    return W.snap_to_grid(spec), lists


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("ang_dih", [(3, 2), (2, 3)])
@pytest.mark.parametrize("system", ["tiles", "three_cells"])
def test_bonded_spline_tables(make_gpu, system, ang_dih, prec):
    """tiles: box 14 (five cells at rc 2.5 + skin 0.3), 500 trimers + 100 chains; three_cells: box 8.4, 100 + 25 -- the path
    without LDS tiles (k_bonded instead of k_bonded_work)."""
    box, nside, ntri, nchain = (14.0, 9, 500, 100) if system == "tiles" else (8.4, 5, 100, 25)
    rc_lj = 2.5
    spec, lists = bonded_spec(box, nside, ntri, nchain, rc_lj)
    kinds = (2, 3) + ang_dih
    g = make_gpu(prec)
    setup(g, spec)
    h2, h3 = g.table_create(*bond_table(), itype=2), g.table_create(*bond_table(), itype=3)       # two kinds in one rows array
    ha, hd = g.table_create(*angle_table(), itype=kinds[2]), g.table_create(*dihedral_table(), itype=kinds[3])
    hl = []
    for arity, kind, par, ids in ((2, "TABULATED", [h2], lists[0]), (2, "TABULATED", [h3], lists[1]), (2, "HARMONIC", [K_CHAIN, R_CHAIN], lists[2]),
                                  (3, "ANG_TABULATED", [ha], lists[3]), (4, "DIH_TABULATED", [hd], lists[4])):
        h = g.list_create(arity, kind, False)
        g.list_set_params(h, par); g.list_add(h, ids)
        hl.append(h)
    L = np.array([box] * 3)
    phi, _ = S.dihedral_angle(spec["pos"], L, lists[4] - 1)
    tk = np.floor((phi + np.pi) / (2.0 * np.pi / 72.0))
    assert tk.min() == 0 and tk.max() == 71                                                        # both end intervals of the dihedral table
    for stage in (0, 1):
        if stage:
            g.run(20)
        x = g.get_state("POS")
        Fp, elj = bonded_pair_part(x, box, spec["types"], lists, rc_lj)
        terms, lin = bonded_terms(x, box, lists, kinds), bonded_terms(x, box, lists, (1, 1, 1, 1))
        F, el = Fp + sum(t[0] for t in terms), [t[1] for t in terms]
        for k in (0, 1, 3, 4):                                    # every tabulated list on its own is far from its linear evaluation
            assert np.abs(lin[k][0] - terms[k][0]).max() > 1e-3 * np.abs(F).max(), k
        g.run(0)
        fg, ob = g.get_state("FORCE"), g.observe()
        print("%s stage %d prec %d: force rel err %.3e; list energies %s" % (system, stage, prec, rel_err(fg, F),
              " ".join("%.2e" % (abs(ob["epot_list"][h] - e) / abs(e)) for h, e in zip(hl, el))))
        assert rel_err(fg, F) < TOL_FB[prec]
        for h, e in zip(hl, el):
            assert ob["epot_list"][h] == pytest.approx(e, rel=TOL_E[prec])
        assert ob["epot_lj"] == pytest.approx(elj, rel=TOL_E[prec], abs=1e-9)


# ---- 10: a reaction puts new bonds into a spline-tabulated list ---------------------------------------------------------

LJR = (1.0, 0.6, RC)
RSEED = 77


def reaction_bond_table():
    r = 0.4 + 0.05 * np.arange(17)                   # [0.4, 1.2]
    return 0.4, 0.05, 20.0 * (r - 0.7) ** 2 + 1.5 * np.cos(25.0 * r), -40.0 * (r - 0.7) + 37.5 * np.sin(25.0 * r)


def check_reacted(g, hb, spec, prec):
    bonds = g.get_list(hb)
    print("bonds formed", len(bonds))
    assert len(bonds) >= 50
    excl = g.get_exclusions()
    have = {(min(a, b), max(a, b)) for a, b in excl.tolist()}
    assert all((min(a, b), max(a, b)) in have for a, b in bonds.tolist())
    x, L = g.get_state("POS"), np.array(spec["box"])
    mat = {(a, b): S.lj(*LJR) for a in range(2) for b in range(a, 2)}
    F, elj, _ = S.pair_sums(x, L, g.get_state("TYPE"), mat, excluded=[(a - 1, b - 1) for a, b in excl.tolist()])
    Fb, eb = S.bond_terms(x, L, bonds - 1, S.Table(*reaction_bond_table(), 2))
    Fbl, _ = S.bond_terms(x, L, bonds - 1, S.Table(*reaction_bond_table(), 1))
    assert rel_err(F + Fbl, F + Fb) > 1e-3
    g.run(0)
    fg, ob = g.get_state("FORCE"), g.observe()
    print("prec %d: force rel err %.3e, list energy %.3e" % (prec, rel_err(fg, F + Fb), abs(ob["epot_list"][hb] - eb) / abs(eb)))
    assert rel_err(fg, F + Fb) < TOL_FB[prec]
    assert ob["epot_list"][hb] == pytest.approx(eb, rel=TOL_E[prec])
    assert ob["epot_lj"] == pytest.approx(elj, rel=TOL_E[prec])


@pytest.mark.parametrize("prec", [64, 32])
def test_reaction_bonds_in_a_spline_list(make_gpu, prec):
    spec = melt("a")
    g = make_gpu(prec)
    setup(g, spec)
    for a in range(2):
        for b in range(a, 2):
            g.nb_lj(a, b, *LJR, True)
    hb = g.list_create(2, "TABULATED", False)
    g.list_set_params(hb, [g.table_create(*reaction_bond_table(), itype=2)])
    g.reaction_init(5, True, 0, RSEED)
    g.reaction_add(0, 1, 1, 1, 0, 1, 0, 1, 1e9, 0.9, bond_list=hb)
    g.reactions_enable(True)
    g.run(20)
    check_reacted(g, hb, spec, prec)


@pytest.mark.parametrize("prec", [64, 32])
def test_reaction_bonds_in_a_spline_list_through_the_shim(tmp_path, prec):
    """the same as SetupReactions builds it: FixedPairListTabulated(system, fpl, Tabulated(itype=2, filename=...))"""
    from chemlab_amd import espp
    spec = melt("a")
    r0, dr, e, f = reaction_bond_table()
    np.savetxt(tmp_path / "table_b1.pot", np.stack([r0 + dr * np.arange(len(e)), e, f], 1), fmt="%.17g")
    prev = espp._factory[0]
    espp.set_engine_factory(lambda: Engine(device=0, precision=prec))
    try:
        system = espp.System()
    finally:
        espp.set_engine_factory(prev)
    try:
        system.rng = espp.esutil.RNG(RSEED)
        system.skin = SKIN
        box = tuple(spec["box"])
        system.bc = espp.bc.OrthorhombicBC(system.rng, box)
        system.storage = espp.storage.DomainDecomposition(system, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), RC, SKIN))
        integrator = espp.integrator.VelocityVerlet(system)
        integrator.dt = DT
        plist = [[i + 1, int(spec["types"][i]), espp.Real3D(*spec["pos"][i]), espp.Real3D(*spec["vel"][i]), 1.0, 0] for i in range(spec["n"])]
        system.storage.addParticles(plist, "id", "type", "pos", "v", "mass", "state")
        system.storage.decompose()
        vl = espp.VerletList(system, cutoff=RC, exclusionlist=espp.DynamicExcludeList(integrator, []))
        ljs = espp.interaction.VerletListLennardJones(vl)
        for a in range(2):
            for b in range(a, 2):
                ljs.setPotential(type1=a, type2=b, potential=espp.interaction.LennardJones(epsilon=LJR[0], sigma=LJR[1], cutoff=LJR[2]))
        system.addInteraction(ljs, "lj")
        fpl = espp.FixedPairList(system.storage)
        inter = espp.interaction.FixedPairListTabulated(system, fpl, espp.interaction.Tabulated(itype=2, filename=str(tmp_path / "table_b1.pot")))
        system.addInteraction(inter, "fpl_reaction")
        ar = espp.integrator.ChemicalReaction(system, vl, system.storage, None, 5)
        ar.nearest_mode = True
        ar.add_reaction(espp.integrator.Reaction(type_1=0, type_2=1, delta_1=1, delta_2=1, min_state_1=0, max_state_1=1, min_state_2=0, max_state_2=1,
                                                 rate=1e9, fpl=fpl, cutoff=0.9))
        integrator.addExtension(ar)
        integrator.run(20)
        check_reacted(system.engine, fpl.handle, spec, prec)
    finally:
        system.engine.close()


# ---- 11: linear data: every kind is the oracle's linear table -------------------------------------------------------------

@pytest.mark.parametrize("itype", [2, 3])
def test_linear_data_matches_the_oracle(make_gpu, make_oracle, itype):
    """columns y = a + b r: Akima and the natural spline reproduce them, so the run of test 7 must give the oracle's
    linear-table trajectory and energies to the fp64 tolerances of test_gpu_parity."""
    spec = melt("a")
    ta, tb = linear_tables()
    g, o = make_gpu(64), make_oracle()
    for e in (g, o):
        setup(e, spec)
        e.nb_lj(0, 1, *LJ01, True)
    g.nb_table(0, 0, *ta, RC, itype=itype); g.nb_table(1, 1, *tb, RC, itype=itype)
    o.nb_table(0, 0, *ta, RC); o.nb_table(1, 1, *tb, RC)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < TOL[64]
    og, oo = g.observe(), o.observe()
    assert og["epot_tab"] == pytest.approx(oo["epot_tab"], rel=1e-11) and og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=1e-11)
    assert og["ekin"] == pytest.approx(oo["ekin"], rel=1e-12)
    g.run(60); o.run(60)
    assert g.timers()["rebuilds"] >= 2
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-8      # (at positions that agree to 1e-9: test_gpu_parity's bound behind a run)
    og, oo = g.observe(), o.observe()
    for k in ("epot_tab", "epot_lj", "ekin"):
        print(k, og[k], oo[k])
        assert og[k] == pytest.approx(oo[k], rel=1e-9)                      # (likewise)
