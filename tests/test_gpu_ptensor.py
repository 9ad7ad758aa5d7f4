"""chem_get_pressure_tensor on the device against tests/ptensor_ref.py, at the engine's own positions and velocities, part by
part and component by component: oriented two-particle probes (LJ, table, Coulomb, capped, resolution-scaled and force-capped
pairs; harmonic, FENE and hybrid bonds; one list of oriented triples or quadruples per angular and dihedral kind of the zoo) whose
six components are pairwise distinct by more than 1000 tolerances in every part, melts under every pair-kernel mode, the
molecule zoo of tests/bonded_ref.py with every bonded kind (angles and dihedrals: non-zero components, zero trace) -- on the tile
path, the per-cell list, the brute-force list, one slab that is its own neighbour and two and three in-process slabs, in both
precisions -- and that asking for the tensor leaves no trace in a run.

Tolerance: the project's virial tolerance (tests/test_gpu_geometry.py, tests/test_gpu_pressure.py: 1e-10 in fp64, 2e-5 in
fp32), per component, relative to the sum of the absolute values of that component's terms, which the reference returns beside
each sum.  In fp32 a pair in the shell of its cutoff may be decided the other way; it moves a component by at most |r F(rc)|
(test_gpu_pressure.shell_slack), and every melt is chosen so that this stays below the tolerance itself.

Measured (MI355X, largest error / scale over the components and paths; DESIGN.md "Pressure tensor" has the table): fp64 at most
3.1e-15 in every non-bonded part, 2.7e-15 kinetic, 5.2e-12 in every list; fp32 6.3e-12 in the lists, at most 1.4e-6 non-bonded, 5.7e-9 kinetic.

The list `angh_pi` (harmonic angle, theta0 = pi) holds the zoo's members 1e-5 off folded, where dU / sin(theta) is 3e6 and the
force kernels' form of the bending term (a difference of nearly equal vectors) is off by 3e-10 of the list's scale; the tensor
pass evaluates bonded_term in its EXACT form and measures 2.4e-14 there."""
import numpy as np
import pytest

import bonded_ref as B
import ptensor_ref as PT
from chemlab_amd import workloads as W
from test_gpu_pressure import PATHS, TOL, ZOO_PATHS, melt, on_ranks, shell_slack, zoo_of

pytestmark = pytest.mark.gpu


def tensor_on_ranks(make_gpu, prec, path, setup, steps=0):
    """[(tensor dict, pressure dict, POS, VEL)] per rank of `path`, all taken at the same state"""
    made, got = [], {}

    def mk(p):
        made.append(make_gpu(p))
        return made[-1]

    def wrapped(g):
        setup(g)
        g.run(steps)
        before = g.pressure()
        got[id(g)] = (g.pressure_tensor(), before, g.pressure_tensor())
    out = on_ranks(mk, prec, path, wrapped)      # (on_ranks makes its engines in rank order and returns in rank order)
    res = []
    for g, (p, x, v) in zip(made, out):
        t, before, again = got[id(g)]
        # pressure(): the same bits before and after a tensor call (its per-list sums are atomics: those to rounding)
        assert all(before[k] == p[k] for k in ("volume", "mv2", "virial_nb"))
        assert np.allclose(before["virial_list"], p["virial_list"], rtol=1e-12, atol=0.0) and before["pressure"] == pytest.approx(p["pressure"], rel=1e-12)
        assert all(np.array_equal(t[k], again[k]) for k in ("kinetic", "virial_nb"))      # block partials folded in a fixed order
        for k in ("virial_list", "virial", "tensor"):                                      # (the per-list sums are atomics: to rounding)
            assert np.allclose(t[k], again[k], rtol=1e-12, atol=1e-12 * max(np.abs(t[k]).max(), 1e-300) if t[k].size else 0.0)
        res.append((t, p, x, v))
    return res


def check(t, p, ref, prec, what, nb_slack=0.0, names=()):
    """every part component by component, then the consistency of the whole"""
    tol = TOL[prec]
    parts = [("kinetic", t["kinetic"], ref["kinetic"], ref["kinetic_scale"], 0.0), ("virial_nb", t["virial_nb"], ref["virial_nb"], ref["virial_nb_scale"], nb_slack)]
    assert t["virial_list"].shape == ref["virial_list"].shape
    for l in range(len(ref["virial_list"])):
        parts.append(("list %s" % (names[l] if names else l), t["virial_list"][l], ref["virial_list"][l], ref["virial_list_scale"][l], 0.0))
    for name, a, b, s, slack in parts:
        err = np.abs(a - b) / np.maximum(s, 1e-300)
        print("%s fp%d %-18s err/scale %s" % (what, prec, name, " ".join("%.1e" % e for e in err)))
    missed = [(name, float((np.abs(a - b) / np.maximum(s, 1e-300)).max())) for name, a, b, s, slack in parts if not np.all(np.abs(a - b) <= tol * s + slack)]
    assert not missed, (what, "err/scale above %g" % tol, missed)
    assert t["volume"] == pytest.approx(ref["volume"], rel=1e-14)
    assert np.all(np.abs(t["virial"] - ref["virial"]) <= tol * (ref["scale"] - ref["kinetic_scale"]) + nb_slack), what
    assert np.all(np.abs(t["tensor"] - ref["tensor"]) <= (tol * ref["scale"] + nb_slack) / ref["volume"]), what
    # consistency: the parts add up, the trace is the scalar pressure
    assert np.all(np.abs(t["virial"] - (t["virial_nb"] + t["virial_list"].sum(0))) <= 1e-14 * ref["scale"])
    assert np.all(np.abs(t["tensor"] - (t["kinetic"] + t["virial"]) / t["volume"]) <= 1e-14 * ref["scale"] / ref["volume"])
    assert abs(t["tensor"][:3].sum() / 3.0 - p["pressure"]) <= (tol * ref["scale"][:3].sum() + 3.0 * nb_slack) / (3.0 * ref["volume"]), what


def same_on_every_rank(out, ref, prec):
    t0 = out[0][0]
    for t, _, _, _ in out[1:]:
        assert all(np.array_equal(t[k], t0[k]) for k in ("kinetic", "virial_nb", "virial_list", "virial", "tensor"))      # one all-reduce, the same arithmetic behind it


# ---- 1: oriented probes --------------------------------------------------------------------------------------------------------
def setup_probe(g, spec):
    W.apply(spec, g, thermostat=False, reactions=False)
    for l in spec["probe_lists"]:
        h = g.list_create(l["arity"], l["kind"], False)
        g.list_set_params(h, [g.table_create(*l["table"])] if l.get("table") is not None else l["params"])
        if l.get("lam") is not None:
            g.list_set_hybrid(h, l["lam"], 0.01)            # lambda = lam at step 0, where the tensor is taken
        g.list_add(h, l["ids"])


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("context", sorted(PT.PROBE_KINDS))
def test_oriented_probes(make_gpu, context, path, prec):
    spec = PT.probe_spec(context, "brute" if path == "brute" else "big")
    out = tensor_on_ranks(make_gpu, prec, path, lambda g: setup_probe(g, spec))
    for r, (t, p, x, v) in enumerate(out):
        pairs = PT.capped_pairs(spec, x) if context == "rescap" else None
        ref = PT.pressure_tensor(spec, x, v, lists=spec["probe_lists"], pairs=pairs)
        # the condition (tests/test_ptensor_ref.py asserts it at the spec's positions): no two components of a part agree
        assert PT.distinct(ref["kinetic"], TOL[prec], ref["kinetic_scale"])
        assert PT.distinct(ref["virial_nb"], TOL[prec], ref["virial_nb_scale"]) or (context == "bonded" and np.all(ref["virial_nb_scale"] == 0.0))
        assert all(PT.distinct(w, TOL[prec], s) for w, s in zip(ref["virial_list"], ref["virial_list_scale"]))
        check(t, p, ref, prec, "probe %s %s rank %d" % (context, path, r), names=[l["name"] for l in spec["probe_lists"]])
    same_on_every_rank(out, ref, prec)


# ---- 2: melts -----------------------------------------------------------------------------------------------------------------
def feature_melt(kind):
    """the jittered lattices of tests/test_gpu_resolution.py / tests/test_gpu_capped.py (9.0^3, tiles; 5.4^3 for the paths
    without tiles is not needed: option tiles = 0 serves): resolution marks, caps, both -- MODE 5, 6, 7 of the pair kernels"""
    import test_gpu_capped as C
    import test_gpu_resolution as R
    spec = R.system("a")
    return {"res": lambda: R.pair_spec(spec), "cap": lambda: C.pair_spec(spec), "rescap": lambda: C.pair_spec(spec, resolution=True)}[kind]()


def melt_of(kind, path):
    """test_gpu_pressure.melt, unless a pair of it lies in the shell of its cutoff and the slack exceeds the tolerance (the
    216-particle LJ melt of the brute-force list): then the same recipe from the first seed that keeps the condition, which is
    decided on the CPU from the spec's own positions and the reference alone"""
    def keeps(spec):
        ref = PT.pressure_tensor(spec, spec["pos"], spec["vel"])
        return shell_slack(spec, spec["pos"], 32) <= TOL[32] * ref["virial_nb_scale"].min()

    spec = melt(kind, path)
    if keeps(spec):
        return spec
    assert kind == "lj"                      # (the recipe below is melt's for this kind)
    import helpers as H
    for case in range(11, 40):
        spec = H.pair_matrix_spec(case, n=spec["n"], kind="lj_only")
        spec["rc"], spec["skin"] = min(spec["rc"], 2.4), min(spec["skin"], 0.3)
        spec["lj"] = [l[:4] + (min(l[4], spec["rc"]),) + l[5:] for l in spec["lj"]]
        box = np.asarray(spec["box"])
        right_box = box.max() < 3 * (spec["rc"] + spec["skin"]) and box.min() > 2 * spec["rc"] if path == "brute" else box.min() >= 6 * (spec["rc"] + spec["skin"])
        if right_box and keeps(spec):
            return spec
    raise AssertionError("no seed keeps the condition")


def melt_slack(spec, x, prec, ref):
    """shell_slack, and its condition: it stays below the tolerance of every component"""
    slack = shell_slack(spec, x, prec)
    assert slack <= TOL[prec] * ref["virial_nb_scale"].min(), (slack, ref["virial_nb_scale"])
    return slack


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("kind", ["lj", "table", "coulomb"])
def test_melt_tensor(make_gpu, kind, path, prec):
    spec = melt_of(kind, path)
    ref0 = PT.pressure_tensor(spec, spec["pos"], spec["vel"])
    melt_slack(spec, spec["pos"], prec, ref0)            # the condition, on the CPU from the spec's own positions, before any GPU run
    out = tensor_on_ranks(make_gpu, prec, path, lambda g: W.apply(spec, g, thermostat=False, reactions=False))
    for r, (t, p, x, v) in enumerate(out):
        ref = PT.pressure_tensor(spec, x, v)
        assert ref["virial_nb_scale"].min() > 0 and t["virial_list"].shape == (0, 6)
        check(t, p, ref, prec, "%s %s rank %d" % (kind, path, r), melt_slack(spec, x, prec, ref))
    same_on_every_rank(out, ref, prec)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ["tiles", "cells", "dd_self"])
@pytest.mark.parametrize("kind", ["res", "cap", "rescap"])
def test_melt_tensor_with_resolution_and_caps(make_gpu, kind, path, prec):
    """MODE 5, 6 and 7 of the tile kernels and the row kernels' resolution and cap packs"""
    spec = feature_melt(kind)
    # the condition, here in the form of the capped and resolution tests: no pair with a term within 2e-6 of its cutoff, on
    # either side -- no pair that fp32 may decide the other way, the slack is zero
    assert PT.capped_pairs(spec, spec["pos"], gap=True) > 2e-6
    out = tensor_on_ranks(make_gpu, prec, path, lambda g: W.apply(spec, g, thermostat=False, reactions=False))
    for r, (t, p, x, v) in enumerate(out):
        assert PT.capped_pairs(spec, x, gap=True) > 2e-6
        ref = PT.pressure_tensor(spec, x, v, pairs=PT.capped_pairs(spec, x))
        check(t, p, ref, prec, "%s %s rank %d" % (kind, path, r))
    same_on_every_rank(out, ref, prec)


def dimer_melt(path):
    """melt("lj") with disjoint nearest-neighbour pairs bonded by ONE harmonic list and excluded: what the tile path evaluates
    inside the force kernel (inline bonds).  The bonded partners sit inside the cutoff, so the single-domain list holds them and
    the energy pass -- and the tensor pass -- take their pair term out again."""
    from scipy.spatial import cKDTree
    import aged_ref
    spec = melt_of("lj", path)
    n, x, L = spec["n"], np.asarray(spec["pos"]), np.asarray(spec["box"], np.float64)
    near = cKDTree(aged_ref.fold(x, L), boxsize=L).query_pairs(1.2 * float(L[0]) / round(n ** (1 / 3)), output_type="ndarray")
    near = near[np.lexsort((near[:, 1], near[:, 0]))]
    used, take = np.zeros(n, bool), []
    for i, j in near:
        if not used[i] and not used[j]:
            used[i] = used[j] = True
            take.append((i, j))
    bonds = np.asarray(take, np.int64) + 1
    d = x[bonds[:, 0] - 1] - x[bonds[:, 1] - 1]
    d -= L * np.rint(d / L)
    r = np.sqrt((d * d).sum(1))
    assert len(bonds) > n // 4 and r.max() < min(l[4] for l in spec["lj"])      # every bonded pair is inside every pair cutoff
    lists = [dict(name="harm", kind="HARMONIC", arity=2, params=[30.0, 0.9 * float(r.mean())], ids=bonds)]
    return dict(spec, exclusions=bonds), lists


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("inline", [1, 0])
@pytest.mark.parametrize("path", ["tiles", "dd_self"])
def test_melt_tensor_with_inline_bonds(make_gpu, path, inline, prec):
    """The excluded pairs of inline bonds: in the list on a single domain (taken out again by the tensor pass), left out by the
    list build on slabs; the same answer with the option off, where the bonded kernels run."""
    spec, lists = dimer_melt(path)

    def setup(g):
        g.set_option("bonds_inline", inline)
        W.apply(dict(spec, exclusions=None), g, thermostat=False, reactions=False)
        h = g.list_create(2, "HARMONIC", False)
        g.list_set_params(h, lists[0]["params"])
        g.list_add(h, lists[0]["ids"])
        g.set_exclusions(spec["exclusions"])
    out = tensor_on_ranks(make_gpu, prec, path, setup)
    for r, (t, p, x, v) in enumerate(out):
        ref = PT.pressure_tensor(spec, x, v, lists=lists)
        unexcluded = PT.pressure_tensor(dict(spec, exclusions=None), x, v)
        assert np.any(np.abs(unexcluded["virial_nb"] - ref["virial_nb"]) > 1e3 * TOL[prec] * ref["virial_nb_scale"])      # the excluded pairs show (the bonds lie along z)
        check(t, p, ref, prec, "dimers %s inline %d rank %d" % (path, inline, r), melt_slack(spec, x, prec, ref), names=["harm"])


# ---- 3: the zoo ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name", sorted(ZOO_PATHS))
def test_zoo_tensor_every_bonded_kind(make_gpu, name, prec):
    """Every bonded kind, each list on its own; velocities s_i (1, 2, 3).  Angle and dihedral lists: components, and no trace."""
    box, path = ZOO_PATHS[name]
    z = zoo_of(box)
    use = [i for i, l in enumerate(z["lists"]) if l["name"] not in B.FINITE_ONLY_LISTS]
    n = z["n"]
    vel = (0.1 * (1 + np.arange(n) % 7) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0))[:, None] * np.array([1.0, 2.0, 3.0])
    out = tensor_on_ranks(make_gpu, prec, path, lambda g: B.build(g, z, use, vel=vel))
    lists = [z["lists"][i] for i in use]
    assert {l["arity"] for l in lists} == {2, 3, 4}
    for r, (t, p, x, v) in enumerate(out):
        ref = PT.pressure_tensor(dict(z, lj=[], tables=[]), x, v, lists=lists)
        assert np.all(ref["virial_nb"] == 0.0) and np.all(t["virial_nb"] == 0.0)            # the zoo's clusters exclude each other completely
        check(t, p, ref, prec, "zoo %s rank %d" % (name, r), names=[l["name"] for l in lists])
        for l, lst in enumerate(lists):
            w, s = t["virial_list"][l], ref["virial_list_scale"][l]
            if lst["arity"] > 2:
                assert np.abs(w).max() > 1e-3 * s.max(), lst["name"]                       # evaluated ...
                assert abs(w[:3].sum()) <= TOL[prec] * s[:3].sum(), lst["name"]             # ... and traceless
                assert p["virial_list"][l] == 0.0
    same_on_every_rank(out, ref, prec)


# ---- 5: no trace in the run -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path,baro", [("tiles", False), ("dd_self", False), ("tiles", True)])      # (the barostat is not served on the decomposed path)
def test_the_tensor_leaves_no_trace_in_a_run(make_gpu, path, prec, baro):
    spec = melt("lj", path)

    def trajectory(ask):
        g = make_gpu(prec)
        for k, v in PATHS[path][1].items():
            g.set_option(k, v)
        W.apply(spec, g, thermostat=False, reactions=False)
        if baro:
            g.barostat_berendsen(1.0, 0.5)
        g.run(10)
        seen = ask(g)
        g.run(10)
        return seen, g.get_state("POS"), g.get_state("VEL"), g.get_state("FORCE"), g.box() if baro else None

    a = trajectory(lambda g: g.pressure())
    b = trajectory(lambda g: (g.pressure(), g.pressure_tensor(), g.pressure())[::2])
    assert b[0][0] == b[0][1] == a[0]                       # pressure(): the same bits before and after the tensor
    for u, w in zip(a[1:4], b[1:4]):
        assert np.array_equal(u, w)
    if baro:
        assert np.array_equal(a[4], b[4]) and not np.array_equal(a[4], np.asarray(spec["box"], np.float64))
