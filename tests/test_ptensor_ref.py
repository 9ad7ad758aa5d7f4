"""CPU tests of tests/ptensor_ref.py, the fp64 reference of the pressure tensor: its two routes agree (sum of d (x) F against
minus the strain derivative of the energy, all nine strains), its trace is the scalar pressure of tests/pressure_ref.py, every
angle and dihedral list of the zoo is traceless and symmetric, and the conditions the device tests lean on hold for the
systems they use: the probes' six components -- two-particle clusters and oriented triples and quadruples of every kind of the
zoo -- are pairwise distinct by more than 1000 fp32 tolerances in every part, and the cutoff-shell slack of the fp32 melts stays
below the tolerance.  No engine in here."""
import numpy as np
import pytest

import aged_ref
import bonded_ref as B
import helpers as H
import pressure_ref as PR
import ptensor_ref as PT

TOL = {64: 1e-10, 32: 2e-5}


def zoo_lists(z):
    return [l for l in z["lists"] if l["name"] not in B.FINITE_ONLY_LISTS]


@pytest.fixture(scope="module")
def zoo_ref():
    z = B.zoo("tiles")
    lists = zoo_lists(z)
    x = aged_ref.fold(z["pos"], z["box"])
    return z, lists, PT.lists_direct(x, z["box"], z["types"], lists), PT.lists_strain(x, z["box"], z["types"], lists)


def test_component_order():
    m = np.arange(9.0).reshape(3, 3)
    assert list(PT.six(m)) == [0.0, 4.0, 8.0, 1.0, 2.0, 5.0] and PT.NAMES == ("xx", "yy", "zz", "xy", "xz", "yz")
    k, ka = PT.kinetic([2.0], [[1.0, 2.0, 3.0]])
    assert list(k) == [2.0, 8.0, 18.0, 4.0, 6.0, 12.0] and list(ka) == list(k)
    w, _ = PT.pairs_direct(np.array([[1.0, 2.0, 3.0]]), np.array([-0.5]))
    assert list(w) == [-0.5, -2.0, -4.5, -1.0, -1.5, -3.0]


@pytest.mark.parametrize("context", ["coulomb", "plain", "rescap"])
def test_two_routes_agree_on_the_nonbonded_pairs(context):
    spec = PT.probe_spec(context)
    d, fs = PT.capped_pairs(spec, spec["pos"]) if context == "rescap" else PT.nonbonded_pairs(spec, spec["pos"])
    assert len(fs) >= 9 and np.abs(fs).min() > 0
    w, a = PT.pairs_direct(d, fs)
    s = PT.pairs_strain(d, fs)
    assert np.abs(s - s.T).max() <= 1e-13 * a.max()
    assert np.all(np.abs(PT.six(s.T) - w) <= 1e-13 * a)


@pytest.mark.parametrize("which", ["coulomb probes", "lj melt", "coulomb melt"])
def test_lj_and_coulomb_pairs_against_the_strain_derivative_of_their_energies(which):
    """-dU/d eps with U written in torch, not the force law: the cross-check of the pair route proper"""
    if which == "coulomb probes":
        spec = PT.probe_spec("coulomb")
    else:
        spec = H.pair_matrix_spec(3 if which == "lj melt" else 7, n=512, kind="lj_only")
        if which == "coulomb melt":
            spec["q"] = np.random.default_rng(3).uniform(-1.0, 1.0, spec["n"])
            ty = spec["type_ids"]
            spec["coulomb"] = [(a, b, 138.935485, 0.9 * spec["rc"]) for i, a in enumerate(ty) for b in ty[i:]]
    d, fs, laws = PT.nonbonded_pairs(spec, spec["pos"], laws=True)
    assert (laws[:, 0] == 0).any() and ((laws[:, 0] == 1).any() or which == "lj melt") and (fs != 0).sum() > 10
    w, a = PT.pairs_direct(d, fs)
    s = PT.pairs_strain_energy(d, fs, laws)
    assert np.all(np.abs(PT.six(s.T) - w) <= 1e-12 * a) and np.abs(s - s.T).max() <= 1e-12 * a.max()


def test_two_routes_agree_on_a_melt_and_the_trace_is_the_pressure():
    rng = np.random.default_rng(5)
    spec = H.pair_matrix_spec(5, n=512, kind="mixed")
    vel = rng.normal(0, 1.0, (spec["n"], 3))
    d, fs = PT.nonbonded_pairs(spec, spec["pos"])
    w, a = PT.pairs_direct(d, fs)
    s = PT.pairs_strain(d, fs)
    assert np.all(np.abs(PT.six(s.T) - w) <= 1e-12 * a) and np.abs(s - s.T).max() <= 1e-12 * a.max()
    t, p = PT.pressure_tensor(spec, spec["pos"], vel), PR.pressure(spec, spec["pos"], vel)
    assert t["tensor"][:3].sum() / 3.0 == pytest.approx(p["pressure"], abs=1e-12 * p["scale"] / (3.0 * p["volume"]))
    assert t["kinetic"][:3].sum() == pytest.approx(p["mv2"], rel=1e-13)
    assert t["virial_nb"][:3].sum() == pytest.approx(p["virial_nb"], abs=1e-12 * p["virial_nb_scale"])


def test_two_routes_agree_on_every_list_of_the_zoo(zoo_ref):
    z, lists, direct, strain = zoo_ref
    assert {l["arity"] for l in lists} == {2, 3, 4}
    for l, (w, a), s in zip(lists, direct, strain):
        assert a.min() > 0, l["name"]
        assert np.all(np.abs(PT.six(s.T) - w) <= 1e-11 * a), (l["name"], PT.six(s.T) - w, a)


def test_angle_and_dihedral_lists_are_traceless_and_symmetric(zoo_ref):
    z, lists, direct, strain = zoo_ref
    for l, (w, a), s in zip(lists, direct, strain):
        assert np.abs(s - s.T).max() <= 1e-10 * a.max(), l["name"]            # no torque: the antisymmetric part vanishes
        if l["arity"] > 2:
            assert abs(w[:3].sum()) <= 1e-10 * a[:3].sum(), l["name"]         # angles alone: no change under uniform scaling
            assert np.abs(w).max() > 1e-3 * a.max(), l["name"]                # ... but the components are there


def test_pair_lists_of_the_zoo_have_the_scalar_virial_as_trace(zoo_ref):
    z, lists, direct, _ = zoo_ref
    x = aged_ref.fold(z["pos"], z["box"])
    rf = PR.lists_rf(x, z["box"], z["types"], lists)
    for l, (w, a), (ws, as_) in zip(lists, direct, rf):
        if l["arity"] == 2:
            assert w[:3].sum() == pytest.approx(ws, abs=1e-12 * as_), l["name"]


def test_hybrid_weight_and_coulomb_bond_in_the_list_routes():
    spec = PT.probe_spec("plain")
    lists = spec["probe_lists"] + [dict(name="c14", kind="COULOMB_BOND", arity=2, params=[138.935485, 1.4], ids=spec["probe_lists"][0]["ids"])]
    q = np.linspace(-1.0, 1.0, spec["n"])
    direct = PT.lists_direct(spec["pos"], spec["box"], spec["types"], lists, q)
    strain = PT.lists_strain(spec["pos"], spec["box"], spec["types"], lists, q)
    for l, (w, a), s in zip(lists, direct, strain):
        assert np.all(np.abs(PT.six(s.T) - w) <= 1e-12 * a), l["name"]
    plain = PT.lists_direct(spec["pos"], spec["box"], spec["types"], [dict(lists[2], lam=None)])[0][0]
    assert np.allclose(direct[2][0], PT.HYB_LAMBDA0 * plain, rtol=1e-13)


# ---- the conditions of the device tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", sorted(PT.PROBE_BOX))
@pytest.mark.parametrize("context", sorted(PT.PROBE_KINDS))
def test_probe_components_are_pairwise_distinct(context, box):
    """In each part the six components differ pairwise by more than 1000 x tolerance x scale (fp32 tolerance: the wider)."""
    spec = PT.probe_spec(context, box)
    L = spec["box"]
    assert np.all(np.floor(L / (spec["rc"] + spec["skin"])) >= 5) if box == "big" else np.floor(L / (spec["rc"] + spec["skin"])).max() < 3
    pairs = PT.capped_pairs(spec, spec["pos"]) if context == "rescap" else None
    ref = PT.pressure_tensor(spec, spec["pos"], spec["vel"], lists=spec["probe_lists"], pairs=pairs)
    assert PT.distinct(ref["kinetic"], TOL[32], ref["kinetic_scale"])
    if context == "bonded":
        assert np.all(ref["virial_nb_scale"] == 0.0) and len(spec["probe_lists"]) == 7      # triples and quadruples alone
    else:
        assert PT.distinct(ref["virial_nb"], TOL[32], ref["virial_nb_scale"])
    for l, lst in enumerate(spec["probe_lists"]):
        assert PT.distinct(ref["virial_list"][l], TOL[32], ref["virial_list_scale"][l]), lst["name"]
    # every kind of the context is there, and some clusters lie across a face, an edge and the corner
    assert set(spec["entries"]) == {k[0] for k in PT.PROBE_KINDS[context]}
    raw = [np.array([p for p in (np.asarray(spec["pos"])[i - 1] for i in e)]) for es in spec["entries"].values() for e in es]
    across = [tuple(bool(np.ptp(p[:, d]) > 0.5 * L[d]) for d in range(3)) for p in raw]      # (folded positions: a cluster across a face spans the box)
    assert any(sum(a) == 1 for a in across) and any(sum(a) == 2 for a in across) and any(sum(a) == 3 for a in across)


@pytest.mark.parametrize("box", sorted(PT.PROBE_BOX))
def test_oriented_triples_and_quadruples(box):
    """One list per angular and dihedral kind of the zoo: the two routes agree, the lists are traceless with components of the
    size of their terms, every cluster has an orientation of its own, and a chain is shorter than a cell."""
    spec = PT.probe_spec("bonded", box)
    lists = spec["probe_lists"]
    zoo_kinds = {l["kind"] for l in B.zoo("tiles")["lists"] if l["arity"] > 2}
    assert {l["kind"] for l in lists} == zoo_kinds and {l["arity"] for l in lists} == {3, 4}
    direct = PT.lists_direct(spec["pos"], spec["box"], spec["types"], lists)
    strain = PT.lists_strain(spec["pos"], spec["box"], spec["types"], lists)
    L, x = spec["box"], np.asarray(spec["pos"])
    firsts = []
    for l, (w, a), s in zip(lists, direct, strain):
        assert np.all(np.abs(PT.six(s.T) - w) <= 1e-12 * a) and np.abs(s - s.T).max() <= 1e-12 * a.max(), l["name"]
        assert abs(w[:3].sum()) <= 1e-12 * a[:3].sum() and np.abs(w).max() > 0.1 * a.max(), l["name"]
        for e in l["ids"]:
            d = x[e[0] - 1] - x[e[1] - 1]
            d -= L * np.rint(d / L)
            firsts.append(d / np.sqrt(d @ d) * (1 if e[0] < e[1] else -1))
            span = x[e - 1] - x[e[0] - 1]
            span -= L * np.rint(span / L)
            assert np.sqrt((span ** 2).sum(1)).max() < spec["rc"] + spec["skin"]
    firsts = np.array(firsts)
    dots = np.abs(firsts @ firsts.T) - np.eye(len(firsts))
    assert dots.max() < 1 - 1e-4                                                                  # no two first bonds parallel
    assert np.all(np.sort(np.abs(firsts), 1)[:, 0] > 1e-3)                                        # ... and none along an axis or in a coordinate plane


def test_probe_pairs_meet_what_their_names_say():
    spec = PT.probe_spec("rescap")
    import capped_ref
    import spline_ref
    t = capped_ref.total(spec["pos"], spec["box"], spec["types"], {(0, 0): spline_ref.lj(*PT.PROBE_LJ), (1, 1): spline_ref.lj(*PT.PROBE_LJ)},
                         {(0, 0): PT.PROBE_CAP}, spec["lam"], {(1, 1): PT.PROBE_FMAX})
    p = t["pairs"]
    assert p["inside"].astype(bool).any() and (p["capped"].astype(bool) & ~p["inside"].astype(bool)).any()      # inside and outside the cap radius
    mk = p["marked"].astype(bool)
    assert np.all((p["w"][mk] > 0) & (p["w"][mk] < 1))                                                          # 0 < lambda_i lambda_j < 1
    mag = np.abs(p["fs"]) * np.sqrt(p["r2"])
    assert (mk & (mag >= PT.PROBE_FMAX * (1 - 1e-12))).any() and (mk & (mag < 0.9 * PT.PROBE_FMAX)).any()        # force-capped and not
    c = PT.probe_spec("coulomb")
    d, fs = PT.nonbonded_pairs(c, c["pos"])
    assert len(fs) == len(c["entries"]["lj"]) + 2 * len(c["entries"]["coul"])                                 # a Coulomb pair carries two terms


def test_melts_of_the_device_tests_keep_the_shell_slack_below_the_tolerance():
    """The fp32 melts: what the pairs in the shell of their cutoff can move a component by stays below tolerance x scale, at the
    spec's own positions (tests/test_gpu_ptensor.py takes the melts from melt_of, which looks for a seed that keeps this, and
    asserts it again at the engine's positions)."""
    import test_gpu_ptensor as G
    from test_gpu_pressure import shell_slack
    for path in ("tiles", "brute"):
        for kind in ("lj", "table", "coulomb"):
            spec = G.melt_of(kind, path)
            ref = PT.pressure_tensor(spec, spec["pos"], spec["vel"])
            assert shell_slack(spec, spec["pos"], 32) <= TOL[32] * ref["virial_nb_scale"].min(), (kind, path)
    for kind in ("res", "cap", "rescap"):
        spec = G.feature_melt(kind)
        assert PT.capped_pairs(spec, spec["pos"], gap=True) > 2e-6, kind
