"""1-4 Coulomb pair lists (CHEM_POT_COULOMB_BOND), host side: the numpy reference itself (tests/coulomb14_ref.py), the shim's
one-library-list-per-kind rule, the driver's restatement of gromacs_topology.py:1391-1409 (with the static interactions
acting), the CPU checker's refusal and the define.  Nothing here needs a GPU."""
import os
import types

import numpy as np
import pytest

import coulomb14_ref as C14
from chemlab_amd import _capi

K_QQ = 138.935485


# ---- 1: the reference ------------------------------------------------------------------------------------------------------

def small_system(n=40, npairs=60, seed=5):
    rng = np.random.default_rng(seed)
    box = np.array([4.0, 4.4, 4.8])
    pos = rng.uniform(0.0, 1.0, (n, 3)) * box
    types_ = rng.integers(0, 3, n)
    q = rng.choice([-1.0, -0.5, 0.417, 0.5, 1.0], n)
    iu = np.triu_indices(n, 1)
    sel = rng.permutation(len(iu[0]))[:npairs]
    return box, pos, types_, q, np.stack([iu[0][sel], iu[1][sel]], 1)


@pytest.mark.parametrize("form", ["plain", "typed", "lambda"])
def test_reference_force_is_minus_the_gradient(form):
    """central differences of U: h = 1e-6 leaves a truncation error ~ h^2 U''' and a rounding error ~ eps U / h, both below
    1e-7 of the largest force here; no listed pair may sit within 10 h of its cutoff (the energy jumps there)"""
    box, pos, types_, q, pairs = small_system()
    kw = dict(k=3.0, rc=1.7)
    if form == "typed":
        kw = dict(types=types_, typed={(0, 0): (3.0, 1.7), (1, 2): (2.0, 2.1), (0, 2): (5.0, 1.2)})
    if form == "lambda":
        kw["lam"] = np.random.default_rng(2).uniform(0.0, 1.0, len(pairs))
    h = 1e-6
    _, _, r = C14.distances(pos, box, pairs)
    kk, rr = C14.entry_params(pairs, kw.get("k", 0.0), kw.get("rc", 1.0), kw.get("types"), kw.get("typed"))
    assert np.abs(r - rr).min() > 10 * h
    assert 5 < (r[kk != 0] <= rr[kk != 0]).sum() < (kk != 0).sum()           # some inside, some outside
    F, e = C14.terms(pos, box, q, pairs, **kw)
    assert np.abs(F).max() > 0
    num = np.zeros_like(F)
    for i in range(len(pos)):
        for c in range(3):
            xp, xm = pos.copy(), pos.copy()
            xp[i, c] += h; xm[i, c] -= h
            num[i, c] = -(C14.energy(xp, box, q, pairs, **kw) - C14.energy(xm, box, q, pairs, **kw)) / (2 * h)
    assert np.abs(num - F).max() < 1e-7 * np.abs(F).max()
    assert np.abs(F.sum(0)).max() < 1e-12 * np.abs(F).max()


def test_reference_closed_form_through_the_face_and_inclusive_cutoff():
    box = np.array([10.0, 10.0, 10.0])
    pos = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [9.5, 1.0, 1.0], [1.0, 4.0, 1.0]])
    q = np.array([1.0, -2.0, 0.5, 1.0])
    pairs = [(0, 1), (0, 2), (0, 3)]                                          # r = 1, r = 1.5 through the boundary, r = 3 (outside)
    F, e = C14.terms(pos, box, q, pairs, k=2.0, rc=1.5)
    assert e == pytest.approx(2.0 * (1.0 * -2.0 / 1.0 + 1.0 * 0.5 / 1.5))     # r = rc counts
    # particle 0 is pulled towards 1 at +x (opposite charges) and pushed away from the image of 2 at x = -0.5 (like charges)
    assert F[0] == pytest.approx([2.0 * 2.0 / 1.0 + 2.0 * 0.5 * 1.5 / 1.5 ** 3, 0.0, 0.0])
    assert F[2] == pytest.approx([-2.0 * 0.5 * 1.5 / 1.5 ** 3, 0.0, 0.0]) and np.all(F[3] == 0.0)
    assert C14.terms(pos, box, q, pairs, k=2.0, rc=1.4999)[1] == pytest.approx(-4.0)
    # an unlisted pair gets nothing however close; lambda scales; a type pair without parameters gets nothing
    assert C14.terms(pos, box, q, [(0, 2)], k=2.0, rc=1.5)[1] == pytest.approx(2.0 * 0.5 / 1.5)
    assert C14.terms(pos, box, q, pairs, k=2.0, rc=1.5, lam=[0.25, 1.0, 1.0])[1] == pytest.approx(2.0 * (0.25 * -2.0 + 0.5 / 1.5))
    ty = np.array([0, 1, 2, 0])
    assert C14.terms(pos, box, q, pairs, types=ty, typed={(1, 0): (3.0, 1.2)})[1] == pytest.approx(-6.0)
    assert list(C14.live([1.0, 0.0, 0.5], [(0, 1), (0, 2)])) == [False, True]


# ---- 2: the shim -------------------------------------------------------------------------------------------------------------

class StubEngine:
    """records the set-up calls the shim makes; list_create hands out consecutive handles"""

    def __init__(self):
        self.calls = []
        self.n = 0
        self.nlists = 0

    def list_create(self, *a, **k):
        self.calls.append(("list_create", a, k))
        self.nlists += 1
        return self.nlists - 1

    def __getattr__(self, name):
        def rec(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return rec


def shim_system(engine):
    from chemlab_amd import espp
    old = espp._factory[0]
    espp.set_engine_factory(lambda: engine)
    try:
        system = espp.System()
    finally:
        espp.set_engine_factory(old)
    system.storage = types.SimpleNamespace(system=system)
    return system


def of(eng, name):
    return [c for c in eng.calls if c[0] == name]


def test_one_list_object_carries_one_library_list_per_kind():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    fpl = espp.FixedPairList(system.storage)
    fpl.addBonds([(1, 4), (5, 8)])
    lj = espp.interaction.FixedPairListLennardJones(system, fpl, espp.interaction.LennardJones(epsilon=0.5, sigma=0.3, cutoff=1.2))
    assert fpl.handle == 0 and of(eng, "list_create") == [("list_create", (2, "LJ_BOND", False), {})]
    assert of(eng, "list_add") == [("list_add", (0, [(1, 4), (5, 8)]), {})]
    pot = espp.interaction.CoulombTruncated(prefactor=K_QQ * 0.5, cutoff=0.9)
    qq = espp.interaction.FixedPairListCoulombTruncated(system, fpl, pot)
    assert fpl.handle == 0                                                     # every earlier caller sees what it saw
    assert of(eng, "list_create")[1] == ("list_create", (2, "COULOMB_BOND", False), {}) and _capi.POT["COULOMB_BOND"] == 6
    assert of(eng, "list_add")[1] == ("list_add", (1, [(1, 4), (5, 8)]), {})   # the same entries
    assert of(eng, "list_set_params")[1] == ("list_set_params", (1, [K_QQ * 0.5, 0.9]), {})
    assert (lj.handle, qq.handle) == (0, 1) and qq.getFixedPairList() is fpl
    fpl.addBonds([(9, 12)])                                                    # later additions reach both
    assert of(eng, "list_add")[2:] == [("list_add", (0, [(9, 12)]), {}), ("list_add", (1, [(9, 12)]), {})]
    # the same kind again binds nothing new
    espp.interaction.FixedPairListCoulombTruncated(system, fpl, pot)
    assert len(of(eng, "list_create")) == 2
    # PotentialEnergy reports the interaction's own list
    eng.observe = lambda: dict(epot_list=[3.0, -7.5])
    assert espp.analysis.PotentialEnergy(system, qq).compute() == -7.5 and espp.analysis.PotentialEnergy(system, lj).compute() == 3.0


def test_types_form_and_lambda_lists():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    fpl = espp.FixedPairList(system.storage)
    fpl.addBonds([(2, 5)])
    lj = espp.interaction.FixedPairListTypesLennardJones(system, fpl)
    lj.setPotential(0, 1, espp.interaction.LennardJones(epsilon=0.5, sigma=0.3, cutoff=1.2))
    qq = espp.interaction.FixedPairListTypesCoulombTruncated(system, fpl)
    assert len(of(eng, "list_create")) == 1                                    # nothing before the first setPotential
    pot = espp.interaction.CoulombTruncated(prefactor=2.0, cutoff=0.9)
    qq.setPotential(type1=0, type2=1, potential=pot)
    qq.setPotential(1, 1, pot)
    assert of(eng, "list_create")[1] == ("list_create", (2, "COULOMB_BOND", True), {})
    assert of(eng, "list_set_params")[1:] == [("list_set_params", (1, [2.0, 0.9]), dict(types=(0, 1))), ("list_set_params", (1, [2.0, 0.9]), dict(types=(1, 1)))]
    assert of(eng, "list_add")[1] == ("list_add", (1, [(2, 5)]), {})
    # FixedPairListLambda: every library list of the object is made hybrid, before it gets entries
    eng2 = StubEngine()
    system2 = shim_system(eng2)
    lam = espp.FixedPairListLambda(system2.storage, 0.25)
    lam.addBonds([(1, 2)])
    espp.interaction.FixedPairListLambdaHarmonic(system2, lam, espp.interaction.Harmonic(K=3.0, r0=1.0))
    espp.interaction.FixedPairListCoulombTruncated(system2, lam, pot)
    names = [c[0] for c in eng2.calls if c[0] in ("list_create", "list_set_hybrid", "list_add")]
    assert names == ["list_create", "list_set_hybrid", "list_add"] * 2
    assert of(eng2, "list_set_hybrid") == [("list_set_hybrid", (0, 0.25, 0.0), {}), ("list_set_hybrid", (1, 0.25, 0.0), {})]
    lam._set_rate(0.5)
    assert of(eng2, "list_set_hybrid")[2:] == [("list_set_hybrid", (0, 0.25, 0.5), {}), ("list_set_hybrid", (1, 0.25, 0.5), {})]


# ---- 3: the driver -----------------------------------------------------------------------------------------------------------

TOP = """[ defaults ]
; nbfunc comb-rule gen-pairs fudgeLJ fudgeQQ
1 2 no 1.0 %(fudge)s

[ atomtypes ]
;name mass charge ptype sigma epsilon
A 1.0 %(qa)s A 0.5 1.0
B 1.0 %(qb)s A 0.5 1.0
C 1.0 0.000 A 0.0 0.0

[ moleculetype ]
MOL 1

[ atoms ]
; nr type resnr residue atom cgnr charge mass
1 A 1 MOL A1 1 %(qa)s 1.0
2 B 1 MOL B1 1 %(qb)s 1.0
3 C 1 MOL C1 1 0.000 1.0

[ bonds ]
1 2 1 0.5 1000.0
2 3 1 0.5 1000.0
%(pairs)s
[ system ]
X

[ molecules ]
MOL 2
"""
PAIRS = "\n[ pairs ]\n1 3 1 0.5 1.0\n1 2 1 0.5 1.0\n"


def read_top(tmp_path, fudge="0.5", qa="0.500", qb="-0.500", pairs=PAIRS):
    from chemlab_amd.chemlab import gromacs_topology
    f = tmp_path / "topol.top"
    f.write_text(TOP % dict(fudge=fudge, qa=qa, qb=qb, pairs=pairs))
    return gromacs_topology.GromacsTopology(str(f)).read()


def pair_setup(tmp_path, qq_cutoff, dynamic=False, **kw):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    gt = read_top(tmp_path, **kw)
    eng = StubEngine()
    system = shim_system(eng)
    dyn = {gt.atoms[3]["type_id"]} if dynamic else ()
    out = gromacs_topology.set_pair_interactions(espp, system, gt, 1.2, dynamic_type_ids=dyn, qq_cutoff=qq_cutoff, pairs_coulomb=True)
    names = [system.getNameOfInteraction(k) for k in range(system.getNumberOfInteractions())]
    return gt, eng, out, names


def test_driver_sets_the_static_and_the_dynamic_pairs(tmp_path):
    gt, eng, out, names = pair_setup(tmp_path, 0.9)
    assert list(gt.pairs) == [(1, 3), (4, 6), (1, 2), (4, 5)]
    assert names == ["lj14_0", "coulomb_14_0"] and list(out) == names
    fpl, inter = out["coulomb_14_0"]
    assert fpl is out["lj14_0"][0]                                             # the SAME list object, as in the reference
    assert (inter.potential.prefactor, inter.potential.cutoff) == (pytest.approx(K_QQ * 0.5, rel=1e-15), 0.9)
    assert of(eng, "list_create") == [("list_create", (2, "LJ_BOND", False), {}), ("list_create", (2, "COULOMB_BOND", False), {})]
    assert of(eng, "list_add")[1] == ("list_add", (1, [(1, 3), (4, 6), (1, 2), (4, 5)]), {})
    assert of(eng, "list_set_params")[1][1] == (1, [K_QQ * 0.5, 0.9])
    # a dynamic type: its pairs move to the Types list, which gets the term for the same type pairs as the dynamic LJ
    gt, eng, out, names = pair_setup(tmp_path, 0.9, dynamic=True)
    assert names == ["lj14_0", "coulomb_14_0", "dyn_lj14", "coulomb_14_1"]
    assert out["coulomb_14_1"][0] is out["lj14_dynamic"][0]
    created = of(eng, "list_create")
    assert [c[1][1:] for c in created] == [("LJ_BOND", False), ("COULOMB_BOND", False), ("LJ_BOND", True), ("COULOMB_BOND", True)]
    tc = gt.atoms[3]["type_id"]
    typed = [c for c in of(eng, "list_set_params") if c[1][0] == 3]
    assert sorted(tuple(sorted(c[2]["types"])) for c in typed) == sorted(tuple(sorted((t, tc))) for t in gt.used_atomsym_atomtype.values())
    assert all(c[1][1] == [K_QQ * 0.5, 0.9] for c in typed)
    assert [c for c in of(eng, "list_add") if c[1][0] == 3] == [("list_add", (3, [(1, 3), (4, 6)]), {})]


@pytest.mark.parametrize("kw, cutoff", [(dict(qa="0.000", qb="0.000"), 0.9), (dict(fudge="0.0"), 0.9), (dict(), 0.0)])
def test_driver_registers_nothing_when_the_term_is_zero(tmp_path, kw, cutoff):
    _, eng, out, names = pair_setup(tmp_path, cutoff, **kw)
    assert names == ["lj14_0"] and list(out) == ["lj14_0"]
    assert [c[1][1] for c in of(eng, "list_create")] == ["LJ_BOND"]


def test_default_keyword_still_refuses(tmp_path):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    gt = read_top(tmp_path)
    system = shim_system(StubEngine())
    with pytest.raises(NotImplementedError, match="1-4 Coulomb"):
        gromacs_topology.set_pair_interactions(espp, system, gt, 1.2, qq_cutoff=0.9)
    src = open(os.path.join(os.path.dirname(_capi.HERE), "chemlab_amd", "start_simulation.py")).read()
    assert "pairs_coulomb=True" in src                                        # the driver itself asks for the term


# ---- 4: the engine layer and the define -----------------------------------------------------------------------------------------

def test_cpu_checker_refuses_the_kind(make_oracle):
    o = make_oracle()
    with pytest.raises(NotImplementedError, match="1-4 Coulomb pairs: the CPU checker has no Coulomb term"):
        o.list_create(2, "COULOMB_BOND")
    with pytest.raises(NotImplementedError, match="1-4 Coulomb"):
        o.list_create(2, 6, True)
    assert o.list_create(2, "LJ_BOND") == 0                                    # every other kind as before


def test_header_holds_the_define():
    hdr = open(os.path.join(os.path.dirname(_capi.HERE), "include", "chem_mi355.h")).read()
    assert "#define CHEM_POT_COULOMB_BOND  6" in hdr and _capi.POT["COULOMB_BOND"] == 6
    assert len(set(_capi.POT.values())) == len(_capi.POT)
