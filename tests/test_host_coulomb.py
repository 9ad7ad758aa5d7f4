"""Truncated Coulomb term, host side: the numpy reference itself (tests/coulomb_ref.py), the espressopp-shaped shim
objects, the driver's restatement of gromacs_topology.py:866-878 with its all-neutral short-cut, the refusal of 1-4 Coulomb
pairs, and the new C symbols.  Nothing here needs a GPU."""
import ctypes
import os
import types

import numpy as np
import pytest

import coulomb_ref as Q
from chemlab_amd import _capi

K_QQ = 138.935485


# ---- 1: the reference ------------------------------------------------------------------------------------------------------

def small_system(n=40, seed=5):
    rng = np.random.default_rng(seed)
    box = np.array([4.0, 4.4, 4.8])
    pos = rng.uniform(0.0, 1.0, (n, 3)) * box
    types_ = rng.integers(0, 3, n)
    q = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], n)
    return box, pos, types_, q


def test_reference_force_is_minus_the_gradient():
    """central differences of U on 40 particles: h = 1e-6 leaves a truncation error ~ h^2 U''' and a rounding error
    ~ eps U / h, both below 1e-7 of the largest force here; no pair may sit within 10 h of the cutoff (the energy jumps)"""
    box, pos, types_, q = small_system()
    k, rc, mask = 3.0, 1.7, {(0, 0), (0, 2), (1, 2), (1, 1)}
    excluded = [(0, 1), (2, 3), (4, 9)]
    h = 1e-6
    assert Q.min_gap_to_cutoff(pos, box, rc) > 10 * h
    F, e, w = Q.coulomb_sums(pos, box, types_, q, k, rc, mask, excluded)
    assert np.abs(F).max() > 0
    num = np.zeros_like(F)
    for i in range(len(pos)):
        for c in range(3):
            xp, xm = pos.copy(), pos.copy()
            xp[i, c] += h; xm[i, c] -= h
            num[i, c] = -(Q.coulomb_energy(xp, box, types_, q, k, rc, mask, excluded) - Q.coulomb_energy(xm, box, types_, q, k, rc, mask, excluded)) / (2 * h)
    assert np.abs(num - F).max() < 1e-7 * np.abs(F).max()
    assert np.abs(F.sum(0)).max() < 1e-12 * np.abs(F).max()
    assert w == pytest.approx(e, rel=1e-13)                       # U ~ 1/r: r . F = U pair by pair


def test_reference_mask_exclusions_and_cutoff():
    box = np.array([10.0, 10.0, 10.0])
    pos = np.array([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [9.5, 1.0, 1.0], [1.0, 4.0, 1.0]])
    types_, q = np.array([0, 1, 0, 1]), np.array([1.0, -2.0, 0.5, 1.0])
    F, e, w = Q.coulomb_sums(pos, box, types_, q, 2.0, 1.5, {(0, 1), (0, 0)})
    # pairs inside 1.5: (0,1) r = 1, (0,2) r = 1.5 through the boundary (inclusive), (1,2) r = 2.5 out, (., 3) r >= 3 out
    assert e == pytest.approx(2.0 * (1.0 * -2.0 / 1.0 + 1.0 * 0.5 / 1.5))
    # particle 0 is pulled towards 1 at +x (opposite charges) and pushed away from the image of 2 at x = -0.5 (like charges)
    assert F[0] == pytest.approx([2.0 * 2.0 / 1.0 + 2.0 * 0.5 * 1.5 / 1.5 ** 3, 0.0, 0.0])
    assert Q.coulomb_sums(pos, box, types_, q, 2.0, 1.5, {(0, 0)})[1] == pytest.approx(2.0 * 0.5 / 1.5)
    assert Q.coulomb_sums(pos, box, types_, q, 2.0, 1.5, {(0, 1), (0, 0)}, excluded=[(0, 1)])[1] == pytest.approx(2.0 * 0.5 / 1.5)
    assert Q.coulomb_sums(pos, box, types_, q, 2.0, 1.4999, {(0, 1), (0, 0)})[1] == pytest.approx(-4.0)


# ---- 2: the shim -------------------------------------------------------------------------------------------------------------

class StubEngine:
    """records the set-up calls the shim makes"""

    def __init__(self):
        self.calls = []
        self.n = 0

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
        return espp.System()
    finally:
        espp.set_engine_factory(old)


def test_shim_objects_reach_the_engine():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    pot = espp.interaction.CoulombTruncated(prefactor=K_QQ * 0.5, cutoff=0.9)
    assert (pot.prefactor, pot.cutoff) == (K_QQ * 0.5, 0.9)
    inter = espp.interaction.VerletListCoulombTruncated(types.SimpleNamespace(system=system))
    inter.setPotential(type1=2, type2=0, potential=pot)
    inter.setPotential(1, 1, pot)
    assert [c for c in eng.calls if c[0] == "nb_coulomb"] == [("nb_coulomb", (2, 0, K_QQ * 0.5, 0.9), {}), ("nb_coulomb", (1, 1, K_QQ * 0.5, 0.9), {})]
    assert inter.getPotential(0, 2) is pot
    # storage.modifyParticle(pid, 'q', v) reaches the engine as a charge; getParticle reads the charge back
    storage = types.SimpleNamespace(system=system)
    espp.storage.DomainDecomposition.modifyParticle(storage, 7, "q", -0.5)
    assert eng.calls[-1] == ("modify_particle", (7, "CHARGE", -0.5), {})
    # the energy row of the driver: PotentialEnergy of the interaction asks the engine for the Coulomb energy
    eng.get_coulomb = lambda: (-12.5, 3.0)
    assert espp.analysis.PotentialEnergy(system, inter).compute() == -12.5


def test_cpu_checker_refuses_the_term(make_oracle):
    from chemlab_amd import espp
    o = make_oracle()
    with pytest.raises(NotImplementedError, match="Coulomb"):
        o.nb_coulomb(0, 0, K_QQ, 0.9)
    with pytest.raises(NotImplementedError, match="Coulomb"):
        o.get_coulomb()
    inter = espp.interaction.VerletListCoulombTruncated(types.SimpleNamespace(system=types.SimpleNamespace(engine=o)))
    with pytest.raises(NotImplementedError, match="Coulomb"):
        inter.setPotential(0, 0, espp.interaction.CoulombTruncated(prefactor=K_QQ, cutoff=0.9))


# ---- 3: the driver's set-up ---------------------------------------------------------------------------------------------------

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


def read_top(tmp_path, fudge="0.5", qa="0.500", qb="-0.500", pairs=""):
    from chemlab_amd.chemlab import gromacs_topology
    f = tmp_path / "topol.top"
    f.write_text(TOP % dict(fudge=fudge, qa=qa, qb=qb, pairs=pairs))
    return gromacs_topology.GromacsTopology(str(f)).read()


def nonbonded(tmp_path, qq_cutoff, **kw):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    gt = read_top(tmp_path, **kw)
    eng = StubEngine()
    system = shim_system(eng)
    log = []
    gromacs_topology.set_nonbonded_interactions(espp, system, gt, types.SimpleNamespace(system=system), 1.2, qq_cutoff=qq_cutoff, log=log.append)
    return gt, system, [c for c in eng.calls if c[0] == "nb_coulomb"], [c for c in eng.calls if c[0] != "nb_coulomb"], log


def test_driver_registers_every_used_type_pair(tmp_path):
    gt, system, qq, other, log = nonbonded(tmp_path, 0.9)
    assert gt.atoms[1]["charge"] == 0.5 and gt.atoms[2]["charge"] == -0.5
    ids = sorted(gt.used_atomsym_atomtype.values())
    assert ids == [0, 1, 2]
    want = [(a, b) for i, a in enumerate(ids) for b in ids[i:]]
    assert [c[1][:2] for c in qq] == want                                   # C-C and A-C too: no LJ there (sigma = 0), Coulomb all the same
    assert all(c[1][2] == pytest.approx(K_QQ * 0.5, rel=1e-15) and c[1][3] == 0.9 for c in qq)
    names = [system.getNameOfInteraction(k) for k in range(system.getNumberOfInteractions())]
    assert names == ["coulomb", "lj"] and not log
    # without the term the remaining calls are the same, one for one
    _, system0, qq0, other0, _ = nonbonded(tmp_path, 0.0)
    assert qq0 == [] and other0 == other
    assert [system0.getNameOfInteraction(k) for k in range(system0.getNumberOfInteractions())] == ["lj"]


@pytest.mark.parametrize("kw, cutoff, says", [(dict(qa="0.000", qb="0.000"), 0.9, True), (dict(fudge="0.0"), 0.9, False), (dict(), 0.0, False)])
def test_driver_registers_nothing_when_the_term_is_zero(tmp_path, kw, cutoff, says):
    _, system, qq, _, log = nonbonded(tmp_path, cutoff, **kw)
    assert qq == []
    assert [system.getNameOfInteraction(k) for k in range(system.getNumberOfInteractions())] == ["lj"]
    assert bool(log) == says and (not says or "not registered" in log[0])


def test_charged_atom_type_alone_keeps_the_term(tmp_path):
    """a reaction product takes its charge from its atom type: a charged type that no atom has yet still counts"""
    from chemlab_amd.chemlab import gromacs_topology
    gt = read_top(tmp_path, qa="0.000", qb="0.000")
    assert not gromacs_topology.has_charges(gt)
    gt.gt.atomtypes["C"]["charge"] = -1.0
    assert gromacs_topology.has_charges(gt)


def test_one_four_coulomb_pairs_are_refused(tmp_path):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    pairs = "\n[ pairs ]\n1 3 1 0.5 1.0\n"
    system = shim_system(StubEngine())
    system.storage = types.SimpleNamespace(system=system)
    gt = read_top(tmp_path, pairs=pairs)
    assert list(gt.pairs) == [(1, 3), (4, 6)]
    with pytest.raises(NotImplementedError, match="1-4 Coulomb"):
        gromacs_topology.set_pair_interactions(espp, system, gt, 1.2, qq_cutoff=0.9)
    # a neutral member whose type can change through a reaction, while some atom type is charged, counts as charged
    gt_dyn = read_top(tmp_path, pairs=pairs)
    gt_dyn.pairs.clear(); gt_dyn.pairs[(3, 6)] = ["1", "0.5", "1.0"]
    assert gromacs_topology.set_pair_interactions(espp, system, gt_dyn, 1.2, qq_cutoff=0.9) is not None      # both members neutral and static
    with pytest.raises(NotImplementedError, match="1-4 Coulomb"):
        gromacs_topology.set_pair_interactions(espp, system, gt_dyn, 1.2, dynamic_type_ids={gt_dyn.atoms[3]["type_id"]}, qq_cutoff=0.9)
    # no charged member, no fudgeQQ or no cutoff: the 1-4 LJ pairs are set up as before
    for gt_ok, cut in ((read_top(tmp_path, pairs=pairs, qa="0.000"), 0.9), (read_top(tmp_path, pairs=pairs, fudge="0.0"), 0.9), (gt, 0.0)):
        assert list(gromacs_topology.set_pair_interactions(espp, system, gt_ok, 1.2, qq_cutoff=cut)) == ["lj14_0"]


# ---- 4: the C ABI ------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_new_symbols():
    assert {"chem_nb_coulomb", "chem_get_coulomb"} <= set(_capi.header_symbols())
    hdr = open(os.path.join(os.path.dirname(_capi.HERE), "include", "chem_mi355.h")).read()
    assert "#define CHEM_STATE_CHARGE  12" in hdr and _capi.STATE["CHARGE"] == 12
    assert "nb_coulomb" in _capi.PRODUCT_ONLY and "get_coulomb" in _capi.PRODUCT_ONLY
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("chem_nb_coulomb", "chem_get_coulomb"):
        assert getattr(lib, name) is not None
