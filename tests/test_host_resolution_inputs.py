"""Dynamic resolution through the Python layers, against an engine that records calls: the espressopp-shaped shim objects
(VerletListDynamicResolution*, BasicDynamicResolution, lambda_adr of particles and of reaction post-processes, store_lambda), the
topology reader's nonbond_params func 11 / func 15, the reaction parser's dissociation equation and its set-up.  No GPU."""
import os
import types

import numpy as np
import pytest

from test_host_coulomb import StubEngine, shim_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def calls(eng, name):
    return [c[1:] for c in eng.calls if c[0] == name]


# ---- the shim ------------------------------------------------------------------------------------------------------------------

def test_scaled_interactions_reach_the_engine():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    vl = types.SimpleNamespace(system=system)
    lj = espp.interaction.VerletListDynamicResolutionLennardJones(vl, False)
    pot = espp.interaction.LennardJones(epsilon=0.8, sigma=0.6, cutoff=1.4)
    lj.setPotential(type1=2, type2=0, potential=pot)
    assert calls(eng, "nb_lj") == [((2, 0, 0.8, 0.6, 1.4, pot.shift == "auto"), {})]
    assert calls(eng, "nb_resolution") == [((2, 0, True, 0.0), {})]          # no cap until setMaxForce
    lj.setPotential(1, 1, pot)
    lj.setMaxForce(25.0)
    assert calls(eng, "nb_resolution")[2:] == [((0, 2, True, 25.0), {}), ((1, 1, True, 25.0), {})]
    assert lj.getPotential(0, 2) is pot
    eng.observe = lambda: dict(epot_lj=-3.5, epot_tab=1.25)
    assert espp.analysis.PotentialEnergy(system, lj).compute() == -3.5
    tab = espp.interaction.VerletListDynamicResolutionTabulated(vl)
    tpot = espp.interaction.Tabulated(itype=1, filename=os.path.join(GOLD, "table_nb_excerpt.pot"), cutoff=1.2)
    tab.setMaxForce(7.0)
    tab.setPotential(0, 1, tpot)
    assert calls(eng, "nb_table")[0][0][:2] == (0, 1) and calls(eng, "nb_resolution")[-1] == ((0, 1, True, 7.0), {})
    assert espp.analysis.PotentialEnergy(system, tab).compute() == 1.25
    for cls in (espp.interaction.VerletListDynamicResolutionLennardJones, espp.interaction.VerletListDynamicResolutionTabulated):
        with pytest.raises(NotImplementedError, match="cg_potential"):
            cls(vl, True)
        with pytest.raises(NotImplementedError, match="cg_potential"):
            cls(vl, cg_potential=True)


def test_basic_dynamic_resolution_registers_rates_and_changes():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    bdr = espp.integrator.BasicDynamicResolution(system, {3: 1e-3, 1: 1e-3})
    tpp = espp.integrator.TopologyParticleProperties(type=4, mass=12.5, lambda_adr=1.0, q=-0.25)
    bdr.add_postprocess(espp.integrator.PostProcessChangeProperty(3, tpp))
    assert calls(eng, "resolution_rate") == []                                # nothing before the extension is added
    espp.integrator.VelocityVerlet(system).addExtension(bdr)
    assert calls(eng, "resolution_rate") == [((1, 1e-3), {}), ((3, 1e-3), dict(new_type=4, new_mass=12.5, new_q=-0.25, new_state=-1))]
    bdr.disconnect()
    assert calls(eng, "resolution_rate")[2:] == [((1, 0.0), {}), ((3, 0.0), {})]
    with pytest.raises(NotImplementedError):
        bdr.add_postprocess(espp.integrator.PostProcessChangeNeighboursProperty(None))


def test_particle_lambda_through_the_storage():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    system.bc = types.SimpleNamespace(boxL=espp.Real3D(4.0, 4.0, 4.0))
    st = espp.storage.DomainDecomposition(system)
    props = ["id", "type", "pos", "mass", "q", "res_id", "state", "lambda_adr"]
    st.addParticles([[1, 0, espp.Real3D(0, 0, 0), 1.0, 0.0, 1, 0, 1.0], [2, 1, espp.Real3D(1, 1, 1), 1.0, 0.0, 1, 0, 0.25]], *props)
    st.decompose()
    (ids, lam), _ = calls(eng, "set_resolution")[0]
    assert ids.tolist() == [1, 2] and lam.tolist() == [1.0, 0.25]
    assert [c[0] for c in eng.calls].index("set_particles") < [c[0] for c in eng.calls].index("set_resolution")
    st.modifyParticle(2, "lambda_adr", 0.5)
    assert eng.calls[-1] == ("modify_particle", (2, "LAMBDA", 0.5), {})
    # all ones: the column is accepted and nothing is sent
    eng2 = StubEngine()
    system2 = shim_system(eng2)
    system2.bc = system.bc
    st2 = espp.storage.DomainDecomposition(system2)
    st2.addParticles([[1, 0, espp.Real3D(0, 0, 0), 1.0, 0.0, 1, 0, 1.0]], *props)
    st2.decompose()
    assert calls(eng2, "set_resolution") == []
    # getParticle reads it back; the trajectory writer stores the real values
    class Eng(StubEngine):
        api = types.SimpleNamespace(nb_coulomb=1, set_resolution=1)
        step = 0

        def get_state(self, what):
            return {"LAMBDA": np.array([1.0, 0.5]), "ID": np.array([1, 2]), "POS": np.zeros((2, 3)), "VEL": np.zeros((2, 3)), "FORCE": np.zeros((2, 3)),
                    "IMAGE": np.zeros((2, 3), np.int32)}.get(what, np.zeros(2))
    eng3 = Eng()
    system3 = shim_system(eng3)
    system3.bc = system.bc
    storage = types.SimpleNamespace(system=system3, _ids=np.array([1, 2]))
    assert espp.storage.DomainDecomposition.getParticle(storage, 2).lambda_adr == 0.5
    for flag, present in ((True, True), (False, False)):
        d = espp.io.DumpH5MD(system3, "x.h5", store_lambda=flag, is_single_prec=False)
        d.dump(0, 0.0)
        key = "particles/atoms/lambda_adr/value"
        assert (key in d.tree()) == present
        if present:
            assert d.tree()[key].tolist() == [[1.0, 0.5]]


# ---- nonbond_params func 11 / func 15 --------------------------------------------------------------------------------------------

TOP = """[ defaults ]
1 2 no 1.0 1.0

[ atomtypes ]
A 1.0 0.000 A 0.5 1.0
B 1.0 0.000 A 0.4 0.5
C 1.0 0.000 A 0.3 0.25
D 1.0 0.000 A 0.0 0.0

[ nonbond_params ]
A A 15 0.6 0.8
A B 15 0.55 0.7 40.0
A C 15 40.0
B B 11 table_nb_excerpt.xvg
B C 11 table_nb_excerpt.xvg 12.5
C C 1 0.35 0.3

[ moleculetype ]
MOL 1

[ atoms ]
1 A 1 MOL A1 1 0.000 1.0
2 B 1 MOL B1 1 0.000 1.0
3 C 1 MOL C1 1 0.000 1.0
4 D 1 MOL D1 1 0.000 1.0

[ system ]
X

[ molecules ]
MOL 2
"""


def test_func_11_and_15_rows_become_scaled_interactions(tmp_path):
    import shutil
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    for ext in ("xvg", "pot"):
        shutil.copy(os.path.join(GOLD, "table_nb_excerpt." + ext), tmp_path / ("table_nb_excerpt." + ext))
    f = tmp_path / "topol.top"
    f.write_text(TOP)
    gt = gromacs_topology.GromacsTopology(str(f)).read()
    eng = StubEngine()
    system = shim_system(eng)
    gromacs_topology.set_nonbonded_interactions(espp, system, gt, types.SimpleNamespace(system=system), 1.2, tab_cutoff=1.1, table_dir=str(tmp_path))
    t = gt.used_atomsym_atomtype
    A, B, C = t["A"], t["B"], t["C"]
    names = [system.getNameOfInteraction(k) for k in range(system.getNumberOfInteractions())]
    assert names == ["tab-dynamic_0", "tab-dynamic_1", "lj-dynamic_0", "lj-dynamic_1", "lj"]      # grouped by max_force, as the reference groups them
    lj = {c[0][:2]: c[0][2:5] for c in calls(eng, "nb_lj")}
    assert lj[(A, A)] == (0.8, 0.6, 1.2) and lj[(A, B)] == (0.7, 0.55, 1.2) and lj[(C, C)] == (0.3, 0.35, 1.2)
    assert lj[(A, C)] == pytest.approx((0.5, 0.4, 1.2))                       # max_force alone: sigma, epsilon from the atom types (rule 2: mean, geometric mean)
    assert {c[0][:2] for c in calls(eng, "nb_table")} == {(B, B), (B, C)} and all(c[0][6] == 1.1 for c in calls(eng, "nb_table"))
    last = {}
    for (a, b, on, cap), _ in calls(eng, "nb_resolution"):
        assert on is True
        last[(min(a, b), max(a, b))] = cap
    assert last == {(A, A): 0.0, (A, B): 40.0, (A, C): 40.0, (B, B): 0.0, (B, C): 12.5}      # C-C (func 1) is not marked
    assert system.getInteraction(names.index("lj-dynamic_1")).max_force == 40.0 and set(system.getInteraction(names.index("lj-dynamic_1")).getAllPotentials()) == {(A, B), (A, C)}


# ---- the dissociation equation -------------------------------------------------------------------------------------------------

def test_parser_reads_the_dissociation_equation():
    from chemlab_amd.chemlab import reaction_parser
    sec = {"reaction": "C(0,3):E(1,2) -> A(-1) + E(1)", "rate": "1", "cutoff": "0.9", "group": "g", "alpha": "1e-5", "diss_rate": "0.25", "min_cutoff": "0.1", "active": "False"}
    g, d = reaction_parser.process_reaction(sec)
    assert g == "g" and d["reaction_type"] == reaction_parser.REACTION_DISSOCIATION
    assert d["reactant_list"]["type_1"] == {"name": "C", "min": "0", "max": "3", "delta": "-1", "new_type": "A"}
    assert d["reactant_list"]["type_2"] == {"name": "E", "min": "1", "max": "2", "delta": "1", "new_type": "E"}
    assert (d["alpha"], d["diss_rate"], d["min_cutoff"], d["cutoff"], d["active"]) == (1e-5, 0.25, 0.1, 0.9, False)
    no_alpha = {k: v for k, v in sec.items() if k != "alpha"}
    with pytest.raises(NotImplementedError, match="`alpha` is required"):
        reaction_parser.process_reaction(no_alpha)
    with pytest.raises(NotImplementedError, match="smooth reaction cutoff"):
        reaction_parser.process_reaction(dict(sec, sigma="0.1", eq_distance="0.5"))


def test_a_dissociation_section_with_alpha_yields_the_call_sequence(tmp_path):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import reaction_parser, reaction_setup
    cfg = tmp_path / "r.cfg"
    cfg.write_text("[general]\ninterval = 10\nnearest = 1\n\n[group_g]\npotential = Harmonic\npotential_options = K=30.0,r0=0.5\n\n"
                   "[reaction_a]\nreaction = A(0,2) + B(0,2) -> A(1):B(1)\nrate = 0.5\ncutoff = 0.6\ngroup = g\n\n"
                   "[reaction_d]\nreaction = A(1,3):B(1,3) -> C(-1) + B(-1)\nrate = 0.0\ncutoff = 0.9\ndiss_rate = 0.125\nalpha = 0.0625\ngroup = g\n")
    rc = reaction_parser.parse_config(str(cfg))
    eng = StubEngine()
    system = shim_system(eng)
    system.rng = None
    system.storage = types.SimpleNamespace(system=system, decompose=lambda: None)
    integrator = espp.integrator.VelocityVerlet(system)
    # stand-in indices for what the recording engine cannot return
    eng.reaction_add = lambda *a, **k: (eng.calls.append(("reaction_add", a, k)), 0)[1]
    eng.dissociation_add = lambda *a, **k: (eng.calls.append(("dissociation_add", a, k)), 1)[1]
    atomtypes = {"A": dict(mass=1.0, charge=0.0), "B": dict(mass=2.0, charge=0.0), "C": dict(mass=3.5, charge=-0.5)}
    topol = types.SimpleNamespace(used_atomsym_atomtype={"A": 0, "B": 1, "C": 2}, gt=types.SimpleNamespace(atomtypes=atomtypes))
    sc = reaction_setup.SetupReactions(espp, system, types.SimpleNamespace(system=system), topol, None, rc)
    ar, fpls = sc.setup_reactions()
    assert sc.dynamic_types == {0, 1, 2} and len(sc.extensions_to_integrator) == 1
    integrator.addExtension(ar)
    for ext in sc.extensions_to_integrator:
        integrator.addExtension(ext)
    (args, kw), = calls(eng, "dissociation_add")
    assert args[:9] == (0, 1, -1, -1, 1, 3, 1, 3, 0.125) and args[9] == 0.9
    assert "new_type_1" not in kw and "new_type_2" not in kw               # on the break both keep their type ...
    assert calls(eng, "reaction_set_resolution") == [((1, 1, 0.0), {}), ((1, 2, 0.0), {})]      # ... and get lambda = 0
    assert calls(eng, "resolution_rate") == [((0, 0.0625), dict(new_type=2, new_mass=3.5, new_q=-0.5, new_state=-1)), ((1, 0.0625), {})]
    names = [c[0] for c in eng.calls]
    assert names.index("dissociation_add") < names.index("reaction_set_resolution") < names.index("reactions_enable") < names.index("resolution_rate")
