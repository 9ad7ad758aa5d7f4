"""Capped pair potentials through the Python layers, against an engine that records calls: the topology reader's
nonbond_params func 13 (`table caprad` -> VerletListTabulatedCapped under the label lj-tab_cap) and func 16 (refused, with its
reason), the shim's capped interactions, the workload key `caps` and the CPU checker's refusal.  No GPU."""
import os
import shutil
import types

import numpy as np
import pytest

from test_host_coulomb import StubEngine, shim_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def calls(eng, name):
    return [c[1:] for c in eng.calls if c[0] == name]


TOP = """[ defaults ]
1 2 no 1.0 1.0

[ atomtypes ]
A 1.0 0.000 A 0.5 1.0
D 1.0 0.000 A 0.4 0.5
E 1.0 0.000 A 0.3 0.25
C 1.0 0.000 A 0.45 0.6

[ nonbond_params ]
A D 13 table_nb_excerpt.xvg 0.29
A E 13 table_a5_excerpt.xvg 0.31
D D 8 table_nb_excerpt.xvg
C C 1 0.35 0.3

[ moleculetype ]
MOL 1

[ atoms ]
1 A 1 MOL A1 1 0.000 1.0
2 D 1 MOL D1 1 0.000 1.0
3 E 1 MOL E1 1 0.000 1.0
4 C 1 MOL C1 1 0.000 1.0

[ system ]
X

[ molecules ]
MOL 2
"""


def read(tmp_path, text):
    from chemlab_amd import espp
    from chemlab_amd.chemlab import gromacs_topology
    for name in ("table_nb_excerpt", "table_a5_excerpt"):
        for ext in ("xvg", "pot"):
            shutil.copy(os.path.join(GOLD, name + "." + ext), tmp_path / (name + "." + ext))
    f = tmp_path / "topol.top"
    f.write_text(text)
    gt = gromacs_topology.GromacsTopology(str(f)).read()
    eng = StubEngine()
    system = shim_system(eng)
    gromacs_topology.set_nonbonded_interactions(espp, system, gt, types.SimpleNamespace(system=system), 1.2, tab_cutoff=1.1, table_dir=str(tmp_path))
    return gt, eng, system


def test_func_13_rows_become_one_capped_tabulated_interaction(tmp_path):
    from chemlab_amd import espp
    gt, eng, system = read(tmp_path, TOP)
    t = gt.used_atomsym_atomtype
    A, D, E = t["A"], t["D"], t["E"]
    names = [system.getNameOfInteraction(k) for k in range(system.getNumberOfInteractions())]
    assert names == ["lj", "lj-tab", "lj-tab_cap"]                          # after lj-tab, as the reference adds it
    inter = system.getInteraction(names.index("lj-tab_cap"))
    assert type(inter) is espp.interaction.VerletListTabulatedCapped
    pots = inter.getAllPotentials()
    assert set(pots) == {(min(A, D), max(A, D)), (min(A, E), max(A, E))}
    pad, pae = inter.getPotential(A, D), inter.getPotential(A, E)
    assert (pad.caprad, pad.cutoff, pad.itype, os.path.basename(pad.filename)) == (0.29, 1.1, 1, "table_nb_excerpt.pot")
    assert (pae.caprad, pae.cutoff, pae.itype, os.path.basename(pae.filename)) == (0.31, 1.1, 1, "table_a5_excerpt.pot")
    # the engine gets the table, then its cap; the plain table pair (func 8) gets none
    caps = {(min(c[0][0], c[0][1]), max(c[0][0], c[0][1])): c[0][2] for c in calls(eng, "nb_cap")}
    assert caps == {(min(A, D), max(A, D)): 0.29, (min(A, E), max(A, E)): 0.31}
    seq = [(c[0], min(c[1][0], c[1][1]), max(c[1][0], c[1][1])) for c in eng.calls if c[0] in ("nb_table", "nb_cap")]
    for pair in caps:
        assert seq.index(("nb_table",) + pair) < seq.index(("nb_cap",) + pair)
    assert ("nb_table", t["D"], t["D"]) in seq and ("nb_cap", t["D"], t["D"]) not in seq
    assert set(system.getInteraction(names.index("lj-tab")).getAllPotentials()) == {(t["D"], t["D"])}
    # the shared accumulator
    eng.observe = lambda: dict(epot_lj=-3.5, epot_tab=1.25)
    assert inter.computeEnergy() == 1.25 and espp.analysis.PotentialEnergy(system, inter).compute() == 1.25


@pytest.mark.parametrize("row", ["A D 13 table_nb_excerpt.xvg", "A D 13 table_nb_excerpt.xvg 0.29 7.0", "A D 13"])
def test_func_13_wants_two_parameters(tmp_path, row):
    with pytest.raises(RuntimeError, match=r"A D func 13: expected `table caprad`, got %d parameters" % (len(row.split()) - 3)):
        read(tmp_path, TOP.replace("A D 13 table_nb_excerpt.xvg 0.29", row))


def test_func_16_is_refused_with_its_reason(tmp_path):
    with pytest.raises(NotImplementedError, match=r"C C func 16: LennardJonesEnergyCapped is not built") as ei:
        read(tmp_path, TOP.replace("C C 1 0.35 0.3", "C C 16 0.35 0.3 0.2"))
    assert "inside the cap radius" in str(ei.value)
    from chemlab_amd import espp
    for name in ("LennardJonesEnergyCapped", "VerletListLennardJonesEnergyCapped"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(espp.interaction, name)()


def test_the_shim_sends_the_potential_and_then_the_cap():
    from chemlab_amd import espp
    eng = StubEngine()
    system = shim_system(eng)
    vl = types.SimpleNamespace(system=system)
    ljc = espp.interaction.VerletListLennardJonesCapped(vl)
    pot = espp.interaction.LennardJonesCapped(0.8, 0.6, 1.4, 0.55, "auto")          # epsilon, sigma, cutoff, caprad, shift
    assert (pot.epsilon, pot.sigma, pot.cutoff, pot.caprad, pot.shift) == (0.8, 0.6, 1.4, 0.55, "auto")
    ljc.setPotential(type1=2, type2=0, potential=pot)
    assert calls(eng, "nb_lj") == [((2, 0, 0.8, 0.6, 1.4, True), {})] and calls(eng, "nb_cap") == [((2, 0, 0.55), {})]
    assert [c[0] for c in eng.calls if c[0] in ("nb_lj", "nb_cap")] == ["nb_lj", "nb_cap"]
    assert ljc.getPotential(0, 2) is pot
    for itype in (1, 2, 3):
        tc = espp.interaction.VerletListTabulatedCapped(vl)
        tp = espp.interaction.TabulatedCapped(itype, os.path.join(GOLD, "table_nb_excerpt.pot"), 1.2, 0.3)      # itype, filename, cutoff, caprad
        tc.setPotential(1, 1, tp)
        (a, kw) = calls(eng, "nb_table")[-1]
        assert a[:2] == (1, 1) and a[6] == 1.2 and kw == ({} if itype == 1 else {"itype": itype})
        assert calls(eng, "nb_cap")[-1] == ((1, 1, 0.3), {})
    with pytest.raises(NotImplementedError):
        espp.interaction.TabulatedCapped(4, os.path.join(GOLD, "table_nb_excerpt.pot"), 1.2, 0.3)
    # a capped LJ interaction next to a plain one: both report the one LJ accumulator
    lj = espp.interaction.VerletListLennardJones(vl)
    eng.observe = lambda: dict(epot_lj=-3.5, epot_tab=1.25)
    assert ljc.computeEnergy() == -3.5 == espp.analysis.PotentialEnergy(system, lj).compute() == espp.analysis.PotentialEnergy(system, ljc).compute()
    assert tc.computeEnergy() == 1.25


def test_workload_key_and_the_cpu_checker(oracle_mod):
    from chemlab_amd import workloads as W
    eng = StubEngine()
    n = 8
    spec = dict(box=[6.0] * 3, rc=1.5, skin=0.3, dt=0.002, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32), pos=np.zeros((n, 3)), mass=np.ones(n),
                lj=[(0, 0, 1.0, 0.5, 1.3)], caps=[(0, 0, 0.7)], gamma=0.0)
    W.apply(spec, eng, thermostat=False, reactions=False)
    order = [c[0] for c in eng.calls if c[0] in ("nb_lj", "nb_cap")]
    assert order == ["nb_lj", "nb_cap"] and calls(eng, "nb_cap") == [((0, 0, 0.7), {})]
    o = oracle_mod.OracleEngine()
    try:
        with pytest.raises(NotImplementedError, match="capped pair potentials: the CPU checker has no cap radius"):
            o.nb_cap(0, 0, 0.7)
    finally:
        o.close()
