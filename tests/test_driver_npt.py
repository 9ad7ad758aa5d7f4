"""The driver (python -m chemlab_amd.start_simulation) with pressure coupling: --pressure / --barostat / --barostat_tau and
--store_pressure (reference start_simulation.py:356-376, 466-469) on the fixture tests/golden/chain_growth_catalytic.

CPU: the refusal of the Langevin barostat, the shim classes, and the two columns --store_pressure adds, on the CPU checker wrapped
so that the calls it does not have (pressure, box) are recorded instead of refused -- what is checked is the driver's own wiring.
GPU: the same fixture with the Berendsen barostat on the product engine."""
import os
import shutil

import numpy as np
import pytest

from chemlab_amd import espp, start_simulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BAR = 0.060221374


def product_factory(prec=32):
    from chemlab_amd.engine import Engine
    return lambda: Engine(device=0, precision=prec)


def stage(tmp_path):
    d = tmp_path / "chain_growth_catalytic"
    shutil.copytree(os.path.join(GOLD, "chain_growth_catalytic"), str(d))
    return d


def test_langevin_barostat_is_refused_by_name(tmp_path, monkeypatch):
    monkeypatch.chdir(stage(tmp_path))
    with pytest.raises(NotImplementedError, match=r"LangevinBarostat.*--barostat br"):
        start_simulation.main(["@params", "--pressure=1.0"], quiet=True)                 # lv is the default of --barostat
    with pytest.raises(NotImplementedError, match=r"LangevinBarostat.*--barostat br"):
        start_simulation.main(["@params", "--pressure=1.0", "--barostat=lv"], quiet=True)
    with pytest.raises(NotImplementedError):
        espp.integrator.LangevinBarostat(None, None, 1.0)


def test_shim_classes_construct(oracle_mod):
    espp.set_engine_factory(lambda: oracle_mod.OracleEngine())
    try:
        system = espp.System()
        system.rng = espp.esutil.RNG(1)
        system.bc = espp.bc.OrthorhombicBC(system.rng, (4.0, 5.0, 6.0))
        system.storage = espp.storage.DomainDecomposition(system, None, None)
        integrator = espp.integrator.VelocityVerlet(system)
        p = espp.analysis.Pressure(system)
        L = espp.analysis.BoxSize(system)
        b = espp.integrator.BerendsenBarostat(system, p)
        b.tau, b.pressure = 2.5, 3.0 * BAR
        assert (b.tau, b.pressure) == (2.5, 3.0 * BAR)
        assert L.compute() == 4.0 and list(system.bc.boxL) == [4.0, 5.0, 6.0]      # the x edge; the checker's box is the one it was given
        with pytest.raises(NotImplementedError, match="Pressure: the CPU checker has no"):
            p.compute()
        with pytest.raises(NotImplementedError, match="BerendsenBarostat: the CPU checker has no barostat"):
            integrator.addExtension(b)
    finally:
        espp.set_engine_factory(product_factory())


def test_store_pressure_adds_the_two_columns(tmp_path, monkeypatch, oracle_mod):
    rec = []

    class Recording(oracle_mod.OracleEngine):
        """the CPU checker, with the entry points it lacks recorded instead of refused"""

        def pressure(self):
            rec.append("pressure")
            return dict(pressure=0.25)

        def box(self):
            rec.append("box")
            return np.array([7.0, 8.0, 9.0])

    espp.set_engine_factory(lambda: Recording())
    try:
        monkeypatch.chdir(stage(tmp_path))
        start_simulation.main(["@params", "--run=1000", "--start_ar=500", "--store_pressure=True"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    lines = [l.strip().split(",") for l in open("sim0_energy_12345.csv")]
    header = lines[0]
    assert header.index("P") == header.index("Ekin") + 1 and header.index("L") == header.index("Ekin") + 2
    assert all(float(r[header.index("P")]) == 0.25 and float(r[header.index("L")]) == 7.0 for r in lines[1:]) and len(lines) > 1
    assert "pressure" in rec and "box" in rec


def test_without_store_pressure_the_columns_are_absent(tmp_path, monkeypatch, oracle_mod):
    espp.set_engine_factory(lambda: oracle_mod.OracleEngine())
    try:
        monkeypatch.chdir(stage(tmp_path))
        start_simulation.main(["@params", "--run=500", "--start_ar=500"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    header = open("sim0_energy_12345.csv").readline().strip().split(",")
    assert "P" not in header and "L" not in header


@pytest.mark.gpu
def test_driver_runs_the_berendsen_barostat_on_the_gpu(tmp_path, monkeypatch):
    espp.set_engine_factory(product_factory(32))
    try:
        monkeypatch.chdir(stage(tmp_path))
        res = start_simulation.main(["@params", "--run=1000", "--start_ar=500", "--pressure", "1.0", "--barostat", "br", "--barostat_tau", "1.0"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    eng = res["system"].engine
    lines = [l.strip().split(",") for l in open("sim0_energy_12345.csv")]
    header = lines[0]
    assert header.index("P") == header.index("Ekin") + 1 and header.index("L") == header.index("Ekin") + 2
    Lcol = np.array([float(r[header.index("L")]) for r in lines[1:]])
    Pcol = np.array([float(r[header.index("P")]) for r in lines[1:]])
    print("L:", Lcol, "P:", Pcol)
    assert len(Lcol) >= 2 and np.isfinite(Lcol).all() and np.isfinite(Pcol).all()
    assert len(set(Lcol.tolist())) > 1                                              # L moves
    box = eng.box()
    assert box[0] == pytest.approx(Lcol[-1], rel=1e-5)                              # (%g keeps six digits)
    conf = [l for l in open("sim0_12345_confout.gro").read().split("\n") if l.strip()]
    assert conf[-1] == "%f %f %f" % tuple(box)
    assert list(res["system"].bc.boxL) == list(box)
