"""g(r) through the driver's hook route (hooks.py: hook_before_sim / hook_end, INTEGRATION.md "Radial distribution functions")
on the shipped fixture tests/golden/mf_espp_cg_1: a hooks.py file in the working directory, as INTEGRATION.md shows it, which the
driver finds itself; analysis.RadialDistrF starts the in-run sampling behind the set-up, the end hook writes the text file.

CPU: on the CPU checker wrapped so that the rdf_* calls it does not have are recorded instead of refused -- the wiring.
GPU: the same run on the product engine; the file holds the g(r) the engine accumulated over the run's twenty frames."""
import os
import shutil

import numpy as np
import pytest

from chemlab_amd import engine as E
from chemlab_amd import espp, start_simulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ARGS = ["@params", "--run=2000", "--start_ar=1000", "--int_step=500", "--energy_collect=500", "--trj_collect=1000", "--rng_seed=7"]


def product_factory(prec=32):
    from chemlab_amd.engine import Engine
    return lambda: Engine(device=0, precision=prec)


def stage(tmp_path):
    d = tmp_path / "mf_espp_cg_1"
    shutil.copytree(os.path.join(GOLD, "mf_espp_cg_1"), str(d))
    return d


# the hooks.py of INTEGRATION.md, written into the working directory, where the driver finds it
HOOKS_PY = '''from chemlab_amd.chemlab import outputs

def hook_before_sim(system, integrator, ar, gt):     # behind the whole set-up, in front of the first integrator.run
    system.rdf = espressopp.analysis.RadialDistrF(system)
    system.rdf.start(nbins=150, types=[(-1, -1), (0, 0)], every=100, split_molecules=True)      # r_max: max_cutoff

def hook_end(system, integrator, ar, gt, args):
    outputs.write_rdf("%s_rdf.dat" % args.output_prefix, system.rdf.result(), labels=["all", "A-A"])
'''


def stage_with_hooks(tmp_path):
    d = stage(tmp_path)
    (d / "hooks.py").write_text(HOOKS_PY)
    return d


def test_integration_md_shows_this_hooks_file():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for line in HOOKS_PY.strip().split("\n"):
        assert line.strip() in text, line


def test_hooks_start_the_sampling_before_the_first_step_and_write_the_file(tmp_path, monkeypatch, oracle_mod):
    rec = []

    class Recording(oracle_mod.OracleEngine):
        """the CPU checker, with the entry points it lacks recorded instead of refused"""

        def supports(self, name):
            return name == "rdf" or oracle_mod.OracleEngine.supports(self, name)

        def rdf_init(self, *a):
            rec.append(("rdf_init", a, self.step))

        def rdf_sample_every(self, every):
            rec.append(("rdf_sample_every", every, self.step))

        def run(self, n):
            rec.append(("run", n))
            return oracle_mod.OracleEngine.run(self, n)

        def rdf(self):
            rec.append(("rdf", self.step))
            return E.rdf_result(1.5, np.ones((2, 2, 150), np.uint64), 20, [7, 3], [0.5, 0.25])

    espp.set_engine_factory(lambda: Recording())
    try:
        monkeypatch.chdir(stage_with_hooks(tmp_path))
        res = start_simulation.main(ARGS, quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    rc = res["system"].max_cutoff
    assert rec[0] == ("rdf_init", (rc, 150, [(-1, -1), (0, 0)], True), 0) and rec[1] == ("rdf_sample_every", 100, 0)
    assert [r for r in rec if r[0] == "run" and r[1] > 0] and rec[-1] == ("rdf", 2000)
    lines = open("sim0_rdf.dat").read().split("\n")
    assert lines[0].startswith("# r g_all_intra g_all_inter g_A-A_intra g_A-A_inter") and len(lines) == 152


@pytest.mark.gpu
def test_driver_writes_g_of_r_for_the_mf_example(tmp_path, monkeypatch):
    espp.set_engine_factory(product_factory(32))
    try:
        monkeypatch.chdir(stage_with_hooks(tmp_path))
        res = start_simulation.main(ARGS, quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    got = res["system"].engine.rdf()
    assert got["frames"] == 20 and got["counts"].shape == (2, 2, 150) and got["r_max"] == res["system"].max_cutoff
    rows = np.array([[float(v) for v in l.split()] for l in open("sim0_rdf.dat").read().split("\n")[1:] if l])
    assert rows.shape == (150, 5) and np.allclose(rows[:, 1:], got["g"].reshape(4, 150).T, rtol=1e-7)
    # (the fixture starts from single-bead molecules: the intramolecular column holds what the few reactions of the run bonded)
    assert rows[:, 2].max() > 0.5 and (rows[:, 1] >= 0).all() and np.isfinite(rows).all() and got["counts"][0, 1].sum() > 10000
