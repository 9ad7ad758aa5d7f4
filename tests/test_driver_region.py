"""The driver (python -m chemlab_amd.start_simulation) on the fixture tests/golden/freeze: a reaction .cfg whose group carries
`ext_type=FreezeRegion` (all six faces, static width, prob) and `ext_type=ChangeParticleType`, a topology with the types A, B, C
and the coordinates of 216 particles.  The fixture holds settings and coordinates only.

CPU: the whole driver runs on the CPU checker, wrapped so that the region calls (which the checker does not have) are
recorded instead of refused -- what is checked is the driver's own wiring: the six regions for both width types, the
FREEZE_<id> type, the enable at k_enable_reactions, the stats file, ChangeParticleType's rule, and every refusal.
GPU: the same run on the product engine; the driver's outputs agree with the engine's logs."""
import os
import shutil

import numpy as np
import pytest

from chemlab_amd import _capi, espp, start_simulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BOX, N = 6.6, 216
A, B, C, FREEZE = 0, 1, 2, 3
FACES = ["-x", "x", "-y", "y", "-z", "z"]


def stage(tmp_path, edit_cfg=None, edit_top=None):
    d = tmp_path / "freeze"
    shutil.copytree(os.path.join(GOLD, "freeze"), str(d))
    if edit_cfg:
        (d / "reaction.cfg").write_text(edit_cfg((d / "reaction.cfg").read_text()))
    if edit_top:
        (d / "topol.top").write_text(edit_top((d / "topol.top").read_text()))
    return d


def product_factory(prec=32):
    from chemlab_amd.engine import Engine
    return lambda: Engine(device=0, precision=prec)


def slab(face, width):
    axis, lo, hi = "xyz".index(face[-1]), [0.0] * 3, [BOX] * 3
    if face.startswith("-"):
        hi[axis] = width[axis]
    else:
        lo[axis] = BOX - width[axis]
    return lo, hi


def recording(oracle_mod, rec):
    class Recording(oracle_mod.OracleEngine):
        """the CPU checker, with the region entry points recorded instead of refused (no rule acts)"""

        def supports(self, name):
            return name == "region" or super().supports(name)

        def region_add(self, lo, hi, target_type, new_type, **k):
            rec.append(("region_add", [float(v) for v in lo], [float(v) for v in hi], target_type, new_type, k, self.step))
            return sum(1 for r in rec if r[0] == "region_add") - 1

        def region_enable(self, rule, on=True):
            rec.append(("region_enable", rule, on, self.step))

        def region_stats(self):
            dt = np.dtype([("step", "i8"), ("rule", "i8"), ("candidates", "i8"), ("changed", "i8")])
            return np.array([(20, 0, 4, 2), (20, 3, 2, 1), (40, 6, 9, 3), (50, 5, 1, 1)], dtype=dt)

    return Recording


def run_recorded(tmp_path, monkeypatch, oracle_mod, edit_cfg=None, edit_top=None):
    rec = []
    espp.set_engine_factory(lambda: recording(oracle_mod, rec)())
    try:
        monkeypatch.chdir(stage(tmp_path, edit_cfg, edit_top))
        res = start_simulation.main(["@params"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    return rec, res


def test_fixture_holds_settings_and_coordinates_only():
    assert sorted(os.listdir(os.path.join(GOLD, "freeze"))) == ["conf.gro", "params", "reaction.cfg", "topol.top"]


@pytest.mark.parametrize("width_type", ["static", "ratio"])
def test_driver_wires_the_regions_on_the_cpu_checker(tmp_path, monkeypatch, oracle_mod, width_type):
    edit = None if width_type == "static" else (lambda t: t.replace("width=0.75\nwidth_type=static", "width=0.125\nwidth_type=ratio"))
    rec, res = run_recorded(tmp_path, monkeypatch, oracle_mod, edit)
    eng = res["system"].engine
    assert eng.n == N and eng.step == 100
    width = [0.75] * 3 if width_type == "static" else [0.125 * BOX] * 3
    adds = [r for r in rec if r[0] == "region_add"]
    assert len(adds) == 7
    # the six slabs in the order of `directions` (default: all six), every one of them a rule of its own: B -> FREEZE_3 on
    # every step, by probability, both resets, mass and charge kept, the run's seed
    for face, r in zip(FACES, adds[:6]):
        lo, hi = slab(face, width)
        assert np.allclose(r[1], lo, rtol=0, atol=1e-12) and np.allclose(r[2], hi, rtol=0, atol=1e-12)
        assert (r[3], r[4]) == (B, FREEZE)
        k = r[5]
        assert k["interval"] == 1 and k["mode"] == "prob" and k["value"] == 0.5 and k["reset_velocity"] and k["reset_force"]
        assert "new_mass" not in k and k["seed"] == 12345
    # ChangeParticleType: the whole box, by count, every 20 steps, nothing reset, properties kept
    r = adds[6]
    assert r[1] == [0.0] * 3 and np.allclose(r[2], [BOX] * 3) and (r[3], r[4]) == (C, B)
    assert r[5]["interval"] == 20 and r[5]["mode"] == "num" and r[5]["num"] == 3 and not r[5].get("reset_velocity") and "new_mass" not in r[5]
    # sent and enabled when the driver adds the integrator extensions: at k_enable_reactions (start_ar = 10 steps), not before
    assert all(a[6] == 10 for a in adds)
    assert [(r[1], r[2], r[3]) for r in rec if r[0] == "region_enable"] == [(k, True, 10) for k in range(7)]
    # the stats file: the rows of the six region rules (not ChangeParticleType's), written at the end of the run
    rows = open("sim0_12345_freeze_stats.dat").read().splitlines()
    assert rows[0].startswith("#") and rows[1:] == ["20 0 4 2", "20 3 2 1", "50 5 1 1"]


def test_options_of_the_section(tmp_path, monkeypatch, oracle_mod):
    edit = lambda t: t.replace("prob=0.5", "directions=-x,z\np_num=4\nstats_file=sinks.dat")
    rec, res = run_recorded(tmp_path, monkeypatch, oracle_mod, edit)
    adds = [r for r in rec if r[0] == "region_add"]
    assert len(adds) == 3 and [(a[1], a[2]) for a in adds[:2]] == [slab("-x", [0.75] * 3), slab("z", [0.75] * 3)]
    assert all(a[5]["mode"] == "num" and a[5]["num"] == 4 for a in adds[:2])
    assert open("sinks.dat").read().splitlines()[1:] == ["20 0 4 2"]
    edit = lambda t: t.replace("prob=0.5", "p_percentage=0.25")
    rec, res = run_recorded(tmp_path / "pct", monkeypatch, oracle_mod, edit)
    assert all(a[5]["mode"] == "fraction" and a[5]["value"] == 0.25 for a in rec if a[0] == "region_add" and a[4] == FREEZE)
    edit = lambda t: t.replace("prob=0.5\n", "")
    rec, res = run_recorded(tmp_path / "all", monkeypatch, oracle_mod, edit)
    assert all(a[5]["mode"] == "all" for a in rec if a[0] == "region_add" and a[4] == FREEZE)


def test_refusals(tmp_path, monkeypatch, oracle_mod):
    rec = []
    cases = [
        (lambda t: t.replace("prob=0.5", "prob=0.5\nremove_particles=True"), None, NotImplementedError, "remove_particles"),
        (lambda t: t.replace("prob=0.5", "p_percentage=1.5"), None, RuntimeError, "p_percentage"),
        (lambda t: t.replace("prob=0.5", "directions=-x,w"), None, RuntimeError, "direction"),
        # thirteen more types in the topology: FREEZE would get id 16 = CHEM_MAX_TYPES
        (None, lambda t: t.replace("[ atomtypes ]\n", "[ atomtypes ]\n" + "".join("  T%d  T%d   1.0   0.0   A   0.5   0.5\n" % (k, k) for k in range(13))),
         RuntimeError, "CHEM_MAX_TYPES"),
    ]
    espp.set_engine_factory(lambda: recording(oracle_mod, rec)())
    try:
        for k, (ecfg, etop, exc, says) in enumerate(cases):
            monkeypatch.chdir(stage(tmp_path / ("case%d" % k), ecfg, etop))
            with pytest.raises(exc, match=says):
                start_simulation.main(["@params"], quiet=True)
        with pytest.raises(NotImplementedError, match="remove_particle"):
            espp.integrator.ChangeInRegion(type("S", (), {})(), espp.ParticleRegion(None, None, [0] * 3, [1] * 3)).set_flags(1, True, True, remove_particle=True)
    finally:
        espp.set_engine_factory(product_factory())
    assert _capi.CHEM_MAX_TYPES == 16
    # the CPU checker itself: asked first, the answer names the extension
    espp.set_engine_factory(lambda: oracle_mod.OracleEngine())
    try:
        for k, (edit, says) in enumerate(((None, "FreezeRegion"), (lambda t: t.replace("extensions=sink,convert", "extensions=convert"), "ChangeParticleType"))):
            monkeypatch.chdir(stage(tmp_path / ("cpu%d" % k), edit))
            with pytest.raises(NotImplementedError, match=says):
                start_simulation.main(["@params"], quiet=True)
        e = oracle_mod.OracleEngine()
        with pytest.raises(NotImplementedError, match="the CPU checker has no region rules"):
            e.region_add([0] * 3, [1] * 3, 0, 1)
        assert not e.supports("region")
        e.close()
    finally:
        espp.set_engine_factory(product_factory())


@pytest.mark.gpu
def test_driver_run_on_the_gpu(tmp_path, monkeypatch):
    espp.set_engine_factory(product_factory(64))
    try:
        monkeypatch.chdir(stage(tmp_path))
        res = start_simulation.main(["@params"], quiet=True)
    finally:
        espp.set_engine_factory(product_factory())
    eng = res["system"].engine
    assert eng.n == N and eng.step == 100
    ch, st, ty = eng.region_changes(), eng.region_stats(), eng.get_state("TYPE")
    print("%d changes in %d firings that changed something" % (len(ch), len(st)))
    frozen, conv = ch[ch["rule"] < 6], ch[ch["rule"] == 6]
    assert len(frozen) > 20 and ch["step"].min() >= 11      # on from step 10: the first firing is at step 11
    # ChangeParticleType: three C per 20 steps, from the first multiple of 20 behind the enable on
    assert sorted(set(conv["step"].tolist())) == [20, 40, 60, 80, 100] and len(conv) == 15
    # final types: every frozen particle is FREEZE_3 (nothing brings one back), every converted one B or frozen later
    assert (ty[frozen["id"] - 1] == FREEZE).all() and len(set(frozen["id"].tolist())) == len(frozen)
    assert np.isin(ty[conv["id"] - 1], [B, FREEZE]).all()
    assert (ty == FREEZE).sum() == len(frozen) and (ty == C).sum() == 72 - 15 and (ty == A).sum() == 72
    # the stats: one row per firing of a rule that changed something, consistent with the changes; the file holds the six sinks
    for s in st:
        assert s["changed"] == ((ch["step"] == s["step"]) & (ch["rule"] == s["rule"])).sum() and s["candidates"] >= s["changed"] > 0
    assert st["changed"].sum() == len(ch)
    rows = [tuple(int(v) for v in l.split()) for l in open("sim0_12345_freeze_stats.dat").read().splitlines()[1:]]
    assert rows == [(int(s["step"]), int(s["rule"]), int(s["candidates"]), int(s["changed"])) for s in st if s["rule"] < 6]
    # the frozen particles were caught inside a slab and B or C before
    assert np.isfinite(eng.get_state("VEL")).all()
