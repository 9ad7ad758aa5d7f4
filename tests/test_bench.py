"""bench.py's command line: what a plain run prints, what --full adds, and the arrays of --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from chemlab_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "late_stage", "f64", "cpu_baseline")


def _reacted_oracle(oracle_mod, n=4000, steps=12):
    spec = W.reactive_melt(n=n, seed=21, interval=5)
    o = oracle_mod.OracleEngine()
    h = W.apply(spec, o)
    o.run(steps)
    return o, h


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_the_state_after_the_last_step(tmp_path, oracle_mod):
    import bench
    o, h = _reacted_oracle(oracle_mod)
    for precision, fdt in ((64, np.float64), (32, np.float32)):
        d = str(tmp_path / str(precision))
        bench.dump_outputs(d, o, h, precision)
        got = _load(d)
        assert sorted(got) == ["bonds", "force", "ids", "pos_unfolded", "state", "type", "vel"]
        assert np.array_equal(got["ids"], o.get_state("ID").astype(np.float64))
        for name, what in (("pos_unfolded", "POS_UNFOLDED"), ("vel", "VEL"), ("force", "FORCE")):
            assert got[name].dtype == fdt and got[name].shape == (o.n, 3)
            assert np.array_equal(got[name], o.get_state(what).astype(fdt))
        assert np.array_equal(got["type"], o.get_state("TYPE").astype(np.float32))
        assert np.array_equal(got["state"], o.get_state("STATE").astype(np.float32))
        b = np.sort(o.get_list(h["reaction_bonds"]), axis=1)
        assert len(b) > 0 and got["bonds"].dtype == np.float64
        assert np.array_equal(got["bonds"], b[np.lexsort((b[:, 1], b[:, 0]))].astype(np.float64))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) < 64e6
    o.close()


def test_dump_outputs_over_budget_writes_a_fixed_seeded_sample(tmp_path, oracle_mod):
    import bench
    o, h = _reacted_oracle(oracle_mod)
    per_particle = 8 + 9 * 4 + 8
    first = None
    for k in range(2):
        d = str(tmp_path / str(k))
        bench.dump_outputs(d, o, h, 32, particle_bytes=1000 * per_particle, bond_bytes=16 * 50)
        got = _load(d)
        assert all(len(got[x]) == 1000 for x in ("ids", "pos_unfolded", "vel", "force", "type", "state"))
        ids = got["ids"].astype(np.int64)
        assert np.all(np.diff(ids) > 0)
        rows = np.searchsorted(o.get_state("ID"), ids)
        assert np.array_equal(got["force"], o.get_state("FORCE")[rows].astype(np.float32))
        assert 0 < len(got["bonds"]) <= 50 and np.isin(got["bonds"][:, 0], ids).all()
        if first is None:
            first = got
        else:
            assert all(np.array_equal(first[x], got[x]) for x in first)
    o.close()


def _bench(tmp_path, *args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                         capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


SMALL = ["--particles", "32000", "--equil", "50", "--interval", "20"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """A plain run: EXACTLY --steps timed steps, the headline fields, none of the --full legs; --dump-outputs writes the
    per-particle state of the single-domain engine (32000 particles: no sampling) and the same inputs every time.  The timed
    steps 53-97 hold the reaction steps 60 and 80: the first one only changes states (virtual reactions), the second bonds."""
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("out%d" % k))
        r = _bench(tmp_path, "--steps", "45", "--warmup", "3", "--dump-outputs", d, *SMALL)
        assert all(key in r for key in HEADLINE) and not any(key in r for key in FULL_ONLY)
        assert r["steps"] == 45 and r["ms_per_step"] > 0 and r["dtype"] == "f32"
        assert abs(r["value"] * r["ms_per_step"] - 1e3) < 1e-6 * 1e3
        got = _load(d)
        assert got["ids"].shape == (32000,) and got["pos_unfolded"].dtype == np.float32
        assert np.isfinite(got["force"]).all() and len(got["bonds"]) > 0
        dumps.append(got)
    # the same seeded inputs in both runs: the same particles and, over 98 steps, the same trajectory up to fp32 summation order
    assert np.array_equal(dumps[0]["ids"], dumps[1]["ids"])
    assert np.abs(dumps[0]["pos_unfolded"] - dumps[1]["pos_unfolded"]).max() < 1e-2


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs(tmp_path):
    r = _bench(tmp_path, "--full", "--steps", "40", "--warmup", "2", "--f64-steps", "5", "--cpu-steps", "2", "--late-stage", "1", *SMALL)
    assert all(key in r for key in HEADLINE + FULL_ONLY)
    assert r["steps"] == 40 and r["f64"]["steps"] == 5 and r["cpu_baseline"]["value"] > 0
    assert "reaction_step_ms" in r["config"] and "msd_after_melting" in r["config"]
