"""Heterogeneous pair-potential matrices on the CPU oracle (no GPU).

The GPU parity tests take the scalar oracle as their reference; these pin that reference for the matrices a CG model
brings -- several types with their own LJ parameters, cutoffs and shifts, inactive type pairs, several tables with their
own grids -- against an independent numpy evaluation (all pairs, minimum image, no list), against known answers on the
table clamps, and pin the threaded build (bench.py's cpu_baseline) against the scalar one.
"""
import numpy as np
import pytest

from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import pair_matrix, pair_matrix_spec, pair_reference, sorted_events


@pytest.mark.parametrize("case", range(8))
def test_numpy_reference_matches_scalar_oracle(make_oracle, case):
    """Frozen configurations of a few hundred particles: forces 1e-12 of the largest, epot_lj / epot_tab / virial_nb 1e-12."""
    spec = pair_matrix_spec(case, fixed=True)
    o = make_oracle()
    W.apply(spec, o, thermostat=False)
    o.run(0)
    f, elj, etab, vir = pair_reference(spec)
    assert rel_err(o.get_state("FORCE"), f) < 1e-12, case
    ob = o.observe()
    scale = 1e-12 * max(abs(elj), abs(etab), 1.0)
    assert ob["epot_lj"] == pytest.approx(elj, rel=1e-12, abs=scale), case
    assert ob["epot_tab"] == pytest.approx(etab, rel=1e-12, abs=scale), case
    assert ob["virial_nb"] == pytest.approx(vir, rel=1e-12, abs=1e-12 * max(abs(vir), 1.0)), case


def test_draws_cover_the_matrix_shapes():
    """The GPU sweep's own draws (tests/test_gpu_pair_matrix.py: pair_matrix_spec(case), case 0..23) reach what the kernels
    branch on: type id 15, two-row tables, tables ending before the pair cutoff, several distinct tables in one draw,
    inactive pairs, the engine's all_active path (every pair of type ids 0..max active), shifts on and off, both uniform
    degenerations."""
    seen = set()
    for case in range(24):
        s = pair_matrix_spec(case)
        ids = s["type_ids"]
        act = {(a, b) for (a, b, *_) in s["lj"]} | {(t[0], t[1]) for t in s["tables"]}
        npairs = len(ids) * (len(ids) + 1) // 2
        seen.add("t15" if 15 in ids else "no15")
        if len(act) < npairs:
            seen.add("inactive")
        elif ids == list(range(max(ids) + 1)):
            seen.add("engine_all_active")
        for t in s["tables"]:
            if len(t[4]) == 2:
                seen.add("nrow2")
            if t[2] + (len(t[4]) - 1) * t[3] < t[6]:
                seen.add("ends_early")
        if len({id(t[4]) for t in s["tables"]}) > 1:
            seen.add("several_tables")
        shifts = {bool(l[5]) for l in s["lj"]}
        if len({l[2:5] for l in s["lj"]}) == 1 and len(s["lj"]) > 1:
            seen.add("uniform_lj+table" if s["tables"] else "uniform_lj")
        if len(shifts) == 2:
            seen.add("shift_on_off")
        assert all(1.5 <= l[4] <= s["rc"] for l in s["lj"]) and all(1.5 <= t[6] <= s["rc"] for t in s["tables"])
    assert seen >= {"t15", "engine_all_active", "inactive", "nrow2", "ends_early", "several_tables", "uniform_lj",
                    "uniform_lj+table", "shift_on_off"}, seen


def _known_answer_system():
    """Isolated pairs (5 apart, box 40): a table (r0 = 0.5, dr = 0.1, six rows, pair cutoff 1.4) on (0,0), LJ on (0,1)
    without shift, nothing on (1,1)."""
    r0, dr = 0.5, 0.1
    e = np.array([4.0, 3.0, 2.5, 1.25, 0.5, 0.25])
    f = np.array([9.0, 7.0, 5.5, 3.25, 1.5, 0.75])
    placed = [(0, 0, 0.8), (0, 0, 0.3), (0, 0, 1.2), (0, 0, 1.45), (0, 1, 1.1), (1, 1, 1.0), (0, 0, 0.65)]
    pos, types = [], []
    for k, (ta, tb, r) in enumerate(placed):
        c = np.array([5.0 + 5.0 * (k % 6), 5.0 + 5.0 * (k // 6), 20.0])
        pos += [c, c + [r, 0.0, 0.0]]
        types += [ta, tb]
    n = len(pos)
    spec = dict(n=n, box=[40.0] * 3, rc=2.0, skin=0.3, dt=0.005, ids=np.arange(1, n + 1), types=np.array(types, np.int32),
                pos=np.array(pos), mass=np.ones(n), lj=[(0, 1, 1.3, 0.9, 1.8, False)], tables=[(0, 0, r0, dr, e, f, 1.4)])
    # the known answers: force on the first particle of each pair along -x (F_i = f(r) (x_i - x_j) / r), energy
    s6 = (0.9 / 1.1) ** 6
    want = [(f[3], e[3]), (f[0], e[0]), (f[5], e[5]), (0.0, 0.0), (24.0 * 1.3 * (2 * s6 * s6 - s6) / 1.1, 4.0 * 1.3 * (s6 * s6 - s6)),
            (0.0, 0.0), (0.5 * (f[1] + f[2]), 0.5 * (e[1] + e[2]))]
    return spec, want


def test_known_answer_pairs_on_grid_points_and_clamps(make_oracle):
    """Pairs exactly on a grid point, below r0 (row 0), between the last row and the pair cutoff (last row), beyond the
    cutoff (nothing), half-way between rows, an LJ pair and an inactive pair -- oracle and numpy reference both."""
    spec, want = _known_answer_system()
    o = make_oracle()
    W.apply(spec, o, thermostat=False)
    o.run(0)
    fo = o.get_state("FORCE")
    fr, elj, etab, vir = pair_reference(spec)
    for k, (fw, ew) in enumerate(want):
        for f in (fo, fr):
            assert f[2 * k][0] == pytest.approx(-fw, rel=1e-12, abs=1e-12), k
            assert f[2 * k + 1][0] == pytest.approx(fw, rel=1e-12, abs=1e-12), k
            assert np.abs(f[2 * k][1:]).max() < 1e-12
    ob = o.observe()
    e_tab = sum(w[1] for k, w in enumerate(want) if k != 4)
    for got in (ob["epot_tab"], etab):
        assert got == pytest.approx(e_tab, rel=1e-12)
    for got in (ob["epot_lj"], elj):
        assert got == pytest.approx(want[4][1], rel=1e-12)
    rs = [0.8, 0.3, 1.2, 1.45, 1.1, 1.0, 0.65]
    assert ob["virial_nb"] == pytest.approx(sum(w[0] * r for w, r in zip(want, rs)), rel=1e-12)
    assert vir == pytest.approx(ob["virial_nb"], rel=1e-12)


def _reactive_matrix(case):
    """The chain-growth melt (types A, B, D) under a random matrix over those three types, with reactions."""
    rng = np.random.default_rng(41000 + case)
    spec = W.reactive_melt(n=int(rng.choice([16 ** 3, 4 * 10 ** 3])), seed=800 + case, interval=int(rng.integers(4, 9)),
                           rc=float(rng.choice([2.2, 2.5])))
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e9
    spec["lj"], spec["tables"] = pair_matrix(rng, [0, 1, 2], spec["rc"], kind=["mixed", "all_active", "uniform_table"][case % 3])
    spec["rebuild_criterion"] = int(rng.integers(0, 2))
    return spec


@pytest.mark.parametrize("case", range(3))
def test_threaded_oracle_matches_scalar(make_oracle, case):
    """OracleEngine(threads=4) -- the list built over cells in parallel, forces into per-thread arrays, e_lj / e_tab split by
    pair kind in a reduction -- against the scalar oracle: forces 1e-13, event log and rebuild count identical, both energy
    terms the same."""
    from oracle.oracle import OracleEngine
    spec = _reactive_matrix(case)
    try:
        t = OracleEngine(threads=4)
    except Exception as e:      # noqa: BLE001
        pytest.fail("threaded oracle unavailable: %s" % e)
    s = make_oracle()
    try:
        W.apply(spec, t); W.apply(spec, s)
        t.run(0); s.run(0)
        assert rel_err(t.get_state("FORCE"), s.get_state("FORCE")) < 1e-13
        iv = spec["reaction"]["interval"]
        for _ in range(4):
            t.run(iv); s.run(iv)
        et, es = sorted_events(t.get_events()), sorted_events(s.get_events())
        assert len(es) > 0 and [e[:4] for e in et] == [e[:4] for e in es]
        assert t.timers()["rebuilds"] == s.timers()["rebuilds"]
        assert np.array_equal(t.get_state("TYPE"), s.get_state("TYPE"))
        assert rel_err(t.get_state("POS_UNFOLDED"), s.get_state("POS_UNFOLDED")) < 1e-12
        t.run(0); s.run(0)
        assert rel_err(t.get_state("FORCE"), s.get_state("FORCE")) < 1e-11
        ot, os_ = t.observe(), s.observe()
        for k in ("epot_lj", "epot_tab", "virial_nb"):
            assert ot[k] == pytest.approx(os_[k], rel=1e-11, abs=1e-11), k
        assert (ot["epot_tab"] != 0.0) == bool(spec["tables"])
    finally:
        t.close()


def test_pair_cutoff_beyond_the_list_cutoff_is_refused(make_oracle):
    """A pair cutoff above max_cutoff is refused at run(), naming the type pair; at max_cutoff it runs."""
    spec = pair_matrix_spec(2, n=256, fixed=True)
    spec["lj"] = [(0, 0, 1.0, 1.0, spec["rc"])]
    spec["types"] = np.where(np.arange(spec["n"]) % 2, 3, 0).astype(np.int32)
    spec["tables"] = []
    o = make_oracle()
    W.apply(spec, o, thermostat=False)
    o.nb_lj(0, 3, 1.0, 1.0, spec["rc"] + 0.05, True)
    with pytest.raises(ChemError) as ex:
        o.run(0)
    assert ex.value.code == _capi.EINVAL and "(0,3)" in str(ex.value)
    e, f = np.zeros(4), np.zeros(4)
    o.nb_lj(0, 3, 1.0, 1.0, spec["rc"], True)
    o.nb_table(3, 3, 0.1, 0.1, e, f, spec["rc"] + 0.5)
    with pytest.raises(ChemError) as ex:
        o.run(0)
    assert ex.value.code == _capi.EINVAL and "(3,3)" in str(ex.value)
    o.nb_lj(3, 3, 0.0, 0.0, spec["rc"] + 1.0, True)       # an inactive pair (sigma = 0) carries no cutoff
    o.run(0)
