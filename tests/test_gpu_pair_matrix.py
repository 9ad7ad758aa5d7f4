"""Heterogeneous pair-potential matrices on the HIP path against the CPU oracle (seeded: every case reproducible).

Every other GPU test runs one LJ parameter set (MODE 2 of the tile force kernel) or one table on type pair (0,0).  These
draw what a CG model brings -- up to 16 types (type id 15 included) with their own LJ parameters, cutoffs and shifts,
inactive type pairs, several tables on their own grids -- and change the potential while a run goes on: reactions and
ATRP turning a type into one with other parameters, modify_particle between runs (single domain and slabs), tables and
LJ sets swapped between runs (MODE 2 -> 0 -> 2), the MixedTabulated table of the espressopp shim re-sent as the conversion
moves.  Oracle semantics: tests/test_oracle_pair_matrix.py pins the oracle on these matrices.
"""
import numpy as np
import pytest

from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import energy_scales, force_error_without_cutoff_flips, pair_matrix, pair_matrix_spec, smooth_table, sorted_events
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks
from test_gpu_sweep import _apply_opts, _refused

pytestmark = pytest.mark.gpu


def _draw(case):
    spec = pair_matrix_spec(case)
    rng = np.random.default_rng(32000 + case)
    spec["rebuild_criterion"] = int(rng.integers(0, 2))
    opts = {}
    if rng.random() < 0.45 and spec["box"][0] / (spec["rc"] + spec["skin"]) >= 5.5:      # >= 5 cells in x and y
        opts["dd_self"] = 1
    if rng.random() < 0.25:
        opts["fused_rebuild"] = 0
    if rng.random() < 0.15 and "dd_self" not in opts:        # (the slab path needs the LDS tiles)
        opts["tiles"] = 0
    if rng.random() < 0.35:
        opts["list_skin"] = spec["skin"] + float(rng.uniform(0.0, 0.3))
    if rng.random() < 0.25:
        opts["skip_inactive_pairs"] = 0
    if rng.random() < 0.4:
        opts["tpp"] = int(rng.choice([1, 2, 4, 8]))
    prec = 64 if rng.random() < 0.6 else 32
    return spec, opts, prec, int(rng.integers(30, 61))


def _energy_ok(a, b, prec, scale=(0.0, 0.0)):
    """fp64 1e-10; fp32 2e-5, or 2e-6 of the sum of the terms' magnitudes (a sum that cancels) plus what pairs on their
    cutoff may contribute -- scale = helpers.energy_scales(spec)[term]."""
    if prec == 64:
        return a == pytest.approx(b, rel=1e-10, abs=1e-12 * scale[0])
    return a == pytest.approx(b, rel=2e-5, abs=2e-6 * scale[0] + scale[1])


@pytest.mark.parametrize("case", range(24))
def test_random_pair_matrix_matches_oracle(make_gpu, make_oracle, case):
    """Forces and the two energy terms at step 0, then a Langevin run: trajectory and rebuild count of the oracle."""
    spec, opts, prec, nsteps = _draw(case)
    g, o = make_gpu(prec), make_oracle()
    _apply_opts(g, opts)
    try:
        W.apply(spec, g, thermostat=False)
        g.run(0)
    except Exception as e:      # noqa: BLE001
        _refused(e, case, opts)
    W.apply(spec, o, thermostat=False)
    o.run(0)
    fg, fo = g.get_state("FORCE"), o.get_state("FORCE")
    if prec == 64:
        assert rel_err(fg, fo) < TOL[64], (case, opts)
    else:
        err, flips = force_error_without_cutoff_flips(spec, fg, fo, TOL_MELT32, max_flips=8)
        assert err < TOL_MELT32 and 0 <= flips <= 8, (case, opts, err, flips)
    og, oo = g.observe(), o.observe()
    sc = energy_scales(spec)
    for k in ("epot_lj", "epot_tab", "virial_nb"):
        assert _energy_ok(og[k], oo[k], prec, sc[k]), (case, opts, k, og[k], oo[k], sc[k])
    for e in (g, o):
        e.thermostat_langevin(spec["kT"], spec["gamma"], spec["seed"])
    g.run(nsteps); o.run(nsteps)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-8 if prec == 64 else 2e-4), (case, opts)
    if prec == 64 and "list_skin" not in opts:
        tg, to = g.timers(), o.timers()
        assert to["rebuilds"] <= tg["rebuilds"] <= to["rebuilds"] + 4, (case, opts, tg["rebuilds"], to["rebuilds"])


# ---- type changes that change the potential ------------------------------------------------------------------------

def _table(rc, seed):
    e, f = smooth_table(np.random.default_rng(seed), 0.005, 0.005, int(rc / 0.005) + 1, rc)
    return (0.005, 0.005, e, f, rc)


def _separated_melt(n=8788, seed=61, interval=6):
    """The chain-growth melt with a matrix that tells B from D: A-B inactive, A-D active (reaction a, B -> D, adds list
    pairs; reaction d, D -> B, removes them), B-B LJ, D-D a table."""
    A, B, D = 0, 1, 2
    spec = W.reactive_melt(n=n, seed=seed, interval=interval)
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e9
    rc = spec["rc"]
    spec["lj"] = [(A, A, 1.0, 1.0, rc), (B, B, 1.4, 0.95, 2.1, False), (A, D, 0.7, 1.05, 2.0), (B, D, 1.1, 1.0, rc)]
    spec["tables"] = [(D, D) + _table(2.2, 5)]
    spec["rebuild_criterion"] = 0
    return spec


def _agree(eg, eo, tg, to, prec):
    """Event logs (sorted_events) and types of the two sides.  fp64: bit for bit.  fp32: the reactive sweep's rule
    (test_gpu_sweep.py) -- a candidate whose distance sits on the reaction radius may fall to the other side, so the logs
    agree but for a handful of events, and no more particles carry another type than such events explain.  Returns the
    number of differing events."""
    if prec == 64:
        assert [e[:4] for e in eg] == [e[:4] for e in eo]
        assert np.array_equal(tg, to)
        return 0
    sg, so = set(e[:4] for e in eg), set(e[:4] for e in eo)
    nd = len(sg ^ so)
    assert nd <= max(4, len(so) // 100), (nd, len(so))
    assert int((np.asarray(tg) != np.asarray(to)).sum()) <= nd
    return nd


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("path", ["single", "dd_self"])
def test_reaction_type_changes_switch_the_potential(make_gpu, make_oracle, prec, path):
    """B <-> D by reactions a and d under a matrix that separates the two: events bit for bit (fp64), trajectory after every
    interval and one step past every reaction step, types, forces."""
    spec = _separated_melt()
    g, o = make_gpu(prec), make_oracle()
    if path == "dd_self":
        g.set_option("dd_self", 1)
    W.apply(spec, g); W.apply(spec, o)
    iv = spec["reaction"]["interval"]
    ntypes0 = int((spec["types"] == 2).sum())
    for k in range(5):
        for e in (g, o):
            e.run(iv)
        for e in (g, o):
            e.run(1)                                       # the step right after the reaction step
        _agree(sorted_events(g.get_events()), sorted_events(o.get_events()), g.get_state("TYPE"), o.get_state("TYPE"), prec)
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-8 if prec == 64 else 2e-4), (k, path)
        for e in (g, o):
            e.run(iv - 1)
    assert {e[3] for e in sorted_events(o.get_events())} >= {0, 3}, "reactions a and d both fired"
    assert int((o.get_state("TYPE") == 2).sum()) != ntypes0


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("P", [2, 3])
def test_reaction_type_changes_on_slabs(make_gpu, make_oracle, P, prec):
    """The same on 2 and 3 in-process slabs: k_react_apply rewrites x4.w of home particles, the ghost copies must follow."""
    spec = _separated_melt(n=16384, seed=62)
    iv = spec["reaction"]["interval"]
    o = make_oracle()
    W.apply(spec, o)
    ref = []
    for _ in range(4):
        o.run(iv); o.run(1)
        ref.append((o.get_state("POS_UNFOLDED"), o.get_state("TYPE"), sorted_events(o.get_events())))
        o.run(iv - 1)
    engs = [make_gpu(prec) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        W.apply(spec, g)
        res = []
        for _ in range(4):
            g.run(iv); g.run(1)
            res.append((g.get_state("POS_UNFOLDED"), g.get_state("TYPE"), sorted_events(g.get_events())))
            g.run(iv - 1)
        return res
    out = _run_ranks(P, rank)
    assert {e[3] for e in sorted_events(o.get_events())} >= {0, 3}
    for r in range(P):
        for k, ((xg, tg, eg), (xo, to, eo)) in enumerate(zip(out[r], ref)):
            _agree(eg, eo, tg, to, prec)
            assert rel_err(xg, xo) < (1e-8 if prec == 64 else 2e-4), (r, k)


def test_atrp_new_type_with_its_own_parameters(make_gpu, make_oracle):
    """ATRPActivator activating into a type (3) whose pair parameters differ from the dormant type's."""
    rng = np.random.default_rng(17)
    spec = W.reactive_melt(n=16 ** 3, rho=0.8, seed=603, interval=9)
    spec["state"] = np.where(spec["types"] == 0, 0, 1).astype(np.int32)
    rc = spec["rc"]
    spec["lj"], spec["tables"] = pair_matrix(rng, [0, 1, 2, 3], rc, kind="mixed")
    spec["lj"] = [l for l in spec["lj"] if 3 not in l[:2]] + [(3, 3, 1.6, 0.9, 2.2), (0, 3, 0.5, 1.08, rc), (1, 3, 1.2, 1.0, 2.0)]
    spec["tables"] = [t for t in spec["tables"] if 3 not in t[:2]] + [(2, 3) + _table(2.0, 9)]
    spec["reaction"]["type_mass"][3] = 1.0
    spec["atrp"] = dict(interval=5, num_particles=600, ratio_activator=0.6, ratio_deactivator=0.4, delta_catalyst=0.2, k_activate=0.8,
                        k_deactivate=0.5, select_from_all=True, seed=11,
                        centers=[dict(type_id=0, state=0, is_activator=False, new_type=3, new_mass=1.0, delta_state=1),
                                 dict(type_id=3, state=1, is_activator=True, new_type=0, new_mass=1.0, delta_state=-1)])
    g, o = make_gpu(64), make_oracle()
    W.apply(spec, g); W.apply(spec, o)
    for _ in range(4):
        g.run(12); o.run(12)
        assert np.array_equal(g.get_state("TYPE"), o.get_state("TYPE"))
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    assert g.atrp_stats() == o.atrp_stats()
    assert int((o.get_state("TYPE") == 3).sum()) > 0
    assert [e[:4] for e in sorted_events(g.get_events())] == [e[:4] for e in sorted_events(o.get_events())]


# ---- inline bonds under a non-uniform matrix -----------------------------------------------------------------------

def _remapped_melt(table):
    """The chain-growth melt with A, B, D renumbered 3, 5, 15 (type pair (3, 0) differs from the bonded pair (3, 3)) under a
    non-uniform matrix: LJ only (MODE 1) or with the bonded pair A-A tabulated (MODE 0).  NVE, so forces compare directly."""
    A, B, D = 3, 5, 15
    spec = W.reactive_melt(n=8788, seed=64, interval=5)
    m = {0: A, 1: B, 2: D}
    spec["types"] = np.vectorize(m.get)(spec["types"]).astype(np.int32)
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e9
        r["type_1"], r["type_2"] = m[r["type_1"]], m[r["type_2"]]
        if r.get("new_type_2", -1) >= 0:
            r["new_type_2"] = m[r["new_type_2"]]
    spec["reaction"]["type_mass"] = {A: 1.0, B: 1.0, D: 1.0}
    rc = spec["rc"]
    spec["lj"] = [(A, A, 1.2, 0.95, rc), (B, B, 0.8, 1.0, 2.2), (D, D, 1.5, 1.05, 2.3), (B, D, 1.0, 1.0, rc, False), (A, D, 0.6, 1.0, 2.0)]
    if table:
        spec["lj"] = spec["lj"][1:]
        spec["tables"] = [(A, A) + _table(2.0, 7)]
    spec["gamma"] = 0.0
    spec["rebuild_criterion"] = 1
    return spec


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("inline", [1, 0])
@pytest.mark.parametrize("table", [False, True])
def test_inline_bonds_under_a_non_uniform_matrix(make_gpu, make_oracle, prec, inline, table):
    """Reaction bonds A-A with the bonded pair's own LJ parameters (MODE 1) or table (MODE 0): the single-domain inline
    bonds add the pair term of bonded partners in the list pass and take it out again through the type-pair matrix."""
    spec = _remapped_melt(table)
    g, o = make_gpu(prec), make_oracle()
    g.set_option("bonds_inline", inline)
    h = W.apply(spec, g); W.apply(spec, o)
    for k in range(4):
        g.run(5); o.run(5)
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-8 if prec == 64 else 2e-4), k
    g.run(0); o.run(0)
    assert len(o.get_list(h["reaction_bonds"])) > 100
    nd = _agree(sorted_events(g.get_events()), sorted_events(o.get_events()), g.get_state("TYPE"), o.get_state("TYPE"), prec)
    if nd == 0:             # (a bond the other side lacks is a force the other side lacks: compared through the trajectory)
        assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (1e-8 if prec == 64 else 5e-4)
        og, oo = g.observe(), o.observe()
        sc = energy_scales(dict(spec, pos=o.get_state("POS"), types=o.get_state("TYPE")))
        for k in ("epot_lj", "epot_tab"):
            assert _energy_ok(og[k], oo[k], prec, sc[k]), k


# ---- modify_particle between runs ----------------------------------------------------------------------------------

def _modify_plan(spec, seed):
    rng = np.random.default_rng(seed)
    pick = rng.choice(spec["n"], size=120, replace=False)
    ids = spec["ids"][pick]
    ti = spec["type_ids"]
    return [(int(i), "TYPE", float(rng.choice(ti))) for i in ids[:80]] + [(int(i), "MASS", float(rng.uniform(0.7, 1.6))) for i in ids[80:]]


def _modify_spec():
    spec = pair_matrix_spec(5, n=16384)
    spec["rebuild_criterion"] = 0
    return spec


@pytest.mark.parametrize("P", [1, 2, 3])
def test_modify_particle_type_between_runs(make_gpu, make_oracle, P):
    """Type and mass changes of particles spread over the box between runs (start_simulation's modifyParticle path): on
    the single domain (P = 1 also through dd_self) and on 2 and 3 in-process slabs, where most of the changed tags are
    neither home nor ghost on a rank.  Trajectory, types and forces of the oracle."""
    spec = _modify_spec()
    plan = _modify_plan(spec, 3)
    o = make_oracle()
    W.apply(spec, o)
    o.run(10)
    for (pid, what, v) in plan:
        o.modify_particle(pid, what, v)
    o.run(15)
    x1, t1 = o.get_state("POS_UNFOLDED"), o.get_state("TYPE")
    for (pid, what, v) in plan[:40]:
        o.modify_particle(pid, what, spec["type_ids"][0])
    o.run(15)
    x2 = o.get_state("POS_UNFOLDED")

    def work(g):
        W.apply(spec, g)
        g.run(10)
        for (pid, what, v) in plan:
            g.modify_particle(pid, what, v)
        g.run(15)
        r = dict(x1=g.get_state("POS_UNFOLDED"), t1=g.get_state("TYPE"))
        for (pid, what, v) in plan[:40]:
            g.modify_particle(pid, what, spec["type_ids"][0])
        g.run(15)
        r["x2"] = g.get_state("POS_UNFOLDED")
        return r
    if P == 1:
        outs = []
        for dd in (0, 1):
            g = make_gpu(64)
            if dd:
                g.set_option("dd_self", 1)
            outs.append(work(g))
    else:
        engs = [make_gpu(64) for _ in range(P)]
        _HUB[0] += 1
        hub = _HUB[0]

        def rank(r):
            engs[r].comm_init_local(P, r, hub)
            return work(engs[r])
        outs = _run_ranks(P, rank)
    assert not np.array_equal(t1, spec["types"])
    for k, r in enumerate(outs):
        assert np.array_equal(r["t1"], t1), k
        assert rel_err(r["x1"], x1) < 1e-8, k
        assert rel_err(r["x2"], x2) < 1e-8, k


# ---- tables and LJ sets swapped in the middle of a run -------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("dd", [0, 1])
def test_table_and_mode_switch_mid_run(make_gpu, make_oracle, prec, dd):
    """Uniform LJ over four types (MODE 2); after k steps a table on one type pair (MODE 0); later that pair back to the
    common LJ set (MODE 2).  The same calls on the oracle; trajectories compared after every leg (rebuild counts are not:
    the HIP path rebuilds when the matrix changes)."""
    spec = pair_matrix_spec(7, n=4 * 16 ** 3)
    ti = spec["type_ids"][:4]
    spec["types"] = np.asarray(ti)[np.arange(spec["n"]) % 4].astype(np.int32)
    rc = spec["rc"]
    spec["lj"] = [(a, b, 1.0, 1.0, rc) for i, a in enumerate(ti) for b in ti[i:]]
    spec["tables"] = []
    spec["type_ids"] = ti
    g, o = make_gpu(prec), make_oracle()
    if dd:
        g.set_option("dd_self", 1)
    W.apply(spec, g); W.apply(spec, o)
    tab = _table(min(rc, 2.2), 11)
    tol = 1e-8 if prec == 64 else 2e-4
    legs = [(12, None), (17, ("tab", ti[1], ti[2])), (11, ("lj", ti[1], ti[2])), (9, ("tab", ti[3], ti[3])), (13, None)]
    for nsteps, change in legs:
        if change is not None:
            for e in (g, o):
                if change[0] == "tab":
                    e.nb_table(change[1], change[2], *tab)
                else:
                    e.nb_lj(change[1], change[2], 1.0, 1.0, rc, True)
        g.run(nsteps); o.run(nsteps)
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < tol, (nsteps, change)
    g.run(0); o.run(0)
    og, oo = g.observe(), o.observe()
    sc = energy_scales(dict(spec, pos=o.get_state("POS"), lj=[l for l in spec["lj"] if l[:2] != (ti[3], ti[3])], tables=[(ti[3], ti[3]) + tab]))
    assert oo["epot_tab"] != 0.0
    for k in ("epot_lj", "epot_tab"):
        assert _energy_ok(og[k], oo[k], prec, sc[k]), k


# ---- MixedTabulated through the espressopp shim ---------------------------------------------------------------------

def _mixed_script(tmp_path, dd, legs=None):
    """test_oracle_extensions' MixedTabulated script on a melt of a few thousand particles: type 0 under the mixed table,
    a pool of type-1 particles whose conversion to type 2 moves the mixture.  Between run() calls pool particles change
    type and the observable is computed, which re-sends the mixed table (chem_nb_table); the second move comes right
    after a step that rebuilt the list.  legs: steps before each move (None: found on this engine -- the second leg runs
    step by step until a rebuild -- and returned for the other engine to replay).  Returns what is compared."""
    from chemlab_amd import espp
    r = 0.002 * np.arange(1, 1001)
    rz = 1.5
    sw = np.clip(1.0 - (r / rz) ** 2, 0.0, None)
    e1 = 3.0 * (1.0 - r / 2.0) ** 2 * sw ** 2
    f1 = 3.0 * (1.0 - r / 2.0) * sw ** 2 + 3.0 * (1.0 - r / 2.0) ** 2 * 4.0 * r / rz ** 2 * sw
    e2 = np.exp(-2.0 * r) * sw ** 2
    f2 = 2.0 * np.exp(-2.0 * r) * sw ** 2 + np.exp(-2.0 * r) * 4.0 * r / rz ** 2 * sw
    np.savetxt(tmp_path / "t1.pot", np.stack([r, e1, f1], 1), fmt="%15.8g")
    np.savetxt(tmp_path / "t2.pot", np.stack([r, e2, f2], 1), fmt="%15.8g")
    system = espp.System()
    if dd:
        system.engine.set_option("dd_self", 1)
    system.rng = espp.esutil.RNG(3)
    system.skin = 0.15
    k = 14
    n = k ** 3
    box = (k * 1.0,) * 3
    system.bc = espp.bc.OrthorhombicBC(system.rng, box)
    system.storage = espp.storage.DomainDecomposition(system, espp.tools.decomp.nodeGrid(1), espp.tools.decomp.cellGrid(box, (1, 1, 1), 1.5, 0.15))
    integrator = espp.integrator.VelocityVerlet(system)
    integrator.dt = 0.004
    rng = np.random.default_rng(5)
    g1 = np.arange(k)
    pos = np.stack(np.meshgrid(g1, g1, g1, indexing="ij"), -1).reshape(-1, 3) + 0.5 + rng.uniform(-0.1, 0.1, (n, 3))
    vel = rng.normal(0.0, 1.2, (n, 3))
    types = np.zeros(n, np.int32)
    pool = rng.choice(n, size=40, replace=False)
    types[pool] = 1
    plist = [[i + 1, int(types[i]), espp.Real3D(*pos[i]), espp.Real3D(*vel[i]), 1.0] for i in range(n)]
    system.storage.addParticles(plist, "id", "type", "pos", "v", "mass")
    system.storage.decompose()
    vl = espp.VerletList(system, cutoff=1.5, exclusionlist=espp.DynamicExcludeList(integrator, []))
    obs = espp.analysis.ChemicalConversion(system, 2, len(pool))
    mix = espp.interaction.VerletListMixedTabulated(vl)
    pot = espp.interaction.MixedTabulated(1, str(tmp_path / "t1.pot"), str(tmp_path / "t2.pot"), obs, cutoff=1.5)
    mix.setPotential(type1=0, type2=0, potential=pot)
    system.addInteraction(mix, "lj-mix_tab")
    pe = espp.analysis.PotentialEnergy(system, mix)
    eng = system.engine
    out = dict(x=[], e=[], f=[], conv=[], mix=[pot.mix_value], reb=[], legs=[])
    integrator.run(0)
    out["f"].append(eng.get_state("FORCE"))
    for m, mv in enumerate([pool[:6], pool[6:15], pool[15:30]]):
        if legs is not None:
            integrator.run(legs[m])
        elif m == 1:                                  # step by step up to the next list rebuild
            r0, steps = eng.timers()["rebuilds"], 0
            while eng.timers()["rebuilds"] == r0:
                integrator.run(1)
                steps += 1
                assert steps < 200
            out["legs"].append(steps)
        else:
            integrator.run(20)
            out["legs"].append(20)
        out["reb"].append(eng.timers()["rebuilds"])
        e_old = pe.compute()                          # mixed-table energy of this configuration under the old mixture
        for i in mv:
            system.storage.modifyParticle(int(i) + 1, "type", 2)
        out["conv"].append(obs.compute())             # the observable's listeners re-send the mixed table
        out["mix"].append(pot.mix_value)
        out["e"].append((e_old, pe.compute()))        # ... and under the new one, same configuration
        integrator.run(0)
        out["f"].append(eng.get_state("FORCE")); out["x"].append(eng.get_state("POS_UNFOLDED"))
    integrator.run(15)
    out["x"].append(eng.get_state("POS_UNFOLDED"))
    if legs is not None:
        out["legs"] = list(legs)
    return out


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("dd", [0, 1])
def test_mixed_tabulated_through_the_shim(tmp_path, prec, dd):
    """nonbond func 10 on the HIP path: the mixed table re-sent through chem_nb_table whenever the conversion moves, between
    runs and once right after a list rebuild -- conversion, mixture, the mixed-table energy before and after each move on
    the same configuration, forces and the trajectory of the same script on the oracle."""
    from chemlab_amd import espp
    from chemlab_amd.engine import Engine
    from oracle.oracle import OracleEngine
    prev = espp._factory[0]
    try:
        espp.set_engine_factory(lambda: OracleEngine())
        ref = _mixed_script(tmp_path, 0)
        espp.set_engine_factory(lambda: Engine(device=0, precision=prec))
        got = _mixed_script(tmp_path, dd, legs=ref["legs"])
    finally:
        espp.set_engine_factory(prev)
    assert ref["conv"] == got["conv"] == [6 / 40, 15 / 40, 30 / 40]
    assert ref["mix"] == got["mix"] == [0.0, 6 / 40, 15 / 40, 30 / 40]
    assert ref["reb"][1] > ref["reb"][0]                          # (rebuild counts are not compared: the HIP path also
                                                                   #  rebuilds when the matrix changes)
    tol_e, tol_f, tol_x = (1e-10, 1e-9, 1e-8) if prec == 64 else (2e-5, 5e-5, 2e-4)
    for (g_old, g_new), (o_old, o_new) in zip(got["e"], ref["e"]):
        assert abs(o_new - o_old) > 1e-3 * abs(o_old)            # the move changed the potential
        assert g_old == pytest.approx(o_old, rel=tol_e) and g_new == pytest.approx(o_new, rel=tol_e)
    for a, b in zip(got["f"], ref["f"]):
        assert rel_err(a, b) < tol_f
    for a, b in zip(got["x"], ref["x"]):
        assert rel_err(a, b) < tol_x


# ---- cutoff refusal -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("list_skin", [0.0, 0.6])
def test_pair_cutoff_beyond_the_list_cutoff_is_refused(make_gpu, list_skin):
    """A pair cutoff above max_cutoff is refused at run() as on the oracle (tests/test_oracle_pair_matrix.py); before,
    the forces depended on the list's radius (option list_skin).  At max_cutoff it runs."""
    spec = pair_matrix_spec(2, n=4000)
    spec["types"] = np.where(np.arange(spec["n"]) % 2, 3, 0).astype(np.int32)
    spec["lj"], spec["tables"] = [(0, 0, 1.0, 1.0, spec["rc"])], []
    spec["rebuild_criterion"] = 0
    g = make_gpu(64)
    if list_skin:
        g.set_option("list_skin", list_skin)
    W.apply(spec, g, thermostat=False)
    g.nb_lj(0, 3, 1.0, 1.0, spec["rc"] + 0.05, True)
    with pytest.raises(ChemError) as ex:
        g.run(0)
    assert ex.value.code == _capi.EINVAL and "(0,3)" in str(ex.value)
    g.nb_lj(0, 3, 1.0, 1.0, spec["rc"], True)
    g.nb_table(3, 3, 0.1, 0.1, np.zeros(4), np.zeros(4), spec["rc"] + 0.5)
    with pytest.raises(ChemError) as ex:
        g.run(0)
    assert ex.value.code == _capi.EINVAL and "(3,3)" in str(ex.value)
    g.nb_table(3, 3, 0.1, 0.1, np.zeros(4), np.zeros(4), spec["rc"])
    g.run(0)
