"""GPU parity tests proper: HIP path (through the C ABI) vs the CPU oracle on identical seeded
inputs.  Tolerances: fp64 mode 1e-10 relative (summation order only); fp32 mode 1e-5 of the largest force for
pair forces -- SURVEY App. E's figure, reachable since the fp32 build keeps its positions as int32 fixed point and
stages tile-local coordinates (round 3; with absolute fp32 coordinates it was 5e-5) --, 5e-5 where K = 1.6e5 bonds
amplify the coordinate rounding (was 5e-4), 2e-5 for one dense crystal slab (26 neighbours at 0.96 sigma: large
cancelling terms).  Integer results (lists, events, states, types) must be bit-identical."""
import os
import sys

import numpy as np
import pytest

from chemlab_amd import workloads as W
from conftest import rel_err
from helpers import brute_pairs, force_error_without_cutoff_flips, geometry_spec, list_difference, sorted_events, total_epot

pytestmark = pytest.mark.gpu

TOL = {64: 1e-10, 32: 1e-5}
TOL_STIFF32 = 5e-5      # systems with K = 1.6e5 harmonic bonds (mf/espp_cg_1 force field)
TOL_MELT32 = 2e-5       # fp32 pair forces of a melt, cutoff-boundary decisions set apart (helpers.force_error_without_cutoff_flips)


def both(make_gpu, make_oracle, spec, prec, **kw):
    # the rebuild trigger is part of the spec so that both sides use the same one
    # (0: reference's accumulated per-step maxima, 1: max true displacement since the last build)
    spec.setdefault("rebuild_criterion", 1)
    g, o = make_gpu(prec), make_oracle()
    hg = W.apply(spec, g, **kw)
    ho = W.apply(spec, o, **kw)
    assert hg == ho
    return g, o, hg


@pytest.mark.parametrize("prec", [64, 32])
def test_lj_melt_forces_energy_and_list(make_gpu, make_oracle, prec):
    spec = W.lj_melt(n=4000, seed=1, jitter=0.08)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < TOL[prec]
    og, oo = g.observe(), o.observe()
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=1e-11 if prec == 64 else 2e-6)
    assert og["ekin"] == pytest.approx(oo["ekin"], rel=1e-12 if prec == 64 else 1e-6)
    assert og["virial_nb"] == pytest.approx(oo["virial_nb"], rel=1e-10 if prec == 64 else 1e-5)
    if prec == 64:
        assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())
    else:
        a = {tuple(p) for p in g.get_verlet_pairs().tolist()}
        b = {tuple(p) for p in o.get_verlet_pairs().tolist()}
        assert len(a ^ b) <= 4      # pairs within fp32 rounding of rc+skin


@pytest.mark.parametrize("tpp", [1, 2, 4, 8, 16, 32, 64])
def test_pair_kernel_lane_widths_agree(make_gpu, make_oracle, tpp):
    spec = W.lj_melt(n=2048, seed=6, jitter=0.08)
    g, o, _ = both(make_gpu, make_oracle, spec, 64, thermostat=False)
    g.set_option("tpp", tpp)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-10


@pytest.mark.parametrize("prec", [64, 32])
def test_tiled_and_per_cell_paths_agree(make_gpu, make_oracle, prec):
    """LDS-tiled list/force kernels (ragged 7x7x7 cell grid) vs the per-cell fall-back vs the oracle."""
    spec = W.reactive_melt(n=8788, seed=5)
    spec["exclusions"] = np.stack([np.arange(1, 2001, 2), np.arange(2, 2002, 2)], 1)
    a, b, o = make_gpu(prec), make_gpu(prec), make_oracle()
    for e in (a, b, o):
        W.apply(spec, e, thermostat=False, reactions=False)
    b.set_option("tiles", 0)
    for e in (a, b, o):
        e.run(0)
    fo = o.get_state("FORCE")
    assert rel_err(a.get_state("FORCE"), fo) < TOL[prec]
    assert rel_err(b.get_state("FORCE"), fo) < TOL[prec]
    assert np.array_equal(a.get_verlet_pairs(), b.get_verlet_pairs())
    if prec == 64:
        assert np.array_equal(a.get_verlet_pairs(), o.get_verlet_pairs())
    oa, oo = a.observe(), o.observe()
    assert oa["epot_lj"] == pytest.approx(oo["epot_lj"], rel=1e-11 if prec == 64 else 2e-6)
    a.run(30); b.run(30); o.run(30)
    assert rel_err(a.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-9 if prec == 64 else 1e-4)
    assert rel_err(b.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-9 if prec == 64 else 1e-4)


def test_small_box_brute_force_list(make_gpu, make_oracle):
    # box edge < 3 (rc+skin): the list is built by the brute-force kernel with minimum image
    rng = np.random.default_rng(3)
    g1 = np.arange(7)
    pos = np.stack(np.meshgrid(g1, g1, g1, indexing="ij"), -1).reshape(-1, 3) * 1.1 + 0.55 + rng.uniform(-0.05, 0.05, (343, 3))
    n = 343
    spec = dict(n=n, box=[7.7, 7.7, 7.7], rc=2.5, skin=0.3, dt=0.004, ids=np.arange(10, 10 + 2 * n, 2),
                types=np.zeros(n, np.int32), pos=pos, vel=rng.normal(0, 0.5, (n, 3)),
                mass=np.ones(n), lj=[(0, 0, 1.0, 1.0, 2.5)], kT=1.0, gamma=0.0, seed=1,
                exclusions=np.array([[10, 12], [14, 30]]))
    g, o, _ = both(make_gpu, make_oracle, spec, 64)
    assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())
    g.run(40); o.run(40)
    assert g.timers()["rebuilds"] == o.timers()["rebuilds"] >= 2
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9


@pytest.mark.parametrize("prec", [64, 32])
def test_multi_type_lj_with_switched_off_pairs(make_gpu, make_oracle, prec):
    spec = W.reactive_melt(n=4000, seed=2)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False, reactions=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < TOL[prec]


@pytest.mark.parametrize("prec", [64, 32])
def test_tabulated_and_bonded_polymer(make_gpu, make_oracle, prec):
    spec = W.polymer_melt(n_chains=128, chain_len=32, seed=3)   # 4096 beads
    g, o, h = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (TOL[64] if prec == 64 else TOL_STIFF32)
    if prec == 32:      # the tabulated pair forces alone (same exclusions, bonded lists without parameters removed)
        pair_only = dict(spec, lists=[])
        g2, o2, _ = both(make_gpu, make_oracle, pair_only, 32, thermostat=False)
        g2.run(0); o2.run(0)
        assert rel_err(g2.get_state("FORCE"), o2.get_state("FORCE")) < TOL[32]
    og, oo = g.observe(), o.observe()
    for k in range(2):
        assert og["epot_list"][k] == pytest.approx(oo["epot_list"][k], rel=1e-11 if prec == 64 else 1e-5)
    assert og["epot_tab"] == pytest.approx(oo["epot_tab"], rel=1e-11 if prec == 64 else 1e-4, abs=1e-3)
    assert og["list_size"] == oo["list_size"]
    if prec == 64:
        assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())   # exclusions honoured


def test_dihedral_and_fene_and_cosine(make_gpu, make_oracle):
    rng = np.random.default_rng(8)
    nm = 125
    base = (np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3) * 4.0 + 1.0)
    off = np.array([[0, 0, 0], [0.9, 0.2, 0.1], [1.2, 1.1, 0.4], [2.1, 1.3, 1.2]])
    pos = (base[:, None, :] + off[None]).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (4 * nm, 3))
    n = 4 * nm
    ids = np.arange(1, n + 1).reshape(nm, 4)
    spec = dict(n=n, box=[20.0] * 3, rc=2.5, skin=0.3, dt=0.002, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32),
                pos=pos, vel=rng.normal(0, 0.3, (n, 3)), mass=np.ones(n), lj=[(0, 0, 0.2, 0.8, 2.5)], kT=1.0, gamma=0.0, seed=1,
                lists=[dict(arity=2, kind="FENE", params=[30.0, 0.0, 2.5], ids=np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 3]]])),
                       dict(arity=3, kind="ANG_COSINE", params=[2.0, np.deg2rad(130)], ids=np.concatenate([ids[:, [0, 1, 2]], ids[:, [1, 2, 3]]])),
                       dict(arity=4, kind="DIH_NCOS", params=[1.5, np.deg2rad(20), 3.0], ids=ids),
                       dict(arity=4, kind="DIH_RB", params=[0.5, -0.3, 0.2, 0.1, -0.1, 0.05], ids=ids[::2])],
                exclusions=np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 3]], ids[:, [0, 2]], ids[:, [1, 3]], ids[:, [0, 3]]]))
    g, o, _ = both(make_gpu, make_oracle, spec, 64)
    dphi = 2 * np.pi / 720                                    # a tabulated dihedral (func 8) on every third molecule as well
    phi = -np.pi + dphi * np.arange(721)
    for eng in (g, o):
        h = eng.list_create(4, "DIH_TABULATED")
        eng.list_set_params(h, [eng.table_create(phi[0], dphi, 0.8 * (1 + np.cos(2 * phi - 0.3)), 1.6 * np.sin(2 * phi - 0.3))])
        eng.list_add(h, ids[::3])
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-10
    og, oo = g.observe(), o.observe()
    assert np.allclose(og["epot_list"], oo["epot_list"], rtol=1e-11)
    g.run(50); o.run(50)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9


@pytest.mark.parametrize("criterion", [0, 1])
def test_nve_trajectory_matches_oracle_fp64(make_gpu, make_oracle, criterion):
    spec = W.lj_melt(n=4000, seed=1)
    spec["rebuild_criterion"] = criterion
    g, o, _ = both(make_gpu, make_oracle, spec, 64, thermostat=False)
    g.run(100); o.run(100)
    assert g.timers()["rebuilds"] == o.timers()["rebuilds"] >= (4 if criterion == 0 else 3)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-8
    assert np.array_equal(g.get_state("IMAGE"), o.get_state("IMAGE"))


def test_fused_and_split_integrator_agree(make_gpu):
    spec = W.lj_melt(n=2048, seed=4, gamma=1.0)
    spec["rebuild_criterion"] = 0
    a, b = make_gpu(64), make_gpu(64)
    W.apply(spec, a); W.apply(spec, b)
    b.set_option("fuse_integrate", 0)
    a.run(40); b.run(40)
    assert rel_err(a.get_state("POS_UNFOLDED"), b.get_state("POS_UNFOLDED")) < 1e-12


def test_langevin_trajectory_matches_oracle_fp64(make_gpu, make_oracle):
    spec = W.lj_melt(n=2048, seed=5, gamma=1.0)
    g, o, _ = both(make_gpu, make_oracle, spec, 64)
    g.run(30); o.run(30)
    g.run(20); o.run(20)      # second call: run()-start force evaluation, phase-0 noise
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-8


def test_fp32_nve_conserves_energy_and_momentum(make_gpu):
    spec = W.lj_melt(n=32000, seed=1)            # C2 at full size
    g = make_gpu(32)
    W.apply(spec, g, thermostat=False)
    g.run(0)
    o0 = g.observe()
    g.run(1000)
    o1 = g.observe()
    drift = abs((o1["ekin"] + o1["epot_lj"]) - (o0["ekin"] + o0["epot_lj"])) / spec["n"]
    assert drift < 2e-3
    assert np.abs(o1["momentum"]).max() < 1e-6 * spec["n"]
    assert g.timers()["rebuilds"] > 30


@pytest.mark.parametrize("prec", [64, 32])
def test_reaction_scan_frozen_positions_bit_identical(make_gpu, make_oracle, prec):
    """One React() on frozen, fp32-representable positions: candidate resolve, new bonds,
    state and type vectors must be bit-identical; r^2 is evaluated in fp64 on both sides."""
    spec = W.reactive_melt(n=8788, seed=11, interval=1, rho=0.8442)   # 13^3*4
    spec["box"] = [float(np.float32(spec["box"][0]))] * 3
    spec = W.snap_to_grid(spec)        # positions both builds represent exactly (fp32 build: int32 fixed point)
    spec["dt"] = 1e-9
    spec["vel"] = np.zeros_like(spec["vel"])
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e12
    g, o, h = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    if prec == 32:
        # dt=1e-9: x += dt*v leaves fp32 positions untouched only if forces*dt^2 underflow the ulp
        pass
    g.run(1); o.run(1)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 1000
    if prec == 64:
        assert eg == eo
    else:
        assert [e[:4] for e in eg] == [e[:4] for e in eo]
        assert np.allclose([e[4] for e in eg], [e[4] for e in eo], rtol=1e-6)
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert np.array_equal(g.get_state("TYPE"), o.get_state("TYPE"))
    assert np.array_equal(g.get_list(h["reaction_bonds"]), o.get_list(h["reaction_bonds"]))


def test_reactive_trajectory_event_log_identical_fp64(make_gpu, make_oracle):
    spec = W.reactive_melt(n=8788, seed=12, interval=25)
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    for _ in range(3):
        g.run(25); o.run(25)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 2000
    assert [e[:4] for e in eg] == [e[:4] for e in eo]
    assert np.allclose([e[4] for e in eg], [e[4] for e in eo], rtol=1e-9)
    assert np.array_equal(g.get_list(h["reaction_bonds"]), o.get_list(h["reaction_bonds"]))
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert np.array_equal(g.get_state("TYPE"), o.get_state("TYPE"))
    assert np.array_equal(g.get_state("RESID"), o.get_state("RESID"))
    assert np.array_equal(g.get_state("MOLID"), o.get_state("MOLID"))
    assert np.array_equal(g.get_exclusions(), o.get_exclusions())
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8


@pytest.mark.parametrize("prec", [32, 64])
def test_fused_rebuild_equals_unfused_chain_bitwise(make_gpu, prec):
    """One persistent rebuild launch (grid barriers, tile queues, bonded work list, exclusions located
    as tile slots) against the chain of separate kernels it replaces (exclusions by tag): the list a
    particle gets does not depend on which workgroup built it or how exclusions were filtered, so the
    two trajectories -- Langevin noise, reactions, new bonds and exclusions included -- are bit-identical."""
    spec = W.reactive_melt(n=8788, seed=21, interval=20)
    a, b = make_gpu(prec), make_gpu(prec)
    for e in (a, b):
        W.apply(spec, e)
    b.set_option("fused_rebuild", 0)
    a.set_option("bonds_inline", 0)      # (the unfused chain evaluates bonds from exact positions, the inline path from the staged image: equal to rounding, not to the bit)
    for _ in range(4):
        a.run(20); b.run(20)
    assert len(a.get_events()) > 1000
    assert a.timers()["rebuilds"] == b.timers()["rebuilds"] > 4
    assert sorted_events(a.get_events()) == sorted_events(b.get_events())
    assert np.array_equal(a.get_exclusions(), b.get_exclusions())
    for what in ("POS", "VEL", "FORCE", "STATE", "TYPE", "RESID", "MOLID"):
        assert np.array_equal(a.get_state(what), b.get_state(what)), what
    assert np.array_equal(a.get_verlet_pairs(), b.get_verlet_pairs())


def test_fused_rebuild_many_exclusions_per_particle(make_gpu, make_oracle):
    """Chains with bonds, angles and dihedrals: inner monomers carry 6 exclusions (> the 4 slots of
    the in-tile exclusion path), chain ends fewer -- both routes inside one list build, against the oracle."""
    spec = W.polymer_melt(n_chains=400, chain_len=24, seed=8)
    g, o, _ = both(make_gpu, make_oracle, spec, 64, thermostat=False)
    g.run(0); o.run(0)
    assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-10
    g.run(40); o.run(40)
    assert g.timers()["rebuilds"] > 3
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())


def test_random_partner_mode_and_partial_rate_identical(make_gpu, make_oracle):
    spec = W.reactive_melt(n=4000, seed=13, interval=10, rate=20.0)     # p = 20*0.005*10 = 1.0 -> use 6.0 -> 0.3
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 6.0
    spec["reaction"]["nearest"] = False
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    g.run(30); o.run(30)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 200
    assert [e[:4] for e in eg] == [e[:4] for e in eo]


def test_topology_manager_parity_trimer_melt(make_gpu, make_oracle):
    spec = W.trimer_melt(n_mol=216, seed=4, interval=20)
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    g.run(60); o.run(60)
    assert len(o.get_events()) > 5
    assert sorted_events(g.get_events()) == sorted_events(o.get_events()) or \
        [e[:4] for e in sorted_events(g.get_events())] == [e[:4] for e in sorted_events(o.get_events())]
    for k in (0, 1, "reaction_bonds"):
        assert np.array_equal(g.get_list(h[k]), o.get_list(h[k]))
    assert np.array_equal(g.get_exclusions(), o.get_exclusions())
    assert np.array_equal(g.get_state("RESID"), o.get_state("RESID"))
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    og, oo = g.observe(), o.observe()
    assert np.allclose(og["epot_list"], oo["epot_list"], rtol=1e-8)
    assert og["list_size"] == oo["list_size"]


def test_modify_particle_and_errors(make_gpu):
    from chemlab_amd.engine import ChemError
    spec = W.lj_melt(n=500, seed=2)
    g = make_gpu(32)
    W.apply(spec, g, thermostat=False)
    g.run(2)
    g.modify_particle(7, "state", 3)
    g.modify_particle(7, "mass", 2.5)
    assert g.get_state("STATE")[6] == 3 and g.get_state("MASS")[6] == 2.5
    with pytest.raises(ChemError):
        g.modify_particle(10 ** 9, "state", 1)
    with pytest.raises(ChemError):
        g.reaction_init(0)
    with pytest.raises(ChemError):
        g.list_create(5, "HARMONIC")


# ---- slab domain decomposition, exercised on ONE GPU: the rank's lower and upper z-neighbour are
# itself (device copies, or RCCL send/recv to self), so migration, ghost layers, the ghost-mode tile
# tables and the candidate gather all run for real and must reproduce the single-domain oracle.
@pytest.mark.parametrize("transport", ["dd_self", "dd_self_rccl"])
def test_dd_self_forces_lists_and_trajectory(make_gpu, make_oracle, transport):
    spec = W.lj_melt(n=8788, seed=31, jitter=0.08, kT=1.5)      # 13^3*4, 7 cell layers
    spec["rebuild_criterion"] = 0
    g, o = make_gpu(64), make_oracle()
    g.set_option(transport, 1)
    W.apply(spec, g, thermostat=False); W.apply(spec, o, thermostat=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-10
    assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())
    og, oo = g.observe(), o.observe()
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=1e-11)
    assert og["ekin"] == pytest.approx(oo["ekin"], rel=1e-12)
    g.run(150); o.run(150)                                      # particles cross z = 0 / L and migrate
    assert g.timers()["rebuilds"] >= 5
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    assert np.array_equal(g.get_state("IMAGE"), o.get_state("IMAGE"))
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-7


def test_dd_self_reactive_polymer_parity(make_gpu, make_oracle):
    spec = W.reactive_melt(n=8788, seed=12, interval=25)
    g, o = make_gpu(64), make_oracle()
    g.set_option("dd_self", 1)
    hg, ho = W.apply(spec, g), W.apply(spec, o)
    for _ in range(3):
        g.run(25); o.run(25)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 2000
    assert [e[:4] for e in eg] == [e[:4] for e in eo]
    assert np.array_equal(g.get_list(hg["reaction_bonds"]), o.get_list(ho["reaction_bonds"]))
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert np.array_equal(g.get_state("TYPE"), o.get_state("TYPE"))
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    og, oo = g.observe(), o.observe()
    assert np.allclose(og["epot_list"], oo["epot_list"], rtol=1e-9)


def test_dd_self_bonded_chains_fp32(make_gpu, make_oracle):
    spec = W.polymer_melt(n_chains=256, chain_len=32, seed=3)     # 8192 beads, bonds/angles across the ghost layer
    g, o = make_gpu(32), make_oracle()
    g.set_option("dd_self", 1)
    W.apply(spec, g, thermostat=False); W.apply(spec, o, thermostat=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < TOL_STIFF32
    g.run(40); o.run(40)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 2e-4


# ---- multi-rank slab decomposition with all ranks inside this process (one host thread per rank,
# device-to-device exchange through chem_comm_init_local): distinct slabs, real neighbours,
# migration between ranks, cross-rank candidate gather -- against the single-domain oracle.
def _run_ranks(P, fn):
    import threading
    out, err = [None] * P, [None] * P

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:   # noqa: BLE001
            err[r] = e
    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    for e in err:
        if e is not None:
            raise e
    return out


_HUB = [100]


@pytest.mark.parametrize("P,n", [(2, 8788), (3, 8788), (4, 16384)])
def test_dd_multi_rank_in_process_lj(make_gpu, make_oracle, P, n):
    spec = W.lj_melt(n=n, seed=33, jitter=0.08, kT=1.5)
    spec["rebuild_criterion"] = 0
    o = make_oracle()
    W.apply(spec, o, thermostat=False)
    o.run(0)
    f0 = o.get_state("FORCE")
    vp0 = o.get_verlet_pairs()
    e0 = o.observe()
    o.run(120)
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        W.apply(spec, g, thermostat=False)
        g.run(0)
        res = dict(f=g.get_state("FORCE"), vp=g.get_verlet_pairs(), obs=g.observe())
        g.run(120)
        res.update(x=g.get_state("POS_UNFOLDED"), v=g.get_state("VEL"), img=g.get_state("IMAGE"), reb=g.timers()["rebuilds"])
        return res
    out = _run_ranks(P, rank)
    for r in range(P):
        assert rel_err(out[r]["f"], f0) < 1e-10
        assert np.array_equal(out[r]["vp"], vp0)
        assert out[r]["obs"]["epot_lj"] == pytest.approx(e0["epot_lj"], rel=1e-11)
        assert out[r]["obs"]["ekin"] == pytest.approx(e0["ekin"], rel=1e-12)
        assert rel_err(out[r]["x"], o.get_state("POS_UNFOLDED")) < 1e-8
        assert np.array_equal(out[r]["img"], o.get_state("IMAGE"))
        assert out[r]["reb"] >= 4


@pytest.mark.parametrize("chunks", [(25, 25, 25), (75,), (10, 41, 24)])
def test_dd_multi_rank_in_process_reactive(make_gpu, make_oracle, chunks):
    # chunks: run() boundaries on, beyond and between the reaction steps (25, 50, 75)
    P = 2
    spec = W.reactive_melt(n=8788, seed=12, interval=25)
    o = make_oracle()
    ho = W.apply(spec, o)
    for k in chunks:
        o.run(k)
    engs = [make_gpu(64) for _ in range(P)]
    _HUB[0] += 1
    hub = _HUB[0]

    def rank(r):
        g = engs[r]
        g.comm_init_local(P, r, hub)
        h = W.apply(spec, g)
        for k in chunks:
            g.run(k)
        return dict(ev=sorted_events(g.get_events()), bonds=g.get_list(h["reaction_bonds"]), st=g.get_state("STATE"),
                    ty=g.get_state("TYPE"), x=g.get_state("POS_UNFOLDED"), el=g.observe()["epot_list"])
    out = _run_ranks(P, rank)
    eo = sorted_events(o.get_events())
    assert len(eo) > 2000
    for r in range(P):
        assert [e[:4] for e in out[r]["ev"]] == [e[:4] for e in eo]
        assert np.array_equal(out[r]["bonds"], o.get_list(ho["reaction_bonds"]))
        assert np.array_equal(out[r]["st"], o.get_state("STATE"))
        assert np.array_equal(out[r]["ty"], o.get_state("TYPE"))
        assert rel_err(out[r]["x"], o.get_state("POS_UNFOLDED")) < 1e-8
        assert np.allclose(out[r]["el"], o.observe()["epot_list"], rtol=1e-9)


@pytest.mark.parametrize("example,argv,min_events", [
    ("chain_growth_catalytic", ["@params", "--run=2500", "--start_ar=500"], 100),
    ("mf_espp_cg_1", ["@params", "--run=3000", "--start_ar=1000", "--int_step=500", "--energy_collect=500", "--trj_collect=1000", "--rng_seed=7"], 5),
    # C1 (BASELINE configs[0]): examples/atrp_lj with its atrp.cfg UNMODIFIED (ATRPActivator + ChangeNeighboursProperty);
    # a hooks.py (start_simulation.py:214-228) creates dormant initiators (FA in state 2) the way examples/atrp_lj/hooks.py does
    ("atrp_lj", ["@params", "--run=3000", "--maximum_conversion=", "--rng_seed=11"], 10)])
def test_driver_on_gpu_matches_driver_on_oracle(tmp_path, monkeypatch, oracle_mod, example, argv, min_events):
    """The py3 start_simulation driver (readers -> espressopp-shaped shim -> C ABI) on shipped example inputs
    (LJ chain growth; tabulated non-bonded melt with Langevin at 800 K; ATRP trimer melt with neighbour property changes and
    registered angle spawning): HIP engine (fp64) vs the oracle behind the same shim."""
    import os, shutil
    from chemlab_amd import espp, start_simulation
    from chemlab_amd.engine import Engine
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", example)
    out = {}
    for name, fac in (("gpu", lambda: Engine(device=0, precision=64)), ("oracle", lambda: oracle_mod.OracleEngine())):
        d = tmp_path / name
        shutil.copytree(gold, str(d))
        if example == "atrp_lj":
            os.makedirs(str(d / "data"), exist_ok=True)
            (d / "hooks.py").write_text(
                "def hook_init_reaction(system, integrator, ar, topol, args):\n"
                "    n2t = topol.atomsym_atomtype\n"
                "    for mol in range(40):\n"
                "        for k, (name, state) in enumerate((('FA', 2), ('PL', 2), ('PA', None))):\n"
                "            pid = 3 * mol * 7 + 1 + k\n"
                "            system.storage.modifyParticle(pid, 'type', n2t[name])\n"
                "            system.storage.modifyParticle(pid, 'mass', topol.gt.atomtypes[name]['mass'])\n"
                "            if state is not None:\n"
                "                system.storage.modifyParticle(pid, 'state', state)\n"
                "    return True\n")
        monkeypatch.chdir(d)
        espp.set_engine_factory(fac)
        try:
            res = start_simulation.main(list(argv), quiet=True)
        finally:
            espp.set_engine_factory(lambda: Engine(device=0, precision=32))
        e = res["system"].engine
        out[name] = dict(ev=sorted_events(e.get_events()), bonds=res["chem_fpls"][0][1].getAllBonds(), st=e.get_state("STATE"),
                         ty=e.get_state("TYPE"), x=e.get_state("POS_UNFOLDED"), atrp=e.atrp_stats())
        if example == "atrp_lj":
            assert os.path.exists("data/cpc01_11_atrp_stats.dat")            # ATRPActivator.stats_filename
    assert len(out["oracle"]["ev"]) > min_events
    assert [v[:4] for v in out["gpu"]["ev"]] == [v[:4] for v in out["oracle"]["ev"]]
    assert out["gpu"]["bonds"] == out["oracle"]["bonds"]
    assert out["gpu"]["atrp"] == out["oracle"]["atrp"] and (example != "atrp_lj" or sum(r["activated"] for r in out["oracle"]["atrp"]) >= 5)
    assert np.array_equal(out["gpu"]["st"], out["oracle"]["st"]) and np.array_equal(out["gpu"]["ty"], out["oracle"]["ty"])
    # (fp64 on both sides: summation order differs in the last bit and a melt amplifies that by ~e^(t/tau); the 3000-step
    #  ATRP run (7.5 tau) ends at 2.5e-6, the discrete outcomes above are identical)
    assert rel_err(out["gpu"]["x"], out["oracle"]["x"]) < (1e-7 if example != "atrp_lj" else 1e-4)


# ---- edge cases and size-independent properties ---------------------------------------------------
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["cubic", "aniso"])
def test_positions_outside_the_box_and_on_its_faces_are_folded(make_gpu, make_oracle, shape, prec):
    """Inputs the readers can produce: coordinates at exactly 0 and L, negative, several box lengths away.
    aniso: box edges 1 : 3 : 10 (3, 10 and 35 cells; a droplet on the corner plus gas), so that the per-axis scales of the
    fp32 position codec differ by a factor of ten."""
    if shape == "cubic":
        spec = W.lj_melt(n=2048, seed=9, jitter=0.05)
    else:
        spec = geometry_spec((3, 10, 34.5), 0.5, "corner_droplet", seed=7700)
    L = spec["box"][0]
    Lv = np.asarray(spec["box"], dtype=np.float64)
    pos = spec["pos"].copy()
    # rigid shifts (no overlaps are created) that put particle 3 exactly on x = 0, particle 4 on y = L and
    # particle 5 on z = -0.0; everything pushed past a face by that must be folded back by the engine
    pos[:, 0] -= pos[3, 0]; pos[:, 1] += Lv[1] - pos[4, 1]; pos[:, 2] -= pos[5, 2]
    pos[3, 0] = 0.0; pos[4, 1] = Lv[1]; pos[5, 2] = -0.0
    pos[0] += [L, 0, 0]; pos[1] -= [0, 2 * Lv[1], 0]; pos[2] += [3 * L, -Lv[1], 5 * Lv[2]]
    # and the particle of particle 3's lattice plane that is nearest to it goes 1e-12 below the face x = 0: less than half a
    # quantum of the fixed-point codec, L / 2^32 = 2e-9 or more (it moves by the jitter at most: no overlap either)
    plane = [k for k in range(6, len(pos)) if abs(pos[k, 0] - np.rint(pos[k, 0] / L) * L) < 0.11]
    below = min(plane, key=lambda k: np.abs(pos[k] - pos[3]).sum())
    pos[below, 0] = np.floor(pos[below, 0] / L + 0.5) * L - 1e-12
    spec["pos"] = pos
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    g.run(0); o.run(0)
    if prec == 64:
        assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())
        assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-10
        g.run(20); o.run(20)
        assert np.array_equal(g.get_state("IMAGE"), o.get_state("IMAGE"))
        assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
        return
    # fp32 build: int32 fixed point, q = rint((x - L/2) / (L / 2^31)), folded and image-counted on the host
    quantum = Lv / 2.0 ** 31
    xg, ug, ig = g.get_state("POS"), g.get_state("POS_UNFOLDED"), g.get_state("IMAGE")
    assert (xg >= 0).all() and (xg < Lv).all()
    bound = 0.5 * quantum + np.spacing(np.abs(pos))
    print("fold %s fp32: worst |unfolded - input| / bound %.3f" % (shape, (np.abs(ug - pos) / bound).max()))
    assert (np.abs(ug - pos) <= bound).all(), (np.abs(ug - pos) / bound).max()
    want = np.floor(pos / Lv).astype(np.int64)
    just_below = (want + 1) * Lv - pos <= 0.5 * quantum          # within half a quantum below a face: image + 1 at position 0 is as good
    assert (ig[~just_below] == want[~just_below]).all()
    assert ((ig[just_below] == want[just_below]) | ((ig[just_below] == want[just_below] + 1) & (xg[just_below] == 0.0))).all()
    assert just_below[below, 0] and just_below.sum() >= 1
    pairs, gap, shell_pairs = brute_pairs(spec)
    assert gap > 1e-9
    diff = list_difference(g.get_verlet_pairs(), dict(spec, pairs=pairs))
    assert diff <= shell_pairs, sorted(diff - shell_pairs)[:5]
    g.run(20); o.run(20)
    # (against the box edge, not the largest unfolded coordinate: particle 2 sits five boxes out, and that would forgive a whole-image slip)
    err = (np.abs(g.get_state("POS_UNFOLDED") - o.get_state("POS_UNFOLDED")) / Lv).max()
    print("fold %s fp32: POS_UNFOLDED / box edge after 20 steps %.2e" % (shape, err))
    assert err < 2e-4, err


@pytest.mark.parametrize("prec", [64, 32])
def test_run_is_additive_and_repeatable(make_gpu, prec):
    """Without a thermostat run(a); run(b) == run(a+b) bit for bit: the force evaluation that opens every
    run() must not change the state.  (With Langevin the opening evaluation draws fresh noise, as
    ESPResSo++'s run() does -- SURVEY 3.3 -- so only repeatability is required there.)  Reactions,
    rebuilds, new bonds and exclusions are active in both halves of the test."""
    spec = W.reactive_melt(n=8788, seed=31, interval=15)
    a, b = make_gpu(prec), make_gpu(prec)
    for e in (a, b):
        W.apply(spec, e, thermostat=False)
    a.run(45)
    b.run(7); b.run(0); b.run(20); b.run(18)        # never split right after a reaction step: a new run()
    assert len(a.get_events()) > 500                 # re-evaluates forces with the new bonds, a running one does not
    assert sorted_events(a.get_events()) == sorted_events(b.get_events())
    for what in ("POS", "VEL", "STATE", "TYPE", "RESID", "MOLID"):
        assert np.array_equal(a.get_state(what), b.get_state(what)), what
    c, d = make_gpu(prec), make_gpu(prec)
    for e in (c, d):
        W.apply(spec, e)                                   # Langevin on
        e.run(20); e.run(25)
    assert len(c.get_events()) > 500
    assert sorted_events(c.get_events()) == sorted_events(d.get_events())
    for what in ("POS", "VEL", "STATE", "TYPE"):
        assert np.array_equal(c.get_state(what), d.get_state(what)), what


def test_reactions_without_candidates_and_two_particle_system(make_gpu, make_oracle):
    spec = W.reactive_melt(n=4000, seed=14, interval=5)
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 0.0                                     # probability 0: scans run, nothing may happen
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    g.run(20); o.run(20)
    assert len(g.get_events()) == 0 and len(o.get_events()) == 0
    assert g.get_list(h["reaction_bonds"]).shape[0] == 0
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    # two particles, one bond, no non-bonded partner inside the cut-off: the smallest valid system
    two = dict(n=2, box=[12.0, 12.0, 12.0], rc=2.5, skin=0.3, dt=0.002, ids=np.array([5, 9]), types=np.zeros(2, np.int32),
               pos=np.array([[1.0, 1.0, 1.0], [11.6, 1.0, 1.0]]), vel=np.zeros((2, 3)), mass=np.array([1.0, 2.0]),
               lj=[(0, 0, 1.0, 1.0, 2.5)], kT=1.0, gamma=0.0, seed=1,
               lists=[dict(arity=2, kind="HARMONIC", params=[30.0, 0.97], ids=np.array([[5, 9]]))], exclusions=np.array([[5, 9]]))
    g2, o2, _ = both(make_gpu, make_oracle, two, 64)
    g2.run(50); o2.run(50)
    assert rel_err(g2.get_state("POS_UNFOLDED"), o2.get_state("POS_UNFOLDED")) < 1e-10
    assert abs(np.asarray(g2.observe()["momentum"])).max() < 1e-12


def test_neighbour_capacity_too_small_is_reported(make_gpu):
    from chemlab_amd.engine import ChemError
    spec = W.lj_melt(n=4000, seed=3)
    g = make_gpu(32)
    W.apply(spec, g, thermostat=False)
    g.set_nlist_capacity(16)            # ~70 neighbours needed
    with pytest.raises(ChemError) as ei:
        g.run(1)
    assert "capacity" in str(ei.value)


def test_full_size_properties_one_million_particles(make_gpu):
    """BASELINE size (the bench workload): properties that need no oracle run.
    * one event per particle and reaction step, bonds unique, exclusions = bonds (both ends known to the log);
    * NVE momentum conserved to fp32 summation noise;
    * a second engine reproduces events and positions bit for bit."""
    spec = W.reactive_melt(n=1000000, rho=0.8, seed=2, interval=40)
    a, b = make_gpu(32), make_gpu(32)
    for e in (a, b):
        W.apply(spec, e, thermostat=False)
    p0 = np.asarray(a.observe()["momentum"])
    a.run(80); b.run(80)
    ev = a.get_events()
    assert len(ev) > 100000
    for st in np.unique(ev["step"]):
        blk = ev[ev["step"] == st]
        ids = np.concatenate([blk["id_a"], blk["id_b"]])
        assert len(np.unique(ids)) == len(ids)
    assert np.array_equal(ev, b.get_events())
    assert np.array_equal(a.get_state("POS"), b.get_state("POS"))
    ex = a.get_exclusions()
    key = np.sort(ex, 1)
    assert len(np.unique(key[:, 0] * (1 << 32) + key[:, 1])) == len(ex)
    in_log = np.zeros(spec["n"] + 2, bool)
    in_log[ev["id_a"]] = True; in_log[ev["id_b"]] = True
    assert in_log[ex].all()
    p1 = np.asarray(a.observe()["momentum"])
    assert np.abs(p1 - p0).max() < 2e-2 * np.sqrt(spec["n"])     # |p| per particle ~1: relative 2e-5 of the random-sum scale
    assert a.timers()["rebuilds"] >= 5


@pytest.mark.parametrize("transport", [None, "dd_self", "dd_self_rccl+overlap"])
def test_one_run_across_reaction_steps_matches_oracle(make_gpu, make_oracle, transport):
    """Regression: the reaction sits between the force evaluation of step s and the first kick of step s+1.
    A list rebuild at the reaction step used to re-sort the particles (and, decomposed, migrate them) away
    from their forces; every parity test that steps in chunks of `interval` missed it because a new run()
    re-evaluates the forces first.  One run() over three reaction steps, single domain and decomposed."""
    spec = W.reactive_melt(n=8788, seed=31, interval=15)
    spec["rebuild_criterion"] = 0
    g, o = make_gpu(64), make_oracle()
    if transport:
        g.set_option(transport.split("+")[0], 1)
        if transport.endswith("+overlap"):                 # interior tiles computed while the halo is in flight
            g.set_option("overlap_halo", 1)
    hg = W.apply(spec, g, thermostat=False); ho = W.apply(spec, o, thermostat=False)
    g.run(50); o.run(50)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 1500 and [e[:4] for e in eg] == [e[:4] for e in eo]
    assert np.array_equal(g.get_list(hg["reaction_bonds"]), o.get_list(ho["reaction_bonds"]))
    assert len(g.get_list(hg["reaction_bonds"])) > 50
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-8
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9


@pytest.mark.parametrize("transport", [None, "dd_self"])
def test_irregular_run_lengths_with_thermostat_and_late_enable(make_gpu, make_oracle, transport):
    """Run lengths that are no multiple of the reaction interval, Langevin on, reactions switched on after the
    first run and off again before the last (start_simulation.py's start_ar/stop_ar) -- the caller decides
    where run() boundaries fall, the trajectory must not care beyond what the reference itself does."""
    spec = W.reactive_melt(n=8788, seed=17, interval=12)
    spec["rebuild_criterion"] = 0
    g, o = make_gpu(64), make_oracle()
    if transport:
        g.set_option(transport, 1)
    hg = W.apply(spec, g); ho = W.apply(spec, o)
    for e in (g, o):
        e.reactions_enable(False)
        e.run(7)
        e.reactions_enable(True)
        e.run(23); e.run(40)
        e.reactions_enable(False)
        e.run(9)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 1500 and [e[:4] for e in eg] == [e[:4] for e in eo]
    assert sorted({e[0] for e in eo}) == [12, 24, 36, 48, 60]
    assert np.array_equal(g.get_list(hg["reaction_bonds"]), o.get_list(ho["reaction_bonds"]))
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8


@pytest.mark.parametrize("prec", [64, 32])
def test_dense_slab_grows_the_tile_capacity(make_gpu, make_oracle, prec):
    """Half the box empty, the other half at twice the mean density: the staged-tile capacity derived from the
    mean occupancy is too small; the first build must notice, grow it and build again (not fail, not truncate)."""
    k = 16
    a = 0.96                                                 # simple cubic, nearest neighbours at 0.96 sigma
    g1 = np.arange(k)
    pos = np.stack(np.meshgrid(np.arange(2 * k), g1, g1, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pos = pos[pos[:, 0] < k] * a + 0.3                       # k^3 particles in the x < L/2 half
    n = len(pos)
    rng = np.random.default_rng(5)
    pos += rng.uniform(-0.02, 0.02, pos.shape)
    L = [2 * k * a, k * a, k * a]
    spec = dict(n=n, box=L, rc=2.5, skin=0.3, dt=0.001, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32), pos=pos,
                vel=np.zeros((n, 3)), mass=np.ones(n), lj=[(0, 0, 1.0, 1.0, 2.5)], kT=1.0, gamma=0.0, seed=1)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (TOL[64] if prec == 64 else 2e-5)   # (fp32: 1.4e-5 measured; 26 neighbours at 0.96 sigma, large cancelling terms)
    if prec == 64:
        assert np.array_equal(g.get_verlet_pairs(), o.get_verlet_pairs())


# ---- BASELINE.json configs[1..3] at their full sizes (production precision fp32 vs the fp64 oracle) ------
def test_baseline_c2_32k_lj_melt(make_gpu, make_oracle):
    spec = W.lj_melt(n=32000, rho=0.8, seed=21, gamma=1.0)
    # a MELT, as BASELINE.json names the configuration: the fcc start is melted first (400 Langevin steps at T = 1 on
    # the HIP path) and both sides then start from that configuration.  (On the near-perfect lattice itself the pair
    # forces of ~20 cancel to net forces below 1, and an error budget relative to the largest NET force is meaningless.)
    m = make_gpu(32); W.apply(spec, m); m.run(400)
    spec = dict(spec, pos=m.get_state("POS"), vel=m.get_state("VEL"))
    g, o, _ = both(make_gpu, make_oracle, spec, 32, thermostat=False)
    g.run(0); o.run(0)
    # a melt has pairs within rounding of rc, where the truncated LJ force jumps by 0.039: those decisions are set apart
    err, flips = force_error_without_cutoff_flips(spec, g.get_state("FORCE"), o.get_state("FORCE"), TOL_MELT32, max_flips=8)
    assert err < TOL_MELT32 and 0 <= flips <= 8, (err, flips)
    og, oo = g.observe(), o.observe()
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=2e-6)
    assert og["virial_nb"] == pytest.approx(oo["virial_nb"], rel=1e-5)
    g.run(20); o.run(20)                                      # NVE, a few rebuilds: fp32 trajectory stays on the fp64 one
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-4


def test_baseline_c3_128k_tabulated_polymer_melt(make_gpu, make_oracle):
    spec = W.polymer_melt(n_chains=4000, chain_len=32, seed=3)       # 128 000 beads, table + bonds + angles + nrexcl 3
    g, o, _ = both(make_gpu, make_oracle, spec, 32, thermostat=False)
    g.run(0); o.run(0)
    # tolerance 5e-5 of the largest force here: K = 1.6e5 bonds amplify the rounding of a coordinate (5e-8 fixed point since
    # round 3; 4e-6 = an fp32 ulp at x ~ 33 before, hence 5e-4 then); the arithmetic of bonded terms is fp64
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < TOL_STIFF32
    og, oo = g.observe(), o.observe()
    for k in range(2):
        assert og["epot_list"][k] == pytest.approx(oo["epot_list"][k], rel=1e-5)
    assert og["epot_tab"] == pytest.approx(oo["epot_tab"], rel=1e-4, abs=1e-2)
    assert og["list_size"] == oo["list_size"] == [4000 * 31, 4000 * 30]
    g.run(20); o.run(20)                                      # 20 steps of the stiff-bond dynamics, a rebuild inside
    assert g.timers()["rebuilds"] == o.timers()["rebuilds"]
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-4
    # the tabulated pair component alone at the pair tolerance (same particles and exclusions, no bonded lists)
    g2, o2, _ = both(make_gpu, make_oracle, dict(spec, lists=[]), 32, thermostat=False)
    g2.run(0); o2.run(0)
    assert rel_err(g2.get_state("FORCE"), o2.get_state("FORCE")) < TOL[32]


def test_baseline_c4_256k_reactive_one_reaction_step(make_gpu, make_oracle):
    """256k monomers, one reaction step on frozen fp32-representable positions: the candidate scan over the
    staged tiles, the resolve and the topology update must give the oracle's events, bonds, states and types."""
    spec = W.reactive_melt(n=256000, rho=0.8, seed=5, interval=1)
    spec["box"] = [float(np.float32(spec["box"][0]))] * 3
    spec = W.snap_to_grid(spec)        # positions both builds represent exactly (fp32 build: int32 fixed point)
    spec["dt"] = 1e-9
    spec["vel"] = np.zeros_like(spec["vel"])
    for r in spec["reaction"]["reactions"]:
        r["rate"] = 1e12
    g, o, h = both(make_gpu, make_oracle, spec, 32, thermostat=False)
    g.run(2); o.run(2)                                        # second step: bond-forming reactions see the new states
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 50000 and [e[:4] for e in eg] == [e[:4] for e in eo]
    assert np.allclose([e[4] for e in eg], [e[4] for e in eo], rtol=1e-6)
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert np.array_equal(g.get_state("TYPE"), o.get_state("TYPE"))
    assert np.array_equal(g.get_list(h["reaction_bonds"]), o.get_list(h["reaction_bonds"]))
    assert np.array_equal(g.get_exclusions(), o.get_exclusions())


def test_baseline_c4_256k_forces_energy_and_reactive_trajectory(make_gpu, make_oracle):
    """C4 at full size in production precision: fp32 pair forces with the A-B / A-D pairs switched off
    (chain_growth_catalytic/topol.top:15-17), energy and virial, then 24 Langevin steps across two reaction steps:
    same event log, positions within the fp32 trajectory tolerance."""
    spec = W.reactive_melt(n=256000, rho=0.8, seed=6, interval=12)
    g, o, h = both(make_gpu, make_oracle, spec, 32)
    g.run(0); o.run(0)
    gf, of = g.get_state("FORCE"), o.get_state("FORCE")
    # the thermostat adds the same keyed noise on both sides (evaluation phase 0); pair part from the lists
    err, flips = force_error_without_cutoff_flips(spec, gf, of, TOL_MELT32, max_flips=40)
    assert err < TOL[32] and 0 <= flips <= 40, (err, flips)
    og, oo = g.observe(), o.observe()
    assert og["epot_lj"] == pytest.approx(oo["epot_lj"], rel=2e-6)
    assert og["virial_nb"] == pytest.approx(oo["virial_nb"], rel=1e-5)
    g.run(24); o.run(24)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 10000 and set(e[0] for e in eo) == {12, 24}
    # fp32 positions can flip a pair across the reaction radius: the logs agree except for a handful of borderline pairs
    sg, so = {e[:4] for e in eg}, {e[:4] for e in eo}
    assert len(sg ^ so) <= max(4, len(so) // 2000)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-4


def test_dd_eight_slabs_at_bench_size_in_process():
    """The N = 8 decomposition of the bench workload (1M particles, 8 slabs of 4-5 cell layers, capacities,
    migration buffers, ghost layers) rehearsed with eight in-process ranks on one GPU: every rank must log the
    same events as a single-domain engine (fp32 on both sides: same arithmetic per pair, same canonical order
    inside cells, so the trajectories agree closely enough for identical discrete outcomes over a short run).
    Nine 1M-particle engines and eight rank threads: run in a child process (tests/dd_eight_slabs_main.py), so that
    whatever goes wrong there is this test's failure, with its stderr, and not the end of the whole session."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dd_eight_slabs_main.py")],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "EIGHT_SLABS_OK" in r.stdout, "child failed (rc %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("prec,thermo", [(64, False), (64, True), (32, True)])
def test_cap_force_matches_oracle(make_gpu, make_oracle, prec, thermo):
    """SURVEY f-1: integrator.CapForce.  A jittered lattice with a few close contacts, cap well below the
    largest forces so that it acts on many particles every step; with and without the Langevin terms on top."""
    spec = W.lj_melt(n=4000, seed=7, jitter=0.16)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=thermo)
    g.cap_force(40.0); o.cap_force(40.0)
    g.run(0); o.run(0)
    fraw = o.get_state("FORCE")
    if not thermo:
        assert (np.linalg.norm(fraw, axis=1) > 40.0).sum() > 50   # get_state returns the evaluated (uncapped) force
    g.run(30); o.run(30)
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < (1e-8 if prec == 64 else 2e-4)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-9 if prec == 64 else 1e-4)
    g.cap_force(0.0); o.cap_force(0.0)                            # switched off again
    g.run(10); o.run(10)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-9 if prec == 64 else 1e-4)


@pytest.mark.parametrize("prec", [64, 32])
def test_tabulated_bonds_match_oracle(make_gpu, make_oracle, prec):
    """SURVEY f-1: bond func 8 (Tabulated(itype=1) on a FixedPairList).  The polymer melt with its harmonic bonds
    replaced by a table of a stiff anharmonic bond (two table handles: a plain list and a typed list share the
    registry), forces, energies and a short trajectory against the oracle."""
    spec = W.polymer_melt(n_chains=128, chain_len=32, seed=3)
    bonds = spec["lists"][0]["ids"]
    spec["lists"] = spec["lists"][1:]                                  # keep the angles
    dr = 0.001
    r = dr * np.arange(1, 2001)
    e = 2.0e4 * (r - 0.7) ** 2 + 1.0e5 * (r - 0.7) ** 4
    f = -(4.0e4 * (r - 0.7) + 4.0e5 * (r - 0.7) ** 3)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    for eng in (g, o):
        t0 = eng.table_create(r[0], dr, e, f)
        t1 = eng.table_create(r[0], dr, 0.5 * e, 0.5 * f)
        h = eng.list_create(2, "TABULATED"); eng.list_set_params(h, [t0]); eng.list_add(h, bonds[::2])
        ht = eng.list_create(2, "TABULATED", True); eng.list_set_params(ht, [t1], types=(0, 0)); eng.list_add(ht, bonds[1::2])
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (1e-10 if prec == 64 else TOL_STIFF32)
    og, oo = g.observe(), o.observe()
    assert np.allclose(og["epot_list"][:3], oo["epot_list"][:3], rtol=1e-10 if prec == 64 else 1e-4)
    assert oo["epot_list"][1] > 0 and oo["epot_list"][2] > 0
    g.run(25); o.run(25)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-8 if prec == 64 else 1e-4)
    from chemlab_amd.engine import ChemError
    with pytest.raises(ChemError):
        g.list_set_params(h, [7.0])                                     # not a table handle


@pytest.mark.parametrize("prec", [64, 32])
def test_tabulated_angles_match_oracle(make_gpu, make_oracle, prec):
    """SURVEY f-1: angle func 8 (TabulatedAngular): the polymer melt with its harmonic angles replaced by a table."""
    spec = W.polymer_melt(n_chains=128, chain_len=32, seed=4)
    angles = spec["lists"][1]["ids"]
    spec["lists"] = spec["lists"][:1]                                  # keep the bonds
    dth = np.pi / 720
    th = dth * np.arange(1, 721)
    th0 = np.deg2rad(119.0)
    e = 244.0 * (th - th0) ** 2 + 30.0 * (th - th0) ** 4
    f = -(488.0 * (th - th0) + 120.0 * (th - th0) ** 3)
    g, o, _ = both(make_gpu, make_oracle, spec, prec, thermostat=False)
    for eng in (g, o):
        h = eng.list_create(3, "ANG_TABULATED"); eng.list_set_params(h, [eng.table_create(th[0], dth, e, f)]); eng.list_add(h, angles)
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < (1e-10 if prec == 64 else TOL_STIFF32)
    og, oo = g.observe(), o.observe()
    assert np.allclose(og["epot_list"][:2], oo["epot_list"][:2], rtol=1e-10 if prec == 64 else 1e-4)
    assert oo["epot_list"][1] > 0
    g.run(25); o.run(25)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < (1e-8 if prec == 64 else 1e-4)


@pytest.mark.parametrize("kind,param,transport", [("berendsen", 0.05, None), ("isokinetic", 4, None), ("berendsen", 0.05, "dd_self")])
def test_rescaling_thermostats_match_oracle(make_gpu, make_oracle, kind, param, transport):
    """SURVEY f-1: BerendsenThermostat / Isokinetic -- global kinetic energy reduction + scaling pass every (k-th) step."""
    spec = W.lj_melt(n=8788, seed=31, jitter=0.08, kT=1.5)
    spec["rebuild_criterion"] = 0
    g, o = make_gpu(64), make_oracle()
    if transport:
        g.set_option(transport, 1)
    W.apply(spec, g, thermostat=False); W.apply(spec, o, thermostat=False)
    for e in (g, o):
        e.thermostat_rescale(kind, 0.9, param)
    g.run(60); o.run(60)
    assert g.observe()["temperature"] == pytest.approx(o.observe()["temperature"], rel=1e-9)
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-8
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    for e in (g, o):
        e.thermostat_rescale(None, 1.0, 1.0)
    g.run(10); o.run(10)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("transport", [None, "dd_self"])
def test_stochastic_velocity_rescaling_matches_oracle(make_gpu, make_oracle, transport):
    """SURVEY f-1: StochasticVelocityRescaling (thermostat = vr): kinetic-energy reduction, ONE keyed scalar draw per step
    on the device (include/chem_philox.h svr_lambda, the same code the oracle runs), scaling pass."""
    spec = W.lj_melt(n=8788, seed=33, jitter=0.08, kT=1.5)
    spec["rebuild_criterion"] = 0
    g, o = make_gpu(64), make_oracle()
    if transport:
        g.set_option(transport, 1)
    W.apply(spec, g, thermostat=False); W.apply(spec, o, thermostat=False)
    for e in (g, o):
        e.thermostat_svr(0.9, 0.05, 5)
    g.run(60); o.run(60)
    assert g.observe()["temperature"] == pytest.approx(o.observe()["temperature"], rel=1e-9)
    assert rel_err(g.get_state("VEL"), o.get_state("VEL")) < 1e-8
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9
    assert abs(g.observe()["temperature"] - 0.9) < 0.1        # it does thermostat (started at 1.5)
    for e in (g, o):
        e.thermostat_svr(0.9, 0.0, 5)
    g.run(10); o.run(10)
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("nearest", [True, False])
def test_max_per_interval_matches_oracle(make_gpu, make_oracle, nearest):
    """SURVEY f-4: ChemicalReaction.max_per_interval -- the same capped event set on the HIP path and the oracle."""
    spec = W.reactive_melt(n=8788, seed=15, interval=10)
    spec["reaction"] = dict(spec["reaction"], max_per_interval=25, nearest=nearest)
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    g.run(30); o.run(30)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) == 75
    assert [e[:4] for e in eg] == [e[:4] for e in eo]
    assert np.array_equal(g.get_list(h["reaction_bonds"]), o.get_list(h["reaction_bonds"]))
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))


@pytest.mark.gpu
def test_change_neighbours_property_matches_oracle(make_gpu, make_oracle):
    """SURVEY f-4: PostProcessChangeNeighboursProperty on the trimer melt (atrp_lj shape): coupling of two MA ends turns the
    middle beads (one bond away) into a new type with state 1 and the far ends (two bonds away) into another."""
    spec = W.trimer_melt(n_mol=216, seed=6, interval=20)
    MA, ML, PA, PL = 0, 1, 2, 3
    spec["lj"] += [(PA, t, 1.0, 1.0, spec["rc"]) for t in (MA, ML, PA)] + [(PL, t, 1.0, 1.0, spec["rc"]) for t in (MA, ML, PA, PL)]
    g, o = make_gpu(64), make_oracle()
    for e in (g, o):
        W.apply(spec, e)
        e.reaction_neighbour_change(0, "both", ML, 1, PL, 1.5, new_state=1)
        e.reaction_neighbour_change(0, "both", MA, 2, PA, 2.0)
    g.run(60); o.run(60)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 10 and [e[:4] for e in eg] == [e[:4] for e in eo]
    tg, to = g.get_state("TYPE"), o.get_state("TYPE")
    assert (to == PL).sum() > 0 and (to == PA).sum() > 0
    assert np.array_equal(tg, to)
    assert np.array_equal(g.get_state("STATE"), o.get_state("STATE"))
    assert np.allclose(g.get_state("MASS"), o.get_state("MASS"))
    assert rel_err(g.get_state("POS_UNFOLDED"), o.get_state("POS_UNFOLDED")) < 1e-8
    g.run(0); o.run(0)
    assert rel_err(g.get_state("FORCE"), o.get_state("FORCE")) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("nranks", [2, 3])
def test_bench_multi_process_over_ipc_on_one_gpu(tmp_path, nranks):
    """The REAL multi-process flow of `bench.py --gpus N` (torchrun rendezvous, one process per rank, per-rank set-up,
    collective order, teardown) on the one leased GPU: RCCL refuses several ranks on a device, the hipIpc transport
    (chem_comm_init_ipc) does not.  The event count and the particle total must equal the single-domain run's."""
    import json, socket, subprocess, sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", CHEM_TRANSPORT="ipc")
    common = ["--steps", "40", "--warmup", "10", "--particles", "64000", "--interval", "20", "--equil", "100", "--cpu-steps", "0", "--f64-steps", "0"]
    if nranks == 2:
        # the way the driver starts it: plainly -- bench.py spawns the ranks itself (a child torch.distributed.run)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(nranks)] + common
        env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(nranks)] + common
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == nranks and d["steps"] == 40 and d["value"] > 0 and d["config"]["transport"] == "ipc"
    assert d["config"]["reaction_steps_timed"] == 2 and d["config"]["reaction_events"] > 0
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--precision", "32", "--no-roofline"] + common,
                         capture_output=True, text=True, timeout=900, env=dict(os.environ), cwd=str(tmp_path))
    assert one.returncode == 0, one.stderr[-3000:]
    d1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    # fp32 trajectories of different decompositions differ in the last bits (summation order), the chemistry of a
    # melt this size over 2 reaction steps stays statistically the same: same order of magnitude of events
    assert 0.5 < d["config"]["reaction_events"] / float(d1["config"]["reaction_events"]) < 2.0


@pytest.mark.gpu
def test_destroying_a_decomposed_context_with_work_in_flight(make_oracle):
    """Round-1 abort (`Memory critical error ... Memory in use` at exit, host segfault inside chem_run): the decomposed
    path's decision kernel writes its verdict into PINNED HOST words (hflag); a context destroyed while such a kernel was
    still queued freed those words under it.  ~CtxT now drains the stream before hipHostFree.  This test destroys
    dd_self contexts right after queueing steps, with no explicit sync, several times in a row."""
    from chemlab_amd.engine import Engine
    spec = W.reactive_melt(n=32000, seed=21, interval=7)
    for k in range(6):
        e = Engine(device=0, precision=32)
        e.set_option("dd_self", 1)
        W.apply(spec, e)
        e.run(5 + 3 * k)          # returns with the last launches possibly still executing
        e.close()                 # chem_destroy: no chem_device_sync before it
    e = Engine(device=0, precision=32)      # the device is still healthy afterwards
    W.apply(spec, e)
    e.run(3)
    assert np.isfinite(e.get_state("FORCE")).all()
    e.close()


@pytest.mark.gpu
def test_excluded_pairs_are_not_reaction_candidates(make_gpu, make_oracle):
    """Candidates are pairs of the Verlet list (reaction_setup.py:416: ChemicalReaction(system, vl, ...)): a pair that is
    excluded from it -- here: already bonded -- never reacts, even while its types and states still fit a reaction."""
    spec = W.reactive_melt(n=8788, seed=17, interval=5)
    for r in spec["reaction"]["reactions"]:          # state windows that stay open after an event: re-reaction possible
        r["min_state_1"], r["max_state_1"], r["min_state_2"], r["max_state_2"], r["delta_1"], r["delta_2"] = 0, 100, 0, 100, 0, 0
        r["is_virtual"] = False
        r.pop("new_type_2", None)
        r["intramolecular"] = True
    g, o, h = both(make_gpu, make_oracle, spec, 64)
    g.run(20); o.run(20)
    eg, eo = sorted_events(g.get_events()), sorted_events(o.get_events())
    assert len(eo) > 1000
    assert [e[:4] for e in eg] == [e[:4] for e in eo]
    pairs = [(min(e[1], e[2]), max(e[1], e[2])) for e in eo]
    assert len(pairs) == len(set(pairs))             # no pair reacted twice
    assert np.array_equal(g.get_list(h["reaction_bonds"]), o.get_list(h["reaction_bonds"]))


def test_force_list_is_a_thin_superset_of_the_exact_list(make_gpu, make_oracle):
    """fp32 list build: the expanded-form distance test admits a shell of ~5e-5 beyond rc+skin (list build);
    the 16-bit force list must contain every active, non-excluded pair of the oracle's Verlet list and nothing
    farther out than that shell.  (Types: reactive_melt switches the A-B and A-D potentials off.)"""
    spec = W.reactive_melt(n=8788, seed=13)
    g, o, _ = both(make_gpu, make_oracle, spec, 32, thermostat=False, reactions=False)
    g.run(0); o.run(0)
    pos = o.get_state("POS"); L = np.array(spec["box"]); rl = spec["rc"] + spec["skin"]
    typ = o.get_state("TYPE").astype(int).ravel()
    pairs = o.get_verlet_pairs() - 1      # particle ids (1..n here) -> tags
    assert pairs.min() == 0
    nb = {}
    for a, b in pairs.tolist():
        nb.setdefault(a, set()).add(b); nb.setdefault(b, set()).add(a)
    f_ref = o.get_state("FORCE")
    checked = 0
    for tag in range(0, spec["n"], 97):
        lst = g.debug_force_list(tag)
        assert len(set(lst.tolist())) == len(lst)
        d = pos[lst] - pos[tag]; d -= L * np.round(d / L)
        r = np.sqrt((d * d).sum(1))
        assert r.max() < rl + 2e-4
        exact = nb.get(tag, set())
        extra = set(lst.tolist()) - exact
        for j in extra:                              # only shell pairs may be extra
            dj = pos[j] - pos[tag]; dj -= L * np.round(dj / L)
            assert np.sqrt((dj * dj).sum()) > rl - 1e-5
        # pairs of the exact list that are missing carry no potential (inactive type pair): the forces agree
        checked += 1
    assert checked > 50
    assert rel_err(g.get_state("FORCE"), f_ref) < TOL[32]

