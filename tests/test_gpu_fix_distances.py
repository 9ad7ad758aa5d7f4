"""Fixed distances / by-product release on the device (include/chem_mi355.h, chem_fix_create ff.) against tests/fixdist_ref.py
(the constraint and the host bookkeeping, restated in numpy / plain Python) and tests/dynres_ref.py (lambda-scaled forces).

Systems: hosts of type 0 (LJ 0-0) on the jittered lattice of tests/test_gpu_spline_tables.py, box "a" 9.0^3 (tiled pair path,
1728 hosts) and "c" 5.4^3 (per-cell path, 343 hosts), rc 1.5, skin 0.3; every host carries two or three dummies of the
interaction-free type 1 at distances 0.30 / 0.40 / 0.35, which no thermostat touches (NVE here).  The smallest shapes that
still reach both pair paths and a resort."""
import numpy as np
import pytest

import dynres_ref as D
import fixdist_ref as FX
import spline_ref as S
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError
from conftest import rel_err
from helpers import force_error_without_cutoff_flips
from test_gpu_parity import TOL, TOL_MELT32, _HUB, _run_ranks
from test_gpu_spline_tables import BOXES, DT, RC, SKIN

pytestmark = pytest.mark.gpu

TOL_F = {64: TOL[64], 32: TOL_MELT32}
TOL_E = {64: 1e-11, 32: 1e-5}             # the energy tolerances of tests/test_gpu_resolution.py
LJ00 = (1.0, 0.5, 1.3)
LJ0Z = (1.0, 0.3, 1.3)                    # host - released molecule, lambda-scaled
DIST = (0.30, 0.40, 0.35)
HOST, DUMMY, R1, R2, Z, T5, WFIN = 0, 1, 2, 3, 4, 5, 6
MZ, MW = 0.5, 0.75


def hosts(shape, seed=1, kT=0.3, vel=True):
    box = np.array(BOXES[shape])
    rng = np.random.default_rng(seed)
    k = np.floor(box / 0.75 + 1e-9).astype(int)
    grid = np.stack(np.meshgrid(*[np.arange(m) for m in k], indexing="ij"), -1).reshape(-1, 3)
    pos = grid * 0.75 - 0.1 + rng.uniform(-0.1, 0.1, grid.shape)
    n = len(pos)
    v = rng.normal(0.0, np.sqrt(kT), (n, 3)) if vel else np.zeros((n, 3))
    spec = dict(n=n, box=box.tolist(), rc=RC, skin=SKIN, dt=DT, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32), pos=pos, vel=v,
                mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32), kT=kT, gamma=0.0, seed=1,
                rebuild_criterion=1, lj=[(HOST, HOST) + LJ00])
    return W.snap_to_grid(spec), grid, rng


def dummies(spec, ndum, rng, kT=0.3, vel=True):
    """ids, positions, velocities of ndum dummies per host (consecutive per host) and the entries (anchor index, target index,
    d) in the order they are added: all first dummies, then all second ones, ..."""
    n = spec["n"]
    u = rng.normal(size=(n, ndum, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    pos = (spec["pos"][:, None, :] + np.array(DIST[:ndum])[None, :, None] * u).reshape(-1, 3)
    v = rng.normal(0.0, np.sqrt(kT), (n * ndum, 3)) if vel else np.zeros((n * ndum, 3))
    ids = np.arange(n + 1, n + n * ndum + 1)
    entries = [(h, n + h * ndum + j, DIST[j]) for j in range(ndum) for h in range(n)]
    return dict(ids=ids, types=np.full(n * ndum, DUMMY, np.int32), pos=pos, vel=v, mass=np.full(n * ndum, 0.25),
                res_id=ids.astype(np.int32)), entries


def with_dummies(spec, dm):
    out = dict(spec)
    for k in ("ids", "types", "pos", "vel", "mass", "res_id"):
        out[k] = np.concatenate([spec[k], dm[k]])
    out["state"] = np.zeros(len(out["ids"]), np.int32)
    out["n"] = len(out["ids"])
    return out


def add_entries(g, h, entries, ndum, only=None):
    """the entries of set h, one call per dummy index (= per distance)"""
    for j in range(ndum):
        rows = [(a + 1, t + 1) for a, t, d in entries if d == DIST[j] and (only is None or a in only)]
        if rows:
            g.fix_add(h, rows, DIST[j])


def build(make_gpu, shape, ndum, prec, seed=1, vel=True):
    spec, grid, rng = hosts(shape, seed, vel=vel)
    dm, entries = dummies(spec, ndum, rng, vel=vel)
    full = with_dummies(spec, dm)
    g = make_gpu(prec)
    W.apply(full, g, thermostat=False, reactions=False)
    h = g.fix_create()
    add_entries(g, h, entries, ndum)
    return g, h, spec, full, entries


def check_distances(g, entries, box, prec, what=""):
    x = g.get_state("POS_UNFOLDED")
    err = np.abs(FX.distances(x, entries, box) - np.array([e[2] for e in entries]))
    dmin = min(e[2] for e in entries)
    bound = 1e-12 * dmin if prec == 64 else 8 * 2.0 ** -24 * max(box)
    print("%s prec %d: largest | |x_t - x_a| - d | = %.3e (bound %.3e)" % (what, prec, err.max(), bound))
    assert err.max() <= bound


# ---- 1: one step at a time ---------------------------------------------------------------------------------------------------

def test_one_step_at_a_time(make_gpu):
    """fp64, NVE; the dummies are appended with add_particles after the hosts are on the device"""
    spec, grid, rng = hosts("c", seed=2)
    dm, entries = dummies(spec, 3, rng)
    g = make_gpu(64)
    W.apply(spec, g, thermostat=False, reactions=False)
    assert g.get_state("POS").shape == (spec["n"], 3)                    # (the hosts are uploaded by now)
    g.add_particles(dm["ids"], dm["types"], dm["pos"], dm["mass"], vel=dm["vel"], res_id=dm["res_id"])
    assert g.n == spec["n"] * 4
    assert np.array_equal(g.get_state("ID"), np.arange(1, g.n + 1)) and np.array_equal(g.get_state("TYPE")[spec["n"]:], dm["types"])
    assert np.allclose(g.get_state("MASS"), np.concatenate([spec["mass"], dm["mass"]]))
    h = g.fix_create()
    add_entries(g, h, entries, 3)
    assert g.fix_count(h) == len(entries)
    pairs, dist = g.fix_get(h)
    assert [(a - 1, t - 1, d) for (a, t), d in zip(pairs.tolist(), dist.tolist())] == entries
    box, L = np.array(spec["box"]), max(spec["box"])
    g.run(0)
    t_idx, a_idx = np.array([e[1] for e in entries]), np.array([e[0] for e in entries])
    x_first = g.get_state("POS_UNFOLDED")
    ex = ev = 0.0
    for s in range(12):
        x, v, f, m = g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("FORCE"), g.get_state("MASS")
        xn, vh = FX.step_model(x, v, f, m, DT, entries, box)
        g.run(1)
        x1, v1, f1 = g.get_state("POS_UNFOLDED"), g.get_state("VEL"), g.get_state("FORCE")
        want_v = vh + 0.5 * DT * f1 / m[:, None]
        ex, ev = max(ex, np.abs(x1 - xn).max()), max(ev, np.abs(v1 - want_v).max() / np.abs(want_v).max())
        assert np.abs(f1[t_idx]).max() == 0.0                           # the dummies feel nothing: v_t = v_a (half step)
        assert np.abs(v1[t_idx] - vh[a_idx]).max() <= 1e-12 * np.abs(want_v).max()
    print("largest position error %.3e (bound %.3e), velocity error %.3e of the largest" % (ex, 1e-12 * L, ev))
    assert ex <= 1e-12 * L and ev <= 1e-12
    # guard: the targets' directions turned, so a kernel that only translated them would have shown
    r0, r1 = FX.min_image(x_first[t_idx] - x_first[a_idx], box), FX.min_image(x1[t_idx] - x1[a_idx], box)
    cosang = (r0 * r1).sum(-1) / np.linalg.norm(r0, axis=-1) / np.linalg.norm(r1, axis=-1)
    turned = np.arccos(np.clip(cosang, -1, 1))
    print("directions turned by up to %.3e rad" % turned.max())
    assert turned.max() > 1e-3


# ---- 2: many steps across resorts ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape,ndum", [("a", 2), ("c", 3)])
def test_many_steps_across_resorts(make_gpu, shape, ndum, prec):
    g, h, spec, full, entries = build(make_gpu, shape, ndum, prec)
    box = np.array(spec["box"])
    g.run(200)
    tm = g.timers()
    print("list rebuilds %d" % tm["list_rebuilds"])
    assert tm["list_rebuilds"] >= 2
    assert g.fix_count(h) == len(entries) and len(g.fix_log()) == 0
    check_distances(g, entries, box, prec, "run(200), %s" % shape)
    v = g.get_state("VEL")
    n = spec["n"]
    vt = v[n:].reshape(n, ndum, 3)
    assert all(np.array_equal(vt[:, 0], vt[:, j]) for j in range(1, ndum))       # targets of one anchor: bit-equal velocities
    if prec == 64:      # run(200) against 200 x run(1): the fused and the unfused integrate launches
        g1, h1, _, _, _ = build(make_gpu, shape, ndum, prec)
        for _ in range(200):
            g1.run(1)
        ex = np.abs(g.get_state("POS_UNFOLDED") - g1.get_state("POS_UNFOLDED")).max()
        ev = np.abs(v - g1.get_state("VEL")).max() / np.abs(v).max()
        print("run(200) against 200 x run(1): positions %.3e, velocities %.3e of the largest" % (ex, ev))
        assert ex <= TOL[64] * max(box) and ev <= TOL[64]
        check_distances(g1, entries, box, prec, "200 x run(1), %s" % shape)


# ---- 3: the hosts do not notice ------------------------------------------------------------------------------------------------

def host_reference(x, spec):
    return D.total(x, spec["box"], spec["types"], np.ones(spec["n"]), {(HOST, HOST): S.lj(*LJ00)}, {})


def compare_hosts(g, spec, prec, what):
    n = spec["n"]
    g.run(0)
    x, f, ob = g.get_state("POS")[:n], g.get_state("FORCE"), g.observe()
    ref = host_reference(x, spec)
    assert np.abs(f[n:]).max() == 0.0
    if prec == 64:
        err, flips = rel_err(f[:n], ref["F"]), 0
    else:
        err, flips = force_error_without_cutoff_flips(dict(spec, pos=x), f[:n], ref["F"], TOL_F[32], max_flips=0)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    print("%s prec %d: force rel err %.3e flips %d, epot_lj %.3e virial_nb %.3e" % (what, prec, err, flips, rel(ob["epot_lj"], ref["e_lj"]), rel(ob["virial_nb"], ref["w_nb"])))
    assert err < TOL_F[prec] and flips == 0
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec]) and ob["virial_nb"] == pytest.approx(ref["w_nb"], rel=TOL_E[prec])


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape", ["a", "c"])
def test_hosts_unaffected(make_gpu, shape, prec):
    g, h, spec, full, entries = build(make_gpu, shape, 2, prec)
    compare_hosts(g, spec, prec, "step 0")
    g.run(50)
    compare_hosts(g, spec, prec, "step 50")
    check_distances(g, entries, np.array(spec["box"]), prec, "step 50")


# ---- 4 - 6: releases ---------------------------------------------------------------------------------------------------------------

def reactive(shape, ndum, seed=3):
    """frozen hosts; disjoint lattice-neighbour pairs far from each other become R1 / R2 (x multiples of 4 and x + 1, y and z
    multiples of 3).  Returns the spec with dummies, the entries and the reacting (R1 index, R2 index) pairs from a scan of
    all R1 - R2 distances."""
    spec, grid, rng = hosts(shape, seed, vel=False)
    k = grid.max(0) + 1
    index = {tuple(c): i for i, c in enumerate(grid.tolist())}
    types = spec["types"].copy()
    for c in grid.tolist():
        if c[0] % 4 == 0 and c[0] + 1 < k[0] and c[1] % 3 == 0 and c[2] % 3 == 0:
            types[index[tuple(c)]] = R1; types[index[(c[0] + 1, c[1], c[2])]] = R2
    spec = dict(spec, types=types)
    dm, entries = dummies(spec, ndum, rng, vel=False)
    full = with_dummies(spec, dm)
    i1, i2 = np.nonzero(types == R1)[0], np.nonzero(types == R2)[0]
    d = FX.min_image(spec["pos"][i1][:, None, :] - spec["pos"][i2][None, :, :], np.array(spec["box"]))
    near = (d * d).sum(-1) < 1.0 ** 2
    assert (near.sum(0) == 1).all() and (near.sum(1) == 1).all() and len(i1) >= 4         # every R1 has exactly one R2 in reach
    pairs = sorted((int(i1[a]), int(i2[b])) for a, b in zip(*np.nonzero(near)))
    return spec, full, entries, pairs


def reactive_engine(make_gpu, full, prec, new_type_1=-1):
    g = make_gpu(prec)
    spec = dict(full, lj=[(HOST, HOST) + LJ00, (HOST, Z) + LJ0Z], resolution=[(HOST, Z, 0.0)])
    W.apply(spec, g, thermostat=False, reactions=False)
    hb = g.list_create(2, "HARMONIC")
    g.list_set_params(hb, [0.0, 0.75])                                 # (a bond that pulls on nothing: the forces stay the pair sums)
    g.reaction_init(1, True, 0, 7)
    r = g.reaction_add(R1, R2, 1, 1, 0, 1, 0, 1, 1e9, 1.0, bond_list=hb, new_type_1=new_type_1, new_mass_1=1.0)
    g.reactions_enable(True)
    return g, r


def reference_release(full, entries, pairs, rules, ndum):
    m = FX.Sets(full["n"])
    h = m.create()
    for j in range(ndum):
        assert m.add(h, [(a, t) for a, t, d in entries if d == DIST[j]], DIST[j])
    m.rules = [(0, role, h, count) for role, count in rules]
    events = sorted(pairs, key=lambda p: (min(p), max(p)))
    rel = m.release_by_reaction([x for a, b in events for x in ((0, 1, a), (0, 2, b))], 1)
    return m, h, rel


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("shape,ndum,count", [("a", 2, 1), ("c", 3, 2), ("c", 2, 3)])
def test_release_by_reaction(make_gpu, shape, ndum, count, prec):
    """the last case: a host with fewer entries (2) than `count` (3)"""
    spec, full, entries, pairs = reactive(shape, ndum)
    g, r = reactive_engine(make_gpu, full, prec)
    h = g.fix_create()
    add_entries(g, h, entries, ndum)
    g.fix_postprocess(h, DUMMY, Z, MZ, 0.0, 3, 0.5)
    g.reaction_release(r, "type_1", h, count)
    g.reaction_release(r, "type_2", h, 1)
    m, hm, rel = reference_release(full, entries, pairs, [(1, count), (2, 1)], ndum)
    g.run(1)
    ev = g.get_events()
    assert sorted((int(e["id_a"]) - 1, int(e["id_b"]) - 1) for e in ev) == pairs
    log = g.fix_log()
    got = [(int(x["step"]), int(x["set"]), int(x["anchor_id"]) - 1, int(x["target_id"]) - 1, int(x["cause"])) for x in log]
    assert got == m.records() and len(got) == len(pairs) * (min(count, ndum) + 1)
    ids, dist = g.fix_get(h)
    assert [(a - 1, t - 1, d) for (a, t), d in zip(ids.tolist(), dist.tolist())] == [e[:3] for e in m.entries(hm)]
    assert g.fix_count(h) == len(entries) - len(got)
    freed = np.array([x[3] for x in got])
    ty, ms, st, lam = g.get_state("TYPE"), g.get_state("MASS"), g.get_state("STATE"), g.get_state("LAMBDA")
    want_ty = full["types"].copy(); want_ty[freed] = Z
    want_lam = np.ones(full["n"]); want_lam[freed] = 0.5
    assert np.array_equal(ty, want_ty) and np.array_equal(lam, want_lam)
    assert np.allclose(ms[freed], MZ) and (st[freed] == 3).all() and (np.delete(st, freed)[spec["n"]:] == 0).all()
    # forces at run(0): the released molecules act through the lambda-scaled pair, which they can only do through fresh lists
    g.run(0)
    x, f, ob = g.get_state("POS"), g.get_state("FORCE"), g.observe()
    sel = np.concatenate([np.arange(spec["n"]), freed])
    ref = D.total(x[sel], spec["box"], ty[sel], lam[sel], {(HOST, HOST): S.lj(*LJ00), (HOST, Z): S.lj(*LJ0Z)}, {(HOST, Z): 0.0})
    fz = np.abs(ref["F"][spec["n"]:]).max() / np.abs(ref["F"]).max()
    print("released molecules: reference force %.3e of the largest" % fz)
    assert fz > 1e-2
    if prec == 64:
        err, flips = rel_err(f[sel], ref["F"]), 0
    else:
        s32 = dict(pos=x[sel], box=spec["box"], types=ty[sel], lj=[(HOST, HOST) + LJ00, (HOST, Z) + LJ0Z])
        err, flips = force_error_without_cutoff_flips(s32, f[sel], ref["F"], TOL_F[32], max_flips=0)
    print("prec %d: force rel err %.3e flips %d" % (prec, err, flips))
    assert err < TOL_F[prec] and flips == 0
    assert np.abs(np.delete(f, sel, axis=0)).max() == 0.0
    assert ob["epot_lj"] == pytest.approx(ref["e_lj"], rel=TOL_E[prec])
    check_distances(g, [e[:3] for e in m.entries(hm)], np.array(spec["box"]), prec, "the entries that stayed")


@pytest.mark.parametrize("prec", [64, 32])
def test_release_by_type(make_gpu, prec):
    # through modify_particle between two runs
    spec, grid, rng = hosts("c")
    dm, entries = dummies(spec, 3, rng)
    full = with_dummies(spec, dm)
    host_a, host_b = 5, 77
    g2 = make_gpu(prec)
    W.apply(full, g2, thermostat=False, reactions=False)
    h = g2.fix_create(HOST, DUMMY)
    add_entries(g2, h, entries, 3)
    g2.fix_postprocess(h, DUMMY, Z, MZ, 0.0, -1, -1.0)
    g2.run(2)
    assert len(g2.fix_log()) == 0
    g2.modify_particle(host_a + 1, "TYPE", T5)
    g2.modify_particle(entries[host_b][1] + 1, "TYPE", T5)              # ... and one target directly (no post-process matches type 5)
    assert len(g2.fix_log()) == 0                                       # (released at the start of the next run)
    g2.run(1)
    got = [(int(x["step"]), int(x["anchor_id"]) - 1, int(x["target_id"]) - 1, int(x["cause"])) for x in g2.fix_log()]
    want = sorted([(2, a, t, FX.CAUSE_TYPE) for a, t, d in entries if a == host_a] + [(2, host_b, entries[host_b][1], FX.CAUSE_TYPE)],
                  key=lambda r: [e[:2] for e in entries].index((r[1], r[2])))
    assert got == want
    ty = g2.get_state("TYPE")
    assert all(ty[t] == Z for _, a, t, _ in want if a == host_a) and ty[entries[host_b][1]] == T5
    left = [e for e in entries if (e[0], e[1]) not in {(w[1], w[2]) for w in want}]
    ids, dist = g2.fix_get(h)
    assert [(a - 1, t - 1, d) for (a, t), d in zip(ids.tolist(), dist.tolist())] == left
    g2.run(20)
    check_distances(g2, left, np.array(spec["box"]), prec, "after a release by type")
    assert len(g2.fix_log()) == len(want)
    # through a reaction that changes the host's type
    rspec, rfull, rentries, rpairs = reactive("c", 2)
    g3, r = reactive_engine(make_gpu, rfull, prec, new_type_1=T5)
    sets = {ty_: g3.fix_create(ty_, DUMMY) for ty_ in (HOST, R1, R2)}
    for ty_, hs in sets.items():
        add_entries(g3, hs, rentries, 2, only=set(np.nonzero(rspec["types"] == ty_)[0].tolist()))
    g3.run(1)
    got = sorted((int(x["step"]), int(x["set"]), int(x["anchor_id"]) - 1, int(x["cause"])) for x in g3.fix_log())
    assert got == sorted((1, sets[R1], a, FX.CAUSE_TYPE) for a, b in rpairs for _ in range(2))
    assert g3.fix_count(sets[R2]) == 2 * len(rpairs) and g3.fix_count(sets[HOST]) == 2 * int((rspec["types"] == HOST).sum())


@pytest.mark.parametrize("prec", [64, 32])
def test_ramp_and_final_type(make_gpu, prec):
    spec, full, entries, pairs = reactive("c", 3)
    g, r = reactive_engine(make_gpu, full, prec)
    g.resolution_rate(Z, 1 / 8, WFIN, MW, 0.0, 2)
    h = g.fix_create()
    add_entries(g, h, entries, 3)
    g.fix_postprocess(h, DUMMY, Z, MZ, 0.0, -1, 0.0)
    g.reaction_release(r, "type_1", h, 1)
    g.run(1)
    freed = np.array([int(x["target_id"]) - 1 for x in g.fix_log()])
    assert len(freed) == len(pairs) and (g.get_state("TYPE")[freed] == Z).all()
    left = [e for e in entries if e[1] not in set(freed.tolist())]
    full_step = D.s_full(0.0, 1, 1 / 8)
    assert full_step == 9
    for s in range(2, 12):
        g.run(1)
        lam, ty = g.get_state("LAMBDA"), g.get_state("TYPE")
        assert np.array_equal(lam[freed], np.full(len(freed), D.lam(0.0, 1, 1 / 8, s)))
        assert (ty[freed] == (Z if s < full_step else WFIN)).all()
        assert np.array_equal(np.delete(lam, freed), np.ones(full["n"] - len(freed)))
        check_distances(g, left, np.array(spec["box"]), prec, "step %d" % s)
    assert np.allclose(g.get_state("MASS")[freed], MW) and (g.get_state("STATE")[freed] == 2).all()
    assert g.fix_count(h) == len(left)


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------

def refused(code, call, *words):
    with pytest.raises(ChemError) as e:
        call()
    assert e.value.code == code and len(str(e.value)) > 20
    for w in words:
        assert w in str(e.value)


def test_refusals(make_gpu):
    spec, grid, rng = hosts("c")
    dm, entries = dummies(spec, 2, rng)
    n = spec["n"]
    g = make_gpu(64)
    refused(_capi.ESTATE, lambda: g.add_particles(dm["ids"], dm["types"], dm["pos"], dm["mass"]))       # before set_particles
    W.apply(spec, g, thermostat=False, reactions=False)
    refused(_capi.EINVAL, lambda: g.add_particles([n, n + 1], [1, 1], np.zeros((2, 3)), 1.0), "greater", str(n))      # ids not above the maximum
    refused(_capi.EINVAL, lambda: g.add_particles([n + 1], [16], np.zeros((1, 3)), 1.0), "CHEM_MAX_TYPES")
    refused(_capi.EINVAL, lambda: g.add_particles([n + 1, n + 1], [1, 1], np.zeros((2, 3)), 1.0), "duplicate")
    assert g.n == n
    g.add_particles(dm["ids"], dm["types"], dm["pos"], dm["mass"], vel=dm["vel"])           # (before the first upload)
    assert g.n == 3 * n
    h = g.fix_create(HOST, DUMMY)
    g.fix_add(h, [(1, n + 1), (1, n + 2)], 0.3)
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, n + 1)], 0.3), "target")                # a second live entry for one target
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, 1)], 0.3), "anchor")                    # a target that is an anchor
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(n + 1, n + 3)], 0.3), "target")            # an anchor that is a target
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, n + 3)], 0.0), "positive")
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, n + 3)], -0.3), "positive")
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, n + 3)], float("nan")), "positive")
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, 2)], 0.3), "one particle")
    refused(_capi.EINVAL, lambda: g.fix_add(h, [(2, 10 * n)], 0.3), "unknown")
    refused(_capi.EINVAL, lambda: g.fix_add(h + 1, [(2, n + 3)], 0.3), "unknown set")
    refused(_capi.EINVAL, lambda: g.fix_postprocess(h, DUMMY, Z, MZ, 0.0, -1, 1.5), "lambda")
    refused(_capi.EINVAL, lambda: g.reaction_release(0, 1, h, 1), "chem_reaction_add")
    assert g.fix_count(h) == 2
    for _ in range(_capi.CHEM_MAX_FIX_SETS - 1):
        g.fix_create()
    refused(_capi.ENOSPC, lambda: g.fix_create(), "CHEM_MAX_FIX_SETS")
    g.run(1)
    refused(_capi.ESTATE, lambda: g.add_particles([3 * n + 1], [1], np.zeros((1, 3)), 1.0), "step 0")
    g.fix_add(h, [(2, n + 3)], 0.3)                                                          # entries may be added between runs
    g.run(1)
    assert g.fix_count(h) == 3 and len(g.fix_log()) == 0
    # two in-process ranks: no entries under a decomposition, and no decomposition over entries
    engs = [make_gpu(64) for _ in range(2)]
    _HUB[0] += 1
    hub = _HUB[0]
    full = with_dummies(spec, dm)

    def rank(rk):
        e = engs[rk]
        e.comm_init_local(2, rk, hub)
        W.apply(full, e, thermostat=False, reactions=False)
        hs = e.fix_create()
        refused(_capi.ENOTIMPL, lambda: e.fix_add(hs, [(1, n + 1)], 0.3), "decomposed")
        return True
    assert _run_ranks(2, rank) == [True, True]
    e = make_gpu(64)
    W.apply(full, e, thermostat=False, reactions=False)
    e.fix_add(e.fix_create(), [(1, n + 1)], 0.3)
    refused(_capi.ENOTIMPL, lambda: e.comm_init_local(2, 0, hub + 1000), "decomposed")
