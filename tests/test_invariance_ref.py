"""The helpers of tests/invariance.py, the references under them, and the oracle under new particle names -- all on the CPU.
The scenes built here are the ones tests/test_gpu_invariance.py runs on the device.

involution     relabel followed by the inverse map gives the spec back; a cyclic permutation three times and a reflection
               twice are the identity (coordinates on a 2^-10 grid in a power-of-two box: to the bit).
references     helpers.pair_reference, aged_ref.exact_pairs, bonded_ref.reference and ptensor_ref.pressure_tensor give the
               mapped-back answer on a transformed spec: forces within 1e-13 of the largest component (fp64 sums in another
               order, nothing else), the same number of pairs, no pair in the shell of its cutoff in any orientation.
oracle         ids reach the oracle through its own id2tag map.  Names in the same ORDER with shuffled rows: the same bits in
               every per-particle array, the same events, lists and exclusions after mapping the names back.  This pins "tag =
               rank by id" on the checker's side before the device is asked the same question."""
import numpy as np
import pytest

import aged_ref as AR
import bonded_ref as B
import helpers as H
import invariance as I
import ptensor_ref as PT
import react_ref as RR
from chemlab_amd import _capi
from chemlab_amd import workloads as W
from chemlab_amd.engine import ChemError

A_, B_, D_, E_ = 0, 1, 2, 3


# ======================================================================================================================
# the scenes of part A (names)
# ======================================================================================================================
def _melt(path):
    from test_gpu_pressure import melt
    return melt("lj", path)


_SCENES = {}


def bonded_scene(path="tiles"):
    """test_gpu_pressure.melt (4096 particles on a jittered 16^3 lattice, several types, Langevin; 216 on the brute-force path)
    with the lattice columns along z cut into chains: harmonic bonds (plain on the even chains, typed on the odd ones), cosine
    angles (plain) and harmonic ones (typed, for the triples whose middle type is in the lower half), dihedrals (plain), the
    1-2 and 1-3 exclusions, thermal groups, and four calls of modify_particle between the runs."""
    if ("bonded", path) in _SCENES:
        return dict(_SCENES[("bonded", path)])
    spec = _melt(path)
    n, ty = spec["n"], spec["type_ids"]
    k = round(n ** (1.0 / 3.0))
    c = 4 if k % 4 == 0 else k
    idx = np.arange(n).reshape(-1, c) + 1
    a = float(spec["box"][0]) / k
    even, odd = idx[0::2], idx[1::2]
    tup = lambda rows, m: np.concatenate([rows[:, j:j + m] for j in range(c - m + 1)])      # noqa: E731
    lower = ty[:max(1, len(ty) // 2)]
    lists = [dict(name="bond", arity=2, kind="HARMONIC", params=[30.0, a], ids=tup(even, 2)),
             dict(name="tbond", arity=2, kind="HARMONIC", ids=tup(odd, 2), typed=[((p, q), [20.0 + p + q, 0.95 * a]) for i, p in enumerate(ty) for q in ty[i:]]),
             dict(name="ang", arity=3, kind="ANG_COSINE", params=[3.0, np.deg2rad(130.0)], ids=tup(even, 3)),
             dict(name="tang", arity=3, kind="ANG_HARMONIC", ids=tup(odd, 3), typed=[((p, m, q), [5.0, np.deg2rad(119.0 + m)]) for m in lower for i, p in enumerate(ty) for q in ty[i:]]),
             dict(name="dih", arity=4, kind="DIH_NCOS", params=[0.5, np.deg2rad(20.0), 3.0], ids=tup(idx, 4))]
    rng = np.random.default_rng(5)
    pick = rng.choice(n, 4, replace=False) + 1
    types = np.asarray(spec["types"])
    spec = dict(spec, lists=lists, exclusions=np.concatenate([tup(idx, 2), tup(idx, 3)[:, [0, 2]]]), thermal_types=[int(t) for t in ty[::2]],
                modify=[(int(pick[0]), "TYPE", float(ty[(ty.index(int(types[pick[0] - 1])) + 1) % len(ty)])), (int(pick[1]), "MASS", 2.5),
                        (int(pick[2]), "CHARGE", -0.75), (int(pick[3]), "STATE", 3.0)], run=(0, 30))
    _SCENES[("bonded", path)] = spec
    return dict(spec)


def reactive_scene(single_domain=True, n=4000):
    """workloads.reactive_melt (4000 particles, six cells per axis, or 256 in a box of the brute-force list; A + B -> A + D, A + A
    chain growth) at rate 3 with an angle
    list that spawns A-A-A, a restriction of the first A + A reaction to two thirds of the A pairs within 1.6, a neighbour
    change behind the second (the bonded A neighbours of a reactant become E), ATRP on the D, and -- single domain only: the
    decomposed path refuses them -- a dissociation rule on the reaction bonds and a region rule B -> D in a slab."""
    key = ("reactive", single_domain, n)
    if key in _SCENES:
        return dict(_SCENES[key])
    from scipy.spatial import cKDTree
    spec = W.reactive_melt(n=n, seed=23, interval=10, rate=3.0, skin=0.25)      # (skin 0.25: six cell layers along z, two per slab of three)
    L = np.asarray(spec["box"], np.float64)
    assert n < 4000 or np.floor(L / (spec["rc"] + spec["skin"])).min() >= 6
    isA = np.nonzero(spec["types"] == A_)[0]
    near = cKDTree(AR.fold(spec["pos"][isA], L), boxsize=L).query_pairs(1.6, output_type="ndarray")
    near = isA[near[np.lexsort((near[:, 1], near[:, 0]))]] + 1
    keep = near[(near[:, 0] + near[:, 1]) % 3 != 0]
    assert n // 8 < len(keep) < len(near)
    spec = dict(spec, lj=spec["lj"] + [(E_, E_, 1.0, 1.0, spec["rc"]), (A_, E_, 1.0, 1.0, spec["rc"])],
                lists=[dict(arity=3, kind="ANG_HARMONIC", params=[1.25, np.pi], ids=np.empty((0, 3), np.int64), register=[(A_, A_, A_)])],
                restrict=[(1, keep)],
                nb_change=[dict(reaction=2, invoke_on="both", old_type=A_, nb_level=1, new_type=E_, new_mass=1.5)],
                atrp=dict(interval=7, num_particles=200, ratio_activator=0.8, ratio_deactivator=0.2, delta_catalyst=0.05, k_activate=1.0, k_deactivate=1.0,
                          select_from_all=True, seed=77,
                          centers=[dict(type_id=D_, state=1, is_activator=False, new_type=D_, new_mass=1.0, delta_state=5),
                                   dict(type_id=D_, state=6, is_activator=True, new_type=D_, new_mass=1.0, delta_state=-5)]),
                run=(0, 60))
    spec["reaction"] = dict(spec["reaction"], type_mass={**spec["reaction"]["type_mass"], E_: 1.5})
    if single_domain:
        spec["dissociation"] = [dict(type_1=A_, type_2=A_, delta_1=0, delta_2=0, min_state_1=0, max_state_1=100, min_state_2=0, max_state_2=100,
                                     diss_rate=4.0, cutoff=1.5, unexclude=True)]
        spec["regions"] = [dict(lo=[0.0, 0.0, 0.0], hi=[0.5 * L[0], L[1], L[2] / 3.0], target_type=B_, new_type=D_, interval=5, mode="prob", value=0.3, seed=5)]
    _SCENES[key] = spec
    return dict(spec)


def resfix_scene():
    """test_gpu_checkpoint's everything-at-once melt (fixed distances, a typed set that releases, a resolution ramp, a hybrid bond
    list, ATRP) with chem_set_resolution on forty B, and eight particles of a type without pair terms appended by
    chem_add_particles -- their ids leave gaps above the top id -- each the target of a fixed distance to an A."""
    if "resfix" in _SCENES:
        return dict(_SCENES["resfix"])
    from test_gpu_checkpoint import _everything_spec
    spec, plain, typed, dfix = _everything_spec()
    n = spec["n"]
    rng = np.random.default_rng(9)
    used = set(np.concatenate([plain, typed]).ravel().tolist())
    isB = [i + 1 for i in np.nonzero(spec["types"] == B_)[0] if i + 1 not in used]
    isA = [i + 1 for i in np.nonzero(spec["types"] == A_)[0] if i + 1 not in used]
    lam_ids = np.asarray(rng.choice(isB, 40, replace=False), np.int64)
    anchors = np.asarray(rng.choice(isA, 8, replace=False), np.int64)
    add_ids = n + np.cumsum(rng.integers(2, 7, 8)).astype(np.int64)
    u = rng.standard_normal((8, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    add = dict(ids=add_ids, types=np.full(8, E_, np.int32), pos=spec["pos"][anchors - 1] + 0.9 * u, vel=0.3 * rng.standard_normal((8, 3)),
               mass=np.full(8, 1.25), state=np.zeros(8, np.int32), res_id=np.arange(n + 1, n + 9, dtype=np.int32))
    spec = dict(spec, lam_set=(lam_ids, np.linspace(0.2, 0.8, 40)), add=add,
                fix=[dict(anchor_type=-1, target_type=-1, pairs=plain, dist=dfix), dict(anchor_type=-1, target_type=B_, pairs=typed, dist=dfix, post=dict(old_type=D_, lam=0.25)),
                     dict(anchor_type=-1, target_type=-1, pairs=np.stack([anchors, add_ids], 1), dist=0.9)],
                hybrid_bonds=(0.0, 0.02), reaction_resolution=[(0, "type_2", 0.0)], run=(0, 53))
    _SCENES["resfix"] = spec
    return dict(spec)


ENTRY_POINTS = {"bonded": ("exclusions", "lists", "modify", "thermal_types"),
                "reactive": ("restrict", "nb_change", "atrp", "register", "dissociation", "regions"),
                "resfix": ("lam_set", "fix", "add")}


def without(spec, what):
    """the scene without one of its entry points"""
    out = dict(spec)
    if what == "register":
        out["lists"] = [{k: v for k, v in l.items() if k != "register"} for l in spec["lists"]]
    elif what == "add":
        out.pop("add")
        out["fix"] = spec["fix"][:-1]
    elif what == "exclusions":
        out["exclusions"] = None
    else:
        out.pop(what)
    return out


def apply_scene(spec, e, thermostat=True, reactions=True):
    """workloads.apply and what it does not know: typed lists, restrictions, neighbour changes, dissociation, regions, appended
    particles, fixed distances, chem_set_resolution.  Returns the handles: lists by index, "reaction_bonds", "fix" [sets]."""
    lists = spec.get("lists") or []
    plain = [i for i, l in enumerate(lists) if l.get("typed") is None]
    hp = W.apply(dict(spec, lists=[lists[i] for i in plain]), e, thermostat=thermostat, reactions=reactions)
    h = {plain[j]: hp[j] for j in range(len(plain))}
    if "reaction_bonds" in hp:
        h["reaction_bonds"] = hp["reaction_bonds"]
    for i, l in enumerate(lists):
        if l.get("typed") is not None:
            h[i] = e.list_create(l["arity"], l["kind"], True)
            for key, p in l["typed"]:
                e.list_set_params(h[i], p, types=key)
            e.list_add(h[i], l["ids"])
    if reactions and spec.get("reaction"):
        for r, pairs in spec.get("restrict", []):
            e.reaction_restrict(r, pairs)
        for nc in spec.get("nb_change", []):
            e.reaction_neighbour_change(**nc)
        for d in spec.get("dissociation", []):
            e.dissociation_add(bond_list=h["reaction_bonds"], **d)
        if spec.get("hybrid_bonds"):
            e.list_set_hybrid(h["reaction_bonds"], *spec["hybrid_bonds"])
        for rr in spec.get("reaction_resolution", []):
            e.reaction_set_resolution(*rr)
    h["regions"] = []
    for rg in spec.get("regions", []):
        h["regions"].append(e.region_add(**rg))
        e.region_enable(h["regions"][-1], True)
    if spec.get("add"):
        e.add_particles(**spec["add"])
    h["fix"] = []
    for f in spec.get("fix", []):
        s = e.fix_create(f["anchor_type"], f["target_type"])
        e.fix_add(s, f["pairs"], f["dist"])
        if f.get("post"):
            e.fix_postprocess(s, **f["post"])
        h["fix"].append(s)
    if spec.get("lam_set") is not None:
        e.set_resolution(*spec["lam_set"])
    return h


ID_FIELDS = {"events": ("id_a", "id_b"), "fix_log": ("anchor_id", "target_id"), "fix_joins": ("anchor_id", "target_id"),
             "removed": ("id_near", "id_far"), "region_changes": ("id",)}


def collect(e, h, full=True):
    """everything an engine can be asked: per-particle arrays by tag, observables, counters, lists and logs (ID_FIELDS: the
    records that carry ids); full = False leaves out what only the product has"""
    out = {k: e.get_state(k) for k in ("ID", "POS", "VEL", "FORCE", "IMAGE", "TYPE", "STATE", "RESID", "MASS", "CHARGE", "POS_UNFOLDED")}
    out["observe"] = e.observe()
    out["step"] = e.step
    t = e.timers()
    out["counters"] = (t["rebuilds"], t["list_rebuilds"], t["nlist_entries"], t["reaction_steps"])
    out["events"] = e.get_events()
    out["exclusions"] = e.get_exclusions()
    out["verlet"] = e.get_verlet_pairs()
    for k, v in h.items():
        if k not in ("fix", "regions"):
            out["list %s" % k] = e.get_list(v)
    if e.supports("atrp_get_stats"):
        out["atrp"] = e.atrp_stats()
    if full and e.supports("get_pressure"):
        out["pressure"] = e.pressure()
        out["tensor"] = e.pressure_tensor()
    if full and e.supports("set_resolution") and e.supports("fix_get"):
        out["LAMBDA"] = e.get_state("LAMBDA")
        out["fix_log"], out["fix_joins"], out["removed"] = e.fix_log(), e.fix_joins(), e.reaction_removed()
        for s in h.get("fix", []):
            out["fix %d" % s] = e.fix_get(s)
    if full and h.get("regions"):
        out["region_changes"], out["region_stats"] = e.region_changes(), e.region_stats()
    return out


def run_scene(e, spec, full=True, **kw):
    """the scene's protocol: set-up, run(first), the modify_particle calls, run(rest); a collect() behind either run"""
    h = apply_scene(spec, e, **kw)
    first, rest = spec["run"]
    e.run(first)
    a = collect(e, h, full)
    for pid, what, val in spec.get("modify", []):
        if what == "CHARGE" and not e.supports("nb_coulomb"):        # (the CPU checker keeps no charge to modify)
            continue
        e.modify_particle(pid, what, val)
    e.run(rest)
    return a, collect(e, h, full)


def _bits(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _bits(a[k], b[k], "%s[%s]" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _bits(x, y, "%s[%d]" % (what, k))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def same_under_names(a, b, m, what=""):
    """collect() of the base run `a` and of the renamed run `b`, m = IdMap base -> renamed.  The names keep their order: every
    array by tag is the same array, every record the same record under the other names, in the same order."""
    assert m.keeps_order()
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for k in a:
        w = "%s %s" % (what, k)
        if k == "ID":
            assert np.array_equal(m.inv(b[k]), a[k]), w
        elif k in ID_FIELDS:
            assert a[k].dtype == b[k].dtype and len(a[k]) == len(b[k]), w
            back = b[k].copy()
            for f in ID_FIELDS[k]:
                back[f] = m.inv(b[k][f])
            assert a[k].tobytes() == back.tobytes(), w              # every field, r2 to the bit
        elif k in ("exclusions", "verlet") or k.startswith("list "):
            assert np.array_equal(m.inv(b[k]), a[k]), w
        elif k.startswith("fix "):
            assert np.array_equal(m.inv(b[k][0]), a[k][0]) and np.array_equal(a[k][1], b[k][1]), w
        else:
            _bits(a[k], b[k], w)


def gapped(spec, seed=1, base=7):
    """A1: names 7 + cumsum(integers(1, 9)) in the old order, rows shuffled"""
    ids = I.all_ids(spec)
    return I.relabel(spec, I.gapped_ids(len(ids), seed, base), np.random.default_rng(seed + 100).permutation(len(spec["ids"])))


def reversed_names(spec):
    """A2: the names in the opposite order (with gaps): every tag changes"""
    ids = I.all_ids(spec)
    g = I.gapped_ids(len(ids), 3)
    return I.relabel(spec, g[::-1].copy()[np.argsort(np.argsort(ids))], np.random.default_rng(4).permutation(len(spec["ids"])))


def differs(a, b):
    """whether two collect() results differ anywhere (the entry point that was left out mattered)"""
    try:
        _bits({k: v for k, v in a.items() if k != "counters"}, {k: v for k, v in b.items() if k != "counters"}, "")
    except AssertionError:
        return True
    return False


# ======================================================================================================================
# involution
# ======================================================================================================================
def _random_spec(seed):
    rng = np.random.default_rng(seed)
    n = 60
    ids = np.sort(rng.choice(500, n, replace=False)) + 1
    L = np.array([8.0, 16.0, 4.0])
    g = lambda m: rng.choice(ids, m)      # noqa: E731
    return dict(n=n, box=L.tolist(), ids=ids, types=rng.integers(0, 3, n).astype(np.int32), pos=rng.integers(0, 4096, (n, 3)) * (L / 4096.0),
                vel=rng.standard_normal((n, 3)), mass=rng.uniform(1, 2, n), state=rng.integers(0, 3, n).astype(np.int32), res_id=rng.integers(1, 9, n).astype(np.int32),
                q=rng.uniform(-1, 1, n), lam=rng.uniform(0, 1, n), exclusions=g(20).reshape(-1, 2),
                lists=[dict(arity=a, kind="X", params=[1.0], ids=g(a * 7).reshape(-1, a)) for a in (2, 3, 4)],
                restrict=[(0, g(10).reshape(-1, 2))], fix=[dict(pairs=g(6).reshape(-1, 2), dist=1.0)], modify=[(int(ids[3]), "TYPE", 1.0)],
                lam_set=(g(5), rng.uniform(0, 1, 5)), add=dict(ids=np.array([900, 910]), pos=rng.integers(0, 4096, (2, 3)) * (L / 4096.0), vel=rng.standard_normal((2, 3))),
                regions=[dict(lo=[1.0, 2.0, 0.5], hi=[3.0, 9.0, 2.5], target_type=0)])


def _same_spec(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            _same_spec(x, y, what + k)
        elif isinstance(x, (list, tuple)) and x and isinstance(x[0], (dict, tuple, list)):
            for u, v in zip(x, y):
                _same_spec(u, v, what + k) if isinstance(u, dict) else [np.testing.assert_array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(u, v)]
        elif isinstance(x, tuple) and isinstance(x[0], np.ndarray):
            for p, q in zip(x, y):
                np.testing.assert_array_equal(p, q)
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=what + k)


@pytest.mark.parametrize("seed", range(3))
def test_relabel_then_inverse_gives_the_spec_back(seed):
    spec = _random_spec(seed)
    rng = np.random.default_rng(seed)
    order = rng.permutation(spec["n"])
    new = rng.permutation(10 ** 10 + 3 * np.arange(spec["n"] + 2))       # beyond 32 bits, in another order
    s1, m = I.relabel(spec, new, order)
    assert not m.keeps_order() and not np.array_equal(s1["ids"], spec["ids"])
    assert np.array_equal(m.inv(s1["ids"]), spec["ids"][order]) and np.array_equal(s1["pos"], spec["pos"][order])
    assert np.array_equal(m.inv(s1["lists"][1]["ids"]), spec["lists"][1]["ids"]) and np.array_equal(m.inv(s1["add"]["ids"]), spec["add"]["ids"])
    s2, m2 = I.relabel(s1, m.inv(I.all_ids(s1)), np.argsort(order))
    _same_spec(spec, s2)
    assert np.array_equal(m2.fwd(new), m.inv(new))
    assert I.relabel(spec, I.gapped_ids(spec["n"] + 2, seed), order)[1].keeps_order()


@pytest.mark.parametrize("seed", range(3))
def test_axis_maps_are_involutions(seed):
    spec = _random_spec(seed)
    for perm in I.CYCLIC:
        s, maps = spec, []
        for _ in range(3):
            s, am = I.permute_axes(s, perm)
            maps.append(am)
        _same_spec(spec, s)
        s1, am = I.permute_axes(spec, perm)
        assert s1["box"] == [spec["box"][p] for p in perm] and np.array_equal(s1["pos"][:, 0], spec["pos"][:, perm[0]])
        assert np.array_equal(am.back_vec(s1["vel"]), spec["vel"]) and np.array_equal(am.back_vec(am.vec(spec["vel"])), spec["vel"])
        t = np.random.default_rng(seed).standard_normal((4, 6))
        assert np.array_equal(am.back_tensor6(am.tensor6(t)), t) and not np.array_equal(am.tensor6(t), t)
    for axis in range(3):
        s1, am = I.reflect(spec, axis)
        s2, _ = I.reflect(s1, axis)
        _same_spec(spec, s2)
        L = spec["box"][axis]
        assert np.array_equal(np.mod(s1["pos"][:, axis] + spec["pos"][:, axis], L), np.zeros(spec["n"])) and np.all(s1["pos"] >= 0) and np.all(s1["pos"][:, axis] < L)
        assert np.array_equal(s1["vel"][:, axis], -spec["vel"][:, axis])
        t = np.arange(1.0, 7.0)
        sg = np.ones(6)
        sg[[c for c, (a, b) in enumerate(I.TENSOR) if (a == axis) != (b == axis)]] = -1.0
        assert np.array_equal(am.tensor6(t), sg * t) and np.array_equal(am.back_tensor6(am.tensor6(t)), t)


def test_tensor_map_is_the_map_of_an_outer_product():
    rng = np.random.default_rng(2)
    u, w = rng.standard_normal(3), rng.standard_normal(3)
    six = lambda p, q: np.array([0.5 * (p[a] * q[b] + p[b] * q[a]) for a, b in I.TENSOR])      # noqa: E731
    for how, _ in I.ORIENTATIONS:
        _, am = I.orient(dict(box=[1.0, 2.0, 4.0]), how)
        assert np.allclose(am.tensor6(six(u, w)), six(am.vec(u), am.vec(w)), rtol=0, atol=1e-15)
        assert np.allclose(am.back_tensor6(six(am.vec(u), am.vec(w))), six(u, w), rtol=0, atol=1e-15)


# ======================================================================================================================
# the references under the helpers
# ======================================================================================================================
def aniso_melt():
    """5 x 6 x 7 cells (helpers.geometry_spec): two types, LJ on 0-0, a table on 0-1 and 1-1, disjoint nearest-neighbour pairs
    bonded by one harmonic list and excluded.  The seed is the first whose pairs stay out of the shell of every cutoff in all
    six orientations (test_no_pair_in_the_shell_of_a_cutoff_in_any_orientation)."""
    if "aniso" in _SCENES:
        return _SCENES["aniso"]
    from scipy.spatial import cKDTree
    for seed in range(7700, 7720):
        spec = H.geometry_spec((5, 6, 7), 0.5, "uniform", seed=seed, ranks=(2,))
        n, L = spec["n"], np.asarray(spec["box"], np.float64)
        r0, dr, e, f = W.synthetic_table(rc=1.5)
        spec = {k: v for k, v in spec.items() if k not in ("pairs", "min_gap", "shell_pairs")}
        spec.update(types=(np.arange(n) % 2).astype(np.int32), lj=[(0, 0, 1.0, 1.0, spec["rc"])], tables=[(0, 1, r0, dr, e, f, 1.5), (1, 1, r0, dr, e, f, 1.4)])
        near = cKDTree(AR.fold(spec["pos"], L), boxsize=L).query_pairs(1.25, output_type="ndarray")
        near = near[np.lexsort((near[:, 1], near[:, 0]))]
        used, take = np.zeros(n, bool), []
        for i, j in near:
            if not used[i] and not used[j]:
                used[i] = used[j] = True
                take.append((i, j))
        bonds = np.asarray(take, np.int64) + 1
        assert len(bonds) > n // 4
        spec.update(exclusions=bonds, lists=[dict(name="harm", kind="HARMONIC", arity=2, params=[30.0, 1.0], ids=bonds)])
        if all(AR.exact_pairs(I.orient(spec, how)[0], I.orient(spec, how)[0]["pos"])["shell_pairs"] == 0 for how, _ in I.ORIENTATIONS):
            _SCENES["aniso"] = spec
            return spec
    raise AssertionError("no seed keeps every pair out of the shell")


def tight_probes(flat=False):
    """aged_ref's closing pairs at the workload's own skin (rebuild criterion 0): the cubic box of 17 cells, or the flat one"""
    return AR.tight_closing_pairs_flat(AR.TIGHT_SKIN) if flat else AR.tight_closing_pairs(AR.TIGHT_SKIN, AR.TIGHT_BOX / 17)


@pytest.mark.parametrize("how", [h for h, _ in I.ORIENTATIONS])
def test_no_pair_in_the_shell_of_a_cutoff_in_any_orientation(how):
    """The cutoff shell condition of every scene of part B, at the positions the scene starts from (the device tests assert it
    again at the engine's own positions): with no pair within 2e-6 of its cutoff fp32 is allowed no flip at all."""
    for name, spec in (("aniso", aniso_melt()), ("tight", tight_probes()), ("tight_flat", tight_probes(True))):
        s, am = I.orient(spec, how)
        for x in (s["pos"], np.asarray(s["pos"]) + s.get("M", 0) * s["dt"] * np.asarray(s["vel"])):      # (the probes: in free flight to their M-th step)
            ref = AR.exact_pairs(s, x)
            assert ref["shell_pairs"] == 0, (name, how)
        base = AR.exact_pairs(spec, spec["pos"])
        assert AR.exact_pairs(s, s["pos"])["npairs"] == base["npairs"] > 0, (name, how)


@pytest.mark.parametrize("how", [h for h, _ in I.ORIENTATIONS if h != "id"])
def test_references_give_the_mapped_back_answer(how):
    """The anisotropic melt turned and renamed (gapped ids, shuffled rows) against itself: every reference the device tests lean
    on.  fp64 sums in another order and nothing else: 1e-13 of the largest force component (of the part's scale)."""
    spec = aniso_melt()
    s, am = I.orient(spec, how)
    s, m = gapped(s, seed=11)
    order = np.argsort(m.inv(s["ids"]))                        # rows of the renamed spec in the order of the base ids (1 .. n: the base rows)
    assert np.array_equal(m.inv(s["ids"])[order], spec["ids"])
    back = lambda f: am.back_vec(f)[order]                     # noqa: E731
    # exact pair sum (ids enter through the exclusions): forces, energies, pair counts
    a, b = AR.exact_pairs(spec, spec["pos"]), AR.exact_pairs(s, s["pos"])
    assert np.abs(back(b["f"]) - a["f"]).max() <= 1e-13 * a["fmax"] and (a["npairs"], a["shell_pairs"]) == (b["npairs"], b["shell_pairs"])
    assert abs(a["epot_lj"] - b["epot_lj"]) <= 1e-13 * abs(a["epot_lj"]) and abs(a["epot_tab"] - b["epot_tab"]) <= 1e-13 * abs(a["epot_tab"])
    unexcluded = AR.exact_pairs(dict(spec, exclusions=np.empty((0, 2), np.int64)), spec["pos"])
    assert unexcluded["npairs"] == a["npairs"] + len(spec["exclusions"])                      # the renamed exclusions name the same pairs
    assert np.array_equal(H.canonical_pairs(m.inv(H.brute_pairs(s)[0])), H.brute_pairs(spec)[0])      # identical pair sets
    # all-pairs reference (it knows no exclusions)
    fa, fb = H.pair_reference(spec)[0], H.pair_reference(s)[0]
    assert np.abs(back(fb) - fa).max() <= 1e-13 * np.abs(fa).max()
    # bonded reference and pressure tensor index by id - 1: the lists go back through the map, the rows into id order
    lists = [dict(l, ids=m.inv(l["ids"])) for l in s["lists"]]
    assert all(np.array_equal(u["ids"], v["ids"]) for u, v in zip(lists, spec["lists"]))
    sb = dict(s, ids=spec["ids"], exclusions=m.inv(s["exclusions"]), **{k: np.asarray(s[k])[order] for k in ("types", "pos", "vel", "mass")})
    ra, rb = B.reference(spec["pos"], spec["box"], spec["types"], spec["lists"]), B.reference(sb["pos"], sb["box"], sb["types"], lists)
    assert np.abs(am.back_vec(rb["force"]) - ra["force"]).max() <= 1e-13 * np.abs(ra["force"]).max() and np.allclose(ra["energy"], rb["energy"], rtol=1e-13, atol=0)
    ta, tb = PT.pressure_tensor(spec, spec["pos"], spec["vel"], lists=spec["lists"]), PT.pressure_tensor(sb, sb["pos"], sb["vel"], lists=lists)
    for k in ("kinetic", "virial_nb", "virial_list", "virial", "tensor"):
        scale = ta[k + "_scale"] if k + "_scale" in ta else ta["scale"] / (ta["volume"] if k == "tensor" else 1.0)
        assert np.all(np.abs(am.back_tensor6(tb[k]) - ta[k]) <= 1e-13 * scale.max()), (how, k)
    assert PT.distinct(ta["virial_nb"], 1e-10, ta["virial_nb_scale"]) and PT.distinct(ta["kinetic"], 1e-10, ta["kinetic_scale"])      # a swap of two components would show


ZOO_BRUTE = list(RR.SMALL)


def oriented_member(name, how):
    """react_ref.member for the member turned into orientation `how`: (spec, per-step [(events, info, snapshot)]), once"""
    key = ("zoo", name, how)
    if key not in _SCENES:
        spec = I.orient(RR.member(name)[0], how)[0]
        ref, out = RR.Reference(spec), []
        iv, each = spec["reaction"]["interval"], spec.get("run_each", spec["reaction"]["interval"])
        for k in range(1, spec["steps"] + 1):          # (the loop of react_ref.member)
            ev, info = ref.step(k * each, model=True) if (k * each) % iv == 0 else ([], {})
            if ref.atrp is not None and (k * each) % ref.atrp["interval"] == 0:
                info["atrp"] = ref.atrp_fire(k * each)
            out.append((ev, info, ref.snapshot()))
        _SCENES[key] = (spec, out)
    return _SCENES[key]


def against_oriented_reference(name, how, got):
    """test_react_ref.check_against_reference with the oriented member's reference"""
    spec, ref = oriented_member(name, how)
    want_ev = []
    for k, ((ev, info, snap), (gev, gsnap)) in enumerate(zip(ref, got)):
        want_ev += RR.ref_events(ev)
        assert gev == want_ev, (name, how, k, len(gev), len(want_ev), sorted(set(gev) ^ set(want_ev))[:6])
        for key, val in snap.items():
            assert np.array_equal(np.asarray(gsnap[key]), val), (name, how, k, key)


@pytest.mark.parametrize("how", [h for h, _ in I.ORIENTATIONS if h != "id"])
def test_reaction_zoo_is_the_same_zoo_in_every_orientation(how):
    """Power-of-two boxes and coordinates on the 2^-10 grid survive the transforms exactly, and the three squares of a distance
    add up without rounding in any order: the reference gives the same events with r2 to the bit, and the same snapshots."""
    for name in list(RR.ZOO) + ZOO_BRUTE:
        spec, ref = oriented_member(name, how)
        assert RR.on_grid(spec) and np.array_equal(W.snap_to_grid(spec)["pos"], spec["pos"]), (name, how)
        for (ev, _, snap), (ev0, _, snap0) in zip(ref, RR.member(name)[1]):
            assert RR.ref_events(ev) == RR.ref_events(ev0), (name, how)
            assert snap.keys() == snap0.keys() and all(np.array_equal(snap[k], snap0[k]) for k in snap), (name, how)


def reversed_chain():
    """react_ref.chain (rate 1e9: every candidate is accepted; nearest; frozen) under reversed names, rows in id order"""
    spec = RR.member("chain")[0]
    renamed, m = reversed_names(spec)
    renamed = I.relabel(renamed, I.all_ids(renamed), np.argsort(renamed["ids"]))[0]
    return spec, renamed, m


def unordered_events(ev, m=None):
    f = (lambda x: int(m.inv(np.array([x]))[0])) if m is not None else int
    return sorted((int(s), min(f(a), f(b)), max(f(a), f(b)), int(r), float(d2).hex()) for s, a, b, r, d2 in ev)


def test_reversed_names_same_reaction_step_without_ties():
    """The no-tie condition of part A2, and what follows from it: no two candidates of the chain share a distance, so neither
    the tie-breaks by tag nor the role of the lower tag decide anything, and the reference picks the same pairs under reversed
    names."""
    spec, renamed, m = reversed_chain()
    assert not m.keeps_order()
    ra, rb = RR.Reference(spec), RR.Reference(renamed)
    iv = spec["reaction"]["interval"]
    (eva, ia), (evb, ib) = ra.step(iv), rb.step(iv)
    assert len({c[3] for c in ia["cand"]}) == len(ia["cand"]) == len(ib["cand"]) > 100              # no distance ties among the candidates
    assert all(r["delta_1"] == r["delta_2"] for r in spec["reaction"]["reactions"])                 # (the roles carry nothing)
    assert unordered_events(eva) == unordered_events(evb, m) and len(eva) > 50
    assert np.array_equal(ra.snapshot()["state"], rb.snapshot()["state"][::-1])


# ======================================================================================================================
# the oracle under new names
# ======================================================================================================================
def _oracle_scene(name):
    if name == "bonded":
        return bonded_scene("tiles")
    return reactive_scene(single_domain=False)      # (the checker has neither dissociation nor region rules)


@pytest.mark.parametrize("name", ["bonded", "reactive"])
def test_oracle_same_bits_under_order_preserving_names(make_oracle, name):
    spec = _oracle_scene(name)
    renamed, m = gapped(spec)
    assert m.keeps_order() and not np.array_equal(renamed["ids"], np.sort(renamed["ids"])) and renamed["ids"].max() > 2 * spec["n"]
    a0, a1 = run_scene(make_oracle(), spec)
    b0, b1 = run_scene(make_oracle(), renamed)
    same_under_names(a0, b0, m, name + " first:")
    same_under_names(a1, b1, m, name + " last:")
    assert not np.array_equal(a1["POS"], a0["POS"])
    if name == "reactive":
        print("reactive: %d events, %d bonds, %d angles, %d ATRP rows" % (len(a1["events"]), len(a1["list reaction_bonds"]), len(a1["list 0"]), len(a1["atrp"])))
        assert len(a1["events"]) > 50 and len(a1["list 0"]) > 0 and (a1["TYPE"] == E_).any()


@pytest.mark.parametrize("name", ["bonded", "reactive"])
def test_oracle_every_entry_point_matters(make_oracle, name):
    spec = _oracle_scene(name)
    full = run_scene(make_oracle(), spec)[1]
    for what in ENTRY_POINTS[name]:
        if what in spec or what == "register":
            assert differs(full, run_scene(make_oracle(), without(spec, what))[1]), (name, what)


def test_oracle_reversed_names_same_forces(make_oracle):
    """Names in the opposite order: every tag changes, the forces at run(0) agree to reordering (1e-12 of the largest)."""
    spec = dict(bonded_scene("tiles"), run=(0, 0))
    renamed, m = reversed_names(spec)
    assert not m.keeps_order()
    a = run_scene(make_oracle(), spec, thermostat=False)[0]
    b = run_scene(make_oracle(), renamed, thermostat=False)[0]
    back = np.argsort(m.inv(b["ID"]))
    assert np.array_equal(m.inv(b["ID"])[back], a["ID"])
    assert np.abs(b["FORCE"][back] - a["FORCE"]).max() <= 1e-12 * np.abs(a["FORCE"]).max()
    assert np.array_equal(b["TYPE"][back], a["TYPE"]) and np.array_equal(H.canonical_pairs(m.inv(b["exclusions"])), H.canonical_pairs(a["exclusions"]))
    assert np.allclose(b["observe"]["epot_list"], a["observe"]["epot_list"], rtol=1e-12, atol=0)


def test_oracle_ids_beyond_32_bits(make_oracle):
    """The default res_id and CHEM_STATE_MOLID are int32 labels made of ids: refused by name for ids that do not fit, and
    everything else works with such ids."""
    spec = dict(bonded_scene("brute"), run=(0, 10))
    big, m = I.relabel(spec, 2 ** 33 + I.gapped_ids(spec["n"], 2), np.random.default_rng(1).permutation(spec["n"]))
    o = make_oracle()
    with pytest.raises(ChemError, match="default res_id") as e:
        apply_scene(dict(big, res_id=None), o)
    assert e.value.code == _capi.EINVAL
    o = make_oracle()
    b = run_scene(o, big)[1]
    with pytest.raises(ChemError, match="CHEM_STATE_MOLID") as e:
        o.get_state("MOLID")
    assert e.value.code == _capi.EINVAL
    same_under_names(run_scene(make_oracle(), spec)[1], b, m, "big ids:")
    assert b["exclusions"].min() > 2 ** 33 and b["verlet"].min() > 2 ** 33
