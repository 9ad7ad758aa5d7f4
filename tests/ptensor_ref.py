"""The pressure tensor restated in fp64 (include/chem_mi355.h "pressure tensor"): the reference of tests/test_ptensor_ref.py
(CPU) and tests/test_gpu_ptensor.py (device).  No engine in here, and nothing of the kernels.

    Pi_ab = (K_ab + W_ab) / V,   components in the order ORDER = xx, yy, zz, xy, xz, yz,
    K_ab = sum_i m_i v_i,a v_i,b,   W_ab = sum d_a F_b over every registered interaction.

W is computed two independent ways from the same FIXED minimum-image vectors:
  direct    the non-bonded pairs from a periodic k-d tree with helpers.pair_eval (the sum aged_ref.exact_pairs forms), or from
            the pair records of capped_ref.total where caps or resolution weights are on: d (x) f d.  The lists from
            bonded_ref's energies: every entry is laid out around its centre from its minimum-image vectors -- pair (d, 0),
            triple (d_ij, 0, d_kj), quadruple (-b1, 0, b2, b2 + b3) -- the forces on its members are minus the autograd gradient,
            and W = sum over the members of (place relative to the centre) (x) (force).
  strain    -dU/d eps_ab at eps = 0 of the same energies with every fixed vector deformed d -> (1 + eps) d, by torch autograd,
            for all nine eps: the full 3 x 3 matrix, whose antisymmetric part has to vanish.  Lists: bonded_ref's energies.  LJ
            and Coulomb pairs: their energies written in torch (pairs_strain_energy).  Tables, caps and resolution weights have
            no energy form here: pairs_strain checks the contraction alone for them, from a surrogate with the same slope.
Every sum comes with the sum of the absolute values of its terms, per component: the scale the comparisons use."""
import numpy as np
import torch

import aged_ref
import bonded_ref
import helpers as H
import pressure_ref as PR

F64 = torch.float64
ORDER = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
NAMES = ("xx", "yy", "zz", "xy", "xz", "yz")


def six(m):
    """the six components of (..., 3, 3) matrices in ORDER (a <= b: the upper triangle)"""
    m = np.asarray(m)
    return np.stack([m[..., a, b] for a, b in ORDER], -1)


def _sum_abs(terms):
    """terms (m, 3, 3) -> (sum[6], sum of |terms|[6])"""
    t = six(np.asarray(terms, np.float64).reshape(-1, 3, 3))
    return t.sum(0), np.abs(t).sum(0)


def kinetic(mass, vel):
    m, v = np.asarray(mass, np.float64), np.asarray(vel, np.float64)
    return _sum_abs(m[:, None, None] * v[:, :, None] * v[:, None, :])


# ---- non-bonded pairs ---------------------------------------------------------------------------------------------------------
def nonbonded_pairs(spec, pos, box=None, laws=False):
    """(d (m, 3), fs (m,)) of every non-bonded term of `spec` at `pos`: F_i = fs d with d = x_i - x_j at the minimum image.  A
    pair with an LJ / table term and a Coulomb term appears twice.  laws = True: a third array (m, 3) with the law of every
    term, (0, eps, sigma) LJ, (1, k q_i q_j, 0) Coulomb, (2, 0, 0) table, for the terms inside their cutoff (fs != 0)."""
    from scipy.spatial import cKDTree
    L = np.asarray(spec["box"] if box is None else box, dtype=np.float64)
    x = aged_ref.fold(pos, L)
    types = np.asarray(spec["types"])
    ids = np.asarray(spec["ids"], dtype=np.int64)
    prm = H.pair_params(spec)
    coul = spec.get("coulomb", [])
    if not prm and not coul:
        return (np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3))) if laws else (np.zeros((0, 3)), np.zeros(0))
    ij = cKDTree(x, boxsize=L).query_pairs(max([H.pair_cutoff(p) for p in prm.values()] + [c[3] for c in coul]), output_type="ndarray")
    ex = spec.get("exclusions")
    if ex is not None and len(ex):
        ex = np.sort(np.asarray(ex, dtype=np.int64).reshape(-1, 2), 1)
        key = np.minimum(ids[ij[:, 0]], ids[ij[:, 1]]) * (ids.max() + 1) + np.maximum(ids[ij[:, 0]], ids[ij[:, 1]])
        ij = ij[~np.isin(key, ex[:, 0] * (ids.max() + 1) + ex[:, 1])]
    d = x[ij[:, 0]] - x[ij[:, 1]]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(1)
    ta, tb = types[ij[:, 0]], types[ij[:, 1]]
    ds, fs, lw = [np.zeros((0, 3))], [np.zeros(0)], [np.zeros((0, 3))]
    for (t1, t2), p in prm.items():
        if t1 > t2:
            continue
        m = ((ta == t1) & (tb == t2)) | ((ta == t2) & (tb == t1))
        ff, _ = H.pair_eval(p, r2[m])
        ds.append(d[m])
        fs.append(np.asarray(ff, np.float64))
        lw.append(np.tile([0.0, p[1], p[2]] if p[0] == "lj" else [2.0, 0.0, 0.0], (int(m.sum()), 1)))
    for (t1, t2, k, rc) in coul:                # k q_i q_j / r inside rc: F_i = (U / r^2) d
        q = np.asarray(spec["q"], np.float64)
        m = (((ta == t1) & (tb == t2)) | ((ta == t2) & (tb == t1))) & (r2 <= rc * rc)
        ds.append(d[m])
        fs.append(k * q[ij[m, 0]] * q[ij[m, 1]] / r2[m] ** 1.5)
        lw.append(np.stack([np.ones(int(m.sum())), k * q[ij[m, 0]] * q[ij[m, 1]], np.zeros(int(m.sum()))], 1))
    if laws:
        return np.concatenate(ds), np.concatenate(fs), np.concatenate(lw)
    return np.concatenate(ds), np.concatenate(fs)


def pairs_direct(d, fs):
    """(W[6], sum |terms|[6]) of pair terms F_i = fs d: d (x) fs d"""
    return _sum_abs(fs[:, None, None] * d[:, :, None] * d[:, None, :])


def pairs_strain(d, fs):
    """the 3 x 3 matrix -dU/d eps of the same terms: each pair's energy is taken to first order around its own distance, with
    slope -fs r, so that autograd supplies nothing but the chain rule through |(1 + eps) d|"""
    eps = torch.zeros((3, 3), dtype=F64, requires_grad=True)
    dv = torch.as_tensor(np.asarray(d, np.float64)) @ (torch.eye(3, dtype=F64) + eps).T
    r = dv.norm(dim=1)
    r0 = r.detach()
    u = (-(torch.as_tensor(np.asarray(fs, np.float64)) * r0) * (r - r0)).sum()
    return -torch.autograd.grad(u, eps)[0].numpy()


def pairs_strain_energy(d, fs, laws):
    """the 3 x 3 matrix -dU/d eps of LJ and Coulomb terms from their ENERGIES, written here in torch: 4 eps (s^12 - s^6) (the shift
    is a constant) and k q_i q_j / r over the pairs inside their cutoff at eps = 0 (the set is fixed: the derivative of a
    truncated term is taken inside).  Owes the direct route nothing but the pairs; tables have no energy form here."""
    inside = np.asarray(fs) != 0.0
    assert not np.any(laws[inside, 0] == 2.0)
    eps = torch.zeros((3, 3), dtype=F64, requires_grad=True)
    r = (torch.as_tensor(np.asarray(d, np.float64)[inside]) @ (torch.eye(3, dtype=F64) + eps).T).norm(dim=1)
    kind, p1, p2 = (torch.as_tensor(laws[inside, k]) for k in range(3))
    s6 = (torch.where(kind == 0, p2, torch.ones_like(p2)) / r) ** 6
    u = torch.where(kind == 0, 4.0 * p1 * (s6 * s6 - s6), p1 / r).sum()
    return -torch.autograd.grad(u, eps)[0].numpy()


# ---- lists --------------------------------------------------------------------------------------------------------------------
def _layout(x, L, idx, arity):
    """the members of every entry relative to its centre (member 1), from the minimum-image vectors: (m, arity, 3)"""
    mi = lambda v: v - L * np.rint(v / L)
    z = np.zeros((len(idx), 3))
    if arity == 2:
        return np.stack([mi(x[idx[:, 0]] - x[idx[:, 1]]), z], 1)
    if arity == 3:
        return np.stack([mi(x[idx[:, 0]] - x[idx[:, 1]]), z, mi(x[idx[:, 2]] - x[idx[:, 1]])], 1)
    b1, b2, b3 = mi(x[idx[:, 1]] - x[idx[:, 0]]), mi(x[idx[:, 2]] - x[idx[:, 1]]), mi(x[idx[:, 3]] - x[idx[:, 2]])
    return np.stack([-b1, z, b2, b2 + b3], 1)


def _list_energy(lst, P, place, q, idx):
    """energy per entry with the members at `place` (m, arity, 3), a tensor: bonded_ref's energies in a box without images"""
    m, ar = place.shape[0], place.shape[1]
    flat = place.reshape(m * ar, 3)
    fake = torch.arange(m * ar).reshape(m, ar)
    far = torch.full((3,), 1e9, dtype=F64)
    if ar == 2:
        r = (place[:, 0] - place[:, 1]).norm(dim=1)
        return PR._weights(lst, m) * PR._pair_energy(lst, r, P, q, idx)
    return bonded_ref._energy(lst["kind"], flat, far, fake, P, lst.get("table"))


def lists_direct(pos, box, types, lists, q=None):
    """[(W[6], sum |terms|[6])] per list, every arity; terms = entries"""
    x, L = np.asarray(pos, np.float64), np.asarray(box, np.float64)
    out = []
    for lst in lists:
        idx, P = bonded_ref.resolve(lst, types)
        if len(idx) == 0:
            out.append((np.zeros(6), np.zeros(6)))
            continue
        place = torch.tensor(_layout(x, L, idx, lst["arity"]), dtype=F64, requires_grad=True)
        u = _list_energy(lst, torch.as_tensor(P, dtype=F64), place, q, idx).sum()
        f = -torch.autograd.grad(u, place)[0].numpy()
        p = place.detach().numpy()
        out.append(_sum_abs((p[:, :, :, None] * f[:, :, None, :]).sum(1)))
    return out


def lists_strain(pos, box, types, lists, q=None):
    """[3 x 3 matrix -dU_l/d eps] per list"""
    x, L = np.asarray(pos, np.float64), np.asarray(box, np.float64)
    out = []
    for lst in lists:
        idx, P = bonded_ref.resolve(lst, types)
        if len(idx) == 0:
            out.append(np.zeros((3, 3)))
            continue
        eps = torch.zeros((3, 3), dtype=F64, requires_grad=True)
        place = torch.as_tensor(_layout(x, L, idx, lst["arity"])) @ (torch.eye(3, dtype=F64) + eps).T
        u = _list_energy(lst, torch.as_tensor(P, dtype=F64), place, q, idx).sum()
        out.append(-torch.autograd.grad(u, eps)[0].numpy())
    return out


# ---- the whole ----------------------------------------------------------------------------------------------------------------
def pressure_tensor(spec, pos, vel, box=None, lists=(), q=None, pairs=None):
    """dict(volume, kinetic, virial_nb, virial_list, virial, tensor: arrays of six (virial_list: (lists, 6)), and *_scale beside
    each: the sums of |terms|; `scale` = all of them together).  pairs: (d, fs) of the non-bonded terms where the spec's matrix
    is not helpers' (caps, resolution weights: the records of capped_ref.total)."""
    L = np.asarray(spec["box"] if box is None else box, dtype=np.float64)
    k, ka = kinetic(spec["mass"], vel)
    d, fs = nonbonded_pairs(spec, pos, L) if pairs is None else pairs
    wnb, anb = pairs_direct(d, fs)
    wl = lists_direct(aged_ref.fold(pos, L), L, spec["types"], lists, q)
    vl = np.array([t[0] for t in wl]).reshape(len(wl), 6)
    al = np.array([t[1] for t in wl]).reshape(len(wl), 6)
    w = wnb + vl.sum(0)
    vol = float(np.prod(L))
    return dict(volume=vol, kinetic=k, kinetic_scale=ka, virial_nb=wnb, virial_nb_scale=anb, virial_list=vl, virial_list_scale=al,
                virial=w, tensor=(k + w) / vol, scale=ka + anb + al.sum(0))


def distinct(values, tol, scale):
    """the probes' condition: the six components differ pairwise by more than 1000 tol scale (scale: per component; the larger
    of the two counts)"""
    v, s = np.asarray(values, np.float64), np.asarray(scale, np.float64)
    return all(abs(v[a] - v[b]) > 1000.0 * tol * max(s[a], s[b]) for a in range(6) for b in range(a + 1, 6))


# ---- oriented probes ----------------------------------------------------------------------------------------------------------
# Isolated two-particle clusters in a sparse box, each along a direction of its own near (1, 2, 3), and every term of a part with
# the same sign (all pairs repulsive, all bonds stretched), so that nothing cancels: the six components of every part then go
# like (1, 4, 9, 2, 3, 6) / 14 of its scale, no two agree, and a swapped or transposed component shows.  The triples and quadruples of
# the probes are bonded_ref's zoo, whose members are rotated at random and sit on faces, edges and the corner as well.
PROBE_RC, PROBE_SKIN = 1.5, 0.3
PROBE_BOX = {"big": (9.0, 9.9, 10.9), "brute": (5.0, 5.2, 5.3)}      # cells per axis 5, 5, 6 (three slabs of two layers) / fewer than three
DIRS = ((1, 2, 3), (3, -1, 2), (-2, 3, 1), (1, -3, 2), (2, 1, -3), (-1, 2, -3), (3, 2, 1), (-3, 1, 2), (2, -3, -1))
PROBE_LJ = (1.0, 1.0, PROBE_RC)            # eps, sigma, cutoff of the 0-0 and 2-2 pairs
PROBE_COUL = (138.935485, 1.4)             # prefactor, cutoff of the 2-2 Coulomb term
PROBE_CAP, PROBE_FMAX = 0.95, 25.0         # cap radius of the 0-0 pairs; max_force of the marked 1-1 pairs
# cluster kinds per context: (name, type of both members, separation)
PROBE_KINDS = {
    "plain": (("lj", 0, 1.0), ("tab", 1, 0.9), ("harm", 3, 1.0), ("fene", 3, 0.8), ("hyb", 3, 1.1)),
    "coulomb": (("coul", 2, 1.1), ("lj", 0, 1.0), ("coul", 2, 1.25)),
    "rescap": (("cap", 0, 0.85), ("res", 1, 1.0), ("cap", 0, 1.2), ("res", 1, 0.8)),      # inside / outside the cap radius; below / above max_force
}
HYB_LAMBDA0 = 0.37


def probe_table():
    """(r0, dr, e, f) of the 1-1 table: a soft well, rows at 0.3 + 0.01 k up to the cutoff"""
    r = 0.3 + 0.01 * np.arange(121)
    return 0.3, 0.01, 2.0 * (r - 1.0) ** 2 - 0.5, -4.0 * (r - 1.0)


def probe_spec(context, box="big"):
    """The two-particle probes of one context ("plain", "coulomb", "rescap") on a grid of sites whose first site of every axis
    sits on the face: site (0, 0, 0) straddles the corner, (0, 0, k) an edge, (0, j, k) a face.  Velocities s_i (1, 2, 3)."""
    if context == "bonded":
        return probe_bonded_spec(box)
    L = np.asarray(PROBE_BOX[box], np.float64)
    m = 3 if box == "big" else 2
    pitch = L / m
    sites = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    kinds = PROBE_KINDS[context]
    pos, types, lam, q, entries = [], [], [], [], {}
    for s, site in enumerate(sites):
        name, ty, r = kinds[s % len(kinds)]
        r *= 1.0 + 0.02 * (s % 4)                   # (no two clusters of a kind alike: nothing cancels between them)
        u = np.array([1.0, 2.0, 3.0]) + 0.1 * np.asarray(DIRS[s % len(DIRS)], np.float64)      # near (1, 2, 3), every cluster its own
        u /= np.sqrt(u @ u)
        c = site * pitch + 0.01 * np.asarray(DIRS[(s + 4) % len(DIRS)])
        i = len(pos)
        pos += [c + 0.5 * r * u, c - 0.5 * r * u]
        types += [ty, ty]
        lam += [0.6, 0.7] if s % 8 < 4 else [0.9, 1.0]
        q += [0.5 + 0.1 * (s % 3), 0.8 - 0.1 * (s % 4)]
        entries.setdefault(name, []).append((i + 1, i + 2) if s % 2 == 0 else (i + 2, i + 1))
    n = len(pos)
    pos = aged_ref.fold(np.asarray(pos), L)
    sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    vel = (0.1 * (1 + np.arange(n) % 7) * sgn)[:, None] * np.array([1.0, 2.0, 3.0])
    spec = dict(name="probe_" + context, n=n, box=L, rc=PROBE_RC, skin=PROBE_SKIN, dt=0.001, ids=np.arange(1, n + 1), types=np.asarray(types, np.int32),
                pos=pos, vel=vel, mass=1.0 + 0.25 * (np.arange(n) % 3), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32),
                lj=[], tables=[], kT=0.0, gamma=0.0, seed=1, probe_lists=[], entries=entries)
    if context == "plain":
        spec["lj"] = [(0, 0) + PROBE_LJ]
        spec["tables"] = [(1, 1) + probe_table() + (PROBE_RC,)]
        bonds = lambda k: np.asarray(entries[k], np.int64)
        spec["probe_lists"] = [dict(name="harm", kind="HARMONIC", arity=2, params=[30.0, 0.9], ids=bonds("harm")),
                               dict(name="fene", kind="FENE", arity=2, params=[30.0, 0.0, 1.5], ids=bonds("fene")),
                               dict(name="hyb", kind="HARMONIC", arity=2, params=[25.0, 0.95], ids=bonds("hyb"), lam=HYB_LAMBDA0)]
    elif context == "coulomb":
        spec["lj"] = [(0, 0) + PROBE_LJ, (2, 2) + PROBE_LJ]
        spec["q"] = np.asarray(q)
        spec["coulomb"] = [(2, 2) + PROBE_COUL]
    else:
        spec["lj"] = [(0, 0) + PROBE_LJ, (1, 1) + PROBE_LJ]
        spec["caps"] = [(0, 0, PROBE_CAP)]
        spec["resolution"] = [(1, 1, PROBE_FMAX)]
        spec["lam"] = np.asarray(lam)
    return spec


def capped_pairs(spec, pos, box=None, gap=False):
    """(d, fs) of a spec with caps and / or resolution marks (probe_spec("rescap"), the melts of the capped and resolution
    tests): the pair records of capped_ref.total -- brute force over all pairs, the force that was applied.
    gap = True: instead, the smallest | r - rc | over the pairs that carry a term there, on either side of their cutoff."""
    import capped_ref
    import spline_ref
    L = np.asarray(spec["box"] if box is None else box, np.float64)
    matrix = {}
    for lj in spec.get("lj", []):
        matrix[(min(lj[0], lj[1]), max(lj[0], lj[1]))] = spline_ref.lj(*lj[2:5])
    for tb in spec.get("tables", []):
        matrix[(min(tb[0], tb[1]), max(tb[0], tb[1]))] = ("tab", spline_ref.Table(*tb[2:6], *(tb[7:8] or (1,))), tb[6])
    caps = {(min(a, b), max(a, b)): c for a, b, c in spec.get("caps", [])}
    marked = {(min(r[0], r[1]), max(r[0], r[1])): (r[2] if len(r) > 2 else 0.0) for r in spec.get("resolution", [])}
    ex = spec.get("exclusions")
    excluded = () if ex is None else [(int(a) - 1, int(b) - 1) for a, b in np.asarray(ex).reshape(-1, 2)]
    if gap:
        return capped_ref.gap_to_cutoff(aged_ref.fold(pos, L), L, spec["types"], matrix, spec.get("lam") if marked else None, marked or None, excluded)
    t = capped_ref.total(aged_ref.fold(pos, L), L, spec["types"], matrix, caps, spec.get("lam") if marked else None, marked or None, excluded)
    return t["pairs"]["d"], t["pairs"]["fs"]


# ---- oriented triples and quadruples --------------------------------------------------------------------------------------------
# One list per angular and dihedral kind of the zoo (bonded_ref._lists: the same parameters and tables), a few clusters each.
# The clusters of a kind share a base geometry well away from the minimum of their term and a base orientation, searched once on
# the CPU among seeded random rotations for the largest pairwise gap between the six reference components; each cluster then
# turns a little further about (1, 2, 3) and bends a little more, so that all are different and their terms add up.
# Bonds of 0.5: a chain spans less than a cell, so every partner is inside the ghost layer of a slab.
PROBE_BONDED = ("angh", "angc", "tabang", "ncos", "rb", "dihh_a", "tabdih")
PROBE_KINDS["bonded"] = tuple((name, 3, 0.5) for name in PROBE_BONDED)
_BOND = 0.5


def _chain(arity, k):
    """members of cluster number k of its kind, centred: bending angle 100 + 1.5 k degrees, dihedral 60 + 2 k degrees"""
    th, phi = np.deg2rad(100.0 + 1.5 * k), np.deg2rad(60.0 + 2.0 * k)
    p = [np.array([_BOND, 0.0, 0.0]), np.zeros(3), _BOND * np.array([np.cos(th), np.sin(th), 0.0])]
    if arity == 4:
        p.append(bonded_ref._place(p[0], p[1], p[2], _BOND, np.deg2rad(110.0), phi))
    p = np.array(p)
    return p - p.mean(0)


def _about_123(angle):
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _gap(w, a):
    """smallest |w_a - w_b| / max(scale_a, scale_b) over the pairs of components"""
    return min(abs(w[i] - w[j]) / max(a[i], a[j]) for i in range(6) for j in range(i + 1, 6))


import functools


@functools.lru_cache(maxsize=None)
def _base_orientation(name):
    lst = dict([l for l in bonded_ref._lists() if l["name"] == name][0])
    ar = lst["arity"]
    lst["ids"] = np.arange(1, ar + 1).reshape(1, ar)
    rng = np.random.default_rng(PROBE_BONDED.index(name) + 1)
    best, best_gap = None, -1.0
    for _ in range(64):
        rot = bonded_ref._rotation(rng)
        gaps = []
        for ks in ((0,), (0, 1), (0, 1, 2), (0, 1, 2, 3)):      # the sets of clusters a kind has in the two boxes
            x = np.concatenate([_chain(ar, k) @ (rot @ _about_123(0.05 * k)).T + 50.0 for k in ks])
            many = dict(lst, ids=np.arange(1, ar * len(ks) + 1).reshape(len(ks), ar))
            w, a = lists_direct(x, np.full(3, 100.0), np.full(len(x), 3), [many])[0]
            gaps.append(_gap(w, a))
        if min(gaps) > best_gap:
            best, best_gap = rot, min(gaps)
    return best


def probe_bonded_spec(box="big"):
    """The oriented triples and quadruples, on the sites of probe_spec (the first site of every axis on the face: corner, edges
    and faces are straddled).  Particles of type 3, which carries no pair term.  Velocities s_i (1, 2, 3)."""
    L = np.asarray(PROBE_BOX[box], np.float64)
    m = 3 if box == "big" else 2
    pitch = L / m
    sites = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3)
    defs = {l["name"]: l for l in bonded_ref._lists()}
    pos, entries = [], {}
    for s, site in enumerate(sites):
        name = PROBE_BONDED[s % len(PROBE_BONDED)]
        ar, k = defs[name]["arity"], s // len(PROBE_BONDED)
        x = _chain(ar, k) @ (_base_orientation(name) @ _about_123(0.05 * k)).T + site * pitch
        i = len(pos)
        pos += list(x)
        ids = tuple(range(i + 1, i + ar + 1))
        entries.setdefault(name, []).append(ids if s % 2 == 0 else ids[::-1])
    n = len(pos)
    sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    vel = (0.1 * (1 + np.arange(n) % 7) * sgn)[:, None] * np.array([1.0, 2.0, 3.0])
    lists = [dict(defs[name], ids=np.asarray(entries[name], np.int64)) for name in PROBE_BONDED]
    return dict(name="probe_bonded", n=n, box=L, rc=PROBE_RC, skin=PROBE_SKIN, dt=0.001, ids=np.arange(1, n + 1), types=np.full(n, 3, np.int32),
                pos=aged_ref.fold(np.asarray(pos), L), vel=vel, mass=1.0 + 0.25 * (np.arange(n) % 3), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), lj=[(0, 0) + PROBE_LJ], tables=[], kT=0.0, gamma=0.0, seed=1, probe_lists=lists, entries=entries)
