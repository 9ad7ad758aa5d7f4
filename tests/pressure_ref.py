"""The pressure and the Berendsen barostat restated in fp64 (include/chem_mi355.h "pressure and barostat"): the reference of
tests/test_pressure_ref.py (CPU) and tests/test_gpu_pressure.py / tests/test_gpu_barostat.py (device).  No engine in here.

    P = (sum_i m_i v_i^2 + W) / (3 V),   W = sum r.F over every registered interaction.

W is computed two independent ways:
  virial_rf        sum over pairs of r_ij . F_ij: the non-bonded pairs from a periodic k-d tree with helpers.pair_eval (the sum
                   aged_ref.exact_pairs forms), the pair lists with the force as minus the gradient of bonded_ref's energies with
                   respect to the separation VECTOR;
  virial_scaling   -dU/dlambda at lambda = 1 of U(lambda x, lambda L), by torch autograd over the same energies (all arities:
                   angles and dihedrals give 0 to rounding).
Every term comes with the sum of the absolute values of its contributions: the scale the comparisons use, so that a W whose
terms nearly cancel does not hide an error.

npt_step is velocity Verlet plus the barostat rule with exact forces:  mu = [1 - (dt / tau)(P0 - P)]^(1/3),  L <- mu L,
x <- mu x, velocities and forces untouched (the next half kick uses the forces from before the scaling)."""
import numpy as np
import torch

import aged_ref
import bonded_ref
import helpers as H

F64 = torch.float64


def mv2(mass, vel):
    return float((np.asarray(mass, np.float64)[:, None] * np.asarray(vel, np.float64) ** 2).sum())


def nonbonded_rf(spec, pos, box=None):
    """(W, sum |terms|) of the non-bonded matrix of `spec` at `pos` (in `box`, default the spec's)."""
    from scipy.spatial import cKDTree
    L = np.asarray(spec["box"] if box is None else box, dtype=np.float64)
    x = aged_ref.fold(pos, L)
    types = np.asarray(spec["types"])
    ids = np.asarray(spec["ids"], dtype=np.int64)
    prm = H.pair_params(spec)
    coul = spec.get("coulomb", [])              # (t1, t2, prefactor, rc): k q_i q_j / r inside rc on top of the pair's LJ / table: r.F = U
    if not prm and not coul:
        return 0.0, 0.0
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
    w = a = 0.0
    for (t1, t2), p in prm.items():
        if t1 > t2:
            continue
        m = ((ta == t1) & (tb == t2)) | ((ta == t2) & (tb == t1))
        ff, _ = H.pair_eval(p, r2[m])
        w += float((ff * r2[m]).sum())
        a += float(np.abs(ff * r2[m]).sum())
    for (t1, t2, k, rc) in coul:
        q = np.asarray(spec["q"], np.float64)
        m = (((ta == t1) & (tb == t2)) | ((ta == t2) & (tb == t1))) & (r2 <= rc * rc)
        t = k * q[ij[m, 0]] * q[ij[m, 1]] / np.sqrt(r2[m])
        w += float(t.sum())
        a += float(np.abs(t).sum())
    return w, a


def _pair_energy(lst, r, P, q=None, idx=None):
    """Energy per entry of a pair list at the distances r (a tensor)."""
    if lst["kind"] == "COULOMB_BOND":            # (prefactor, cutoff): k q_i q_j / r inside the cutoff, no shift
        qq = torch.as_tensor(q[idx[:, 0]] * q[idx[:, 1]], dtype=F64)
        u = P[:, 0] * qq / r
        return torch.where(r <= P[:, 1], u, torch.zeros_like(u))
    m = r.shape[0]
    x = torch.cat([torch.stack([r, torch.zeros_like(r), torch.zeros_like(r)], 1), torch.zeros((m, 3), dtype=F64)])
    fake = torch.stack([torch.arange(m), torch.arange(m) + m], 1)
    return bonded_ref._energy(lst["kind"], x, torch.full((3,), 1e9, dtype=F64), fake, P, lst.get("table"))


def _weights(lst, m):
    lam = lst.get("lam")
    return torch.ones(m, dtype=F64) if lam is None else torch.as_tensor(np.broadcast_to(np.asarray(lam, np.float64), (m,)).copy(), dtype=F64)


def lists_rf(pos, box, types, lists, q=None):
    """[(W_l, sum |terms|)] per list: r_ij . F_ij of every entry of a pair list (times its lambda, lst["lam"], if any); triples
    and quadruples are (0, 0) -- they depend on angles alone."""
    x = np.asarray(pos, np.float64)
    L = np.asarray(box, np.float64)
    out = []
    for lst in lists:
        idx, P = bonded_ref.resolve(lst, types)
        if lst["arity"] != 2 or len(idx) == 0:
            out.append((0.0, 0.0))
            continue
        d0 = x[idx[:, 0]] - x[idx[:, 1]]
        d0 -= L * np.rint(d0 / L)
        d = torch.tensor(d0, dtype=F64, requires_grad=True)
        u = (_weights(lst, len(idx)) * _pair_energy(lst, d.norm(dim=1), torch.as_tensor(P, dtype=F64), q, idx)).sum()
        f = -torch.autograd.grad(u, d)[0]
        t = (d.detach() * f).sum(1).numpy()
        out.append((float(t.sum()), float(np.abs(t).sum())))
    return out


def lists_scaling(pos, box, types, lists, q=None):
    """[-dU_l/dlambda at lambda = 1] per list, positions and box scaled together (every arity)."""
    out = []
    for lst in lists:
        idx, P = bonded_ref.resolve(lst, types)
        if len(idx) == 0:
            out.append(0.0)
            continue
        lam = torch.tensor(1.0, dtype=F64, requires_grad=True)
        x = torch.tensor(np.asarray(pos, np.float64), dtype=F64) * lam
        L = torch.tensor(np.asarray(box, np.float64), dtype=F64) * lam
        Pt, it = torch.as_tensor(P, dtype=F64), torch.as_tensor(idx)
        if lst["arity"] == 2:
            r = bonded_ref._mi(x[it[:, 0]] - x[it[:, 1]], L).norm(dim=1)
            u = (_weights(lst, len(idx)) * _pair_energy(lst, r, Pt, q, idx)).sum()
        else:
            u = bonded_ref._energy(lst["kind"], x, L, it, Pt, lst.get("table")).sum()
        g = torch.autograd.grad(u, lam, allow_unused=True)[0]
        out.append(0.0 if g is None else -float(g))
    return out


def lj_scaling(spec, pos, box=None):
    """-dU/dlambda at lambda = 1 of the LJ part of the spec's matrix (tables have no autograd form here: a spec with tables is
    refused).  The set of pairs inside their cutoff is taken at lambda = 1: the shifted energy is continuous there."""
    from scipy.spatial import cKDTree
    assert not spec.get("tables")
    L0 = np.asarray(spec["box"] if box is None else box, dtype=np.float64)
    x0 = aged_ref.fold(pos, L0)
    types = np.asarray(spec["types"])
    prm = H.pair_params(spec)
    ij = cKDTree(x0, boxsize=L0).query_pairs(max(p[3] for p in prm.values()), output_type="ndarray")
    lam = torch.tensor(1.0, dtype=F64, requires_grad=True)
    x, L = torch.tensor(x0, dtype=F64) * lam, torch.tensor(L0, dtype=F64) * lam
    d = bonded_ref._mi(x[ij[:, 0]] - x[ij[:, 1]], L)
    r = d.norm(dim=1)
    eps, sig, rc = (np.array([prm.get((int(a), int(b)), ("lj", 0.0, 1.0, 0.0, 0.0))[k] for a, b in zip(types[ij[:, 0]], types[ij[:, 1]])]) for k in (1, 2, 3))
    inside = torch.as_tensor(r.detach().numpy() <= rc)
    u = torch.where(inside, bonded_ref._lj(r, torch.as_tensor(eps), torch.as_tensor(sig)), torch.zeros_like(r)).sum()
    return -float(torch.autograd.grad(u, lam)[0])


def pressure(spec, pos, vel, box=None, lists=(), q=None):
    """dict(pressure, volume, mv2, virial_nb, virial_list, virial, scale): `scale` = mv2 + the sums of |terms| of every part."""
    L = np.asarray(spec["box"] if box is None else box, dtype=np.float64)
    k = mv2(spec["mass"], vel)
    wnb, anb = nonbonded_rf(spec, pos, L)
    wl = lists_rf(aged_ref.fold(pos, L), L, spec["types"], lists, q)
    w = wnb + sum(t[0] for t in wl)
    vol = float(np.prod(L))
    return dict(pressure=(k + w) / (3.0 * vol), volume=vol, mv2=k, virial_nb=wnb, virial_nb_scale=anb, virial_list=[t[0] for t in wl],
                virial_list_scale=[t[1] for t in wl], virial=w, scale=k + anb + sum(t[1] for t in wl))


def mu3(dt, tau, p0, p):
    return 1.0 - (dt / tau) * (p0 - p)


def npt_step(spec, x, v, f, L, force_fn, dt, tau, p0):
    """One step of velocity Verlet with the barostat behind it.  x unfolded, f the forces the step starts with; force_fn(x, L)
    -> (forces, W).  Returns (x', v', f', L', P): f' are the forces at x(t+dt) BEFORE the scaling, x' and L' are scaled."""
    m = np.asarray(spec["mass"], np.float64)[:, None]
    v = v + 0.5 * dt * f / m
    x = x + dt * v
    f, w = force_fn(x, L)
    v = v + 0.5 * dt * f / m
    p = (float((m * v * v).sum()) + w) / (3.0 * float(np.prod(L)))
    m3 = mu3(dt, tau, p0, p)
    if not m3 > 0:
        raise ArithmeticError("Berendsen barostat: mu^3 = %g <= 0" % m3)
    mu = np.cbrt(m3)
    return x * mu, v, f, L * mu, p


def exact_force_fn(spec):
    """force_fn of npt_step for a spec with non-bonded terms only: aged_ref.exact_pairs at the given box."""
    def fn(x, L):
        r = aged_ref.exact_pairs(dict(spec, box=L), x)
        return r["f"], r["virial_nb"]
    return fn


# ---- the cold lattice of the lists-under-scaling tests (tests/test_gpu_barostat.py; its guard: tests/test_pressure_ref.py) ----
# a thin skin, so that the scalings use it up before the cell count changes: shrink starts at 5.31 cells of rc + skin = 2.6 with
# the (2, 1, 1) shell at 2.6026, just outside the list radius -- 4 % of compression bring it inside rc, 5.9 % cross the threshold
COLD_RC, COLD_SKIN, COLD_SIDE = 2.5, 0.1, 13
COLD_SPACING = {"shrink": 17.0 / 16.0, "grow": 125.0 / 128.0}
COLD_DP, COLD_RATE = 400.0, 3e-3            # P0 = P(start) +- COLD_DP; tau such that |mu^3 - 1| = COLD_RATE at the start: |mu - 1| = 1e-3


def cold_lattice(direction):
    """13^3 particles on a simple cubic lattice, displaced by multiples of 1 / 512 (exactly representable in fp32 and fp64; net
    forces of the size of a pair force), zero velocities.  shrink: 5.31 cells of rc + skin per axis; grow: 4.88."""
    a = COLD_SPACING[direction]
    n = COLD_SIDE ** 3
    rng = np.random.default_rng(13)
    grid = np.stack(np.meshgrid(*[np.arange(COLD_SIDE)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = (grid + 0.5) * a + rng.integers(-32, 33, (n, 3)) / 512.0
    L = COLD_SIDE * a
    return dict(name="cold", n=n, box=np.array([L] * 3), rc=COLD_RC, skin=COLD_SKIN, dt=0.00025, ids=np.arange(1, n + 1), types=np.zeros(n, np.int32),
                pos=pos, vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32),
                lj=[(0, 0, 1.0, 1.0, COLD_RC)], tables=[], kT=0.0, gamma=0.0, seed=1)


def cold_coupling(spec, direction):
    """(P0, tau) of the lists-under-scaling runs."""
    p_start = pressure(spec, spec["pos"], spec["vel"])["pressure"]
    return p_start + (COLD_DP if direction == "shrink" else -COLD_DP), spec["dt"] * COLD_DP / COLD_RATE
