"""Reference of the hybrid triple and quadruple lists (include/chem_mi355.h, chem_list_set_hybrid_tuples) for the tests: the
terms lambda_e U_e of every entry and the forces -grad(sum_e lambda_e U_e), in torch fp64 on the CPU by autograd.  The energies
are bonded_ref's (resolve and _energy are imported, not copied), so no force formula appears here either.  An entry whose
lambda is exactly 0 is left out of the sum, as the rule set says -- not multiplied: its energy need not be finite.

lambda_e comes from birth steps the TEST knows by construction (the event log of the reaction that spawned the tuple, or the
step of its list_add), never from the engine: ramp() is the one expression min(1, lambda0 + rate (step - birth)).

spawned() restates what the topology manager spawns around a new bond (chem_topology_register), with the step of every tuple,
from the bond graph and the event log alone."""
import numpy as np
import torch

from bonded_ref import F64, _energy, resolve


def ramp(lambda0, rate, step, birth):
    return np.minimum(1.0, lambda0 + rate * (step - np.asarray(birth, dtype=np.float64)))


def _aligned(lst, types, lam):
    """resolve() of the list, and lam (one value per row of lst["ids"]) for the rows it kept (a typed list drops rows)"""
    ids = np.asarray(lst["ids"], dtype=np.int64).reshape(-1, lst["arity"])
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(ids),))
    idx, P = resolve(lst, types)
    if len(idx) == len(ids):
        return idx, P, lam.copy()
    where = {tuple(r): k for k, r in enumerate((ids - 1).tolist())}
    return idx, P, lam[[where[tuple(r)] for r in idx.tolist()]]


def reference(pos, box, types, lists, lams):
    """lists: as bonded_ref.reference takes them; lams: per list, one lambda per row of its ids (or one scalar).
    Returns force (n, 3), energy per list (sum of lambda U), per_entry: per list the lambda U of every resolved row."""
    x = torch.tensor(np.asarray(pos, dtype=np.float64), dtype=F64, requires_grad=True)
    L = torch.tensor(np.asarray(box, dtype=np.float64), dtype=F64)
    total, energy, per_entry = x.sum() * 0.0, [], []
    for lst, lam in zip(lists, lams):
        idx, P, lam = _aligned(lst, types, lam)
        u = np.zeros(len(idx))
        on = np.nonzero(lam != 0.0)[0]
        if len(on):
            ue = _energy(lst["kind"], x, L, torch.as_tensor(idx[on]), torch.as_tensor(P[on], dtype=F64), lst.get("table")) * torch.as_tensor(lam[on], dtype=F64)
            total = total + ue.sum()
            u[on] = ue.detach().numpy()
        energy.append(float(u.sum()))
        per_entry.append(u)
    force = -torch.autograd.grad(total, x)[0].numpy()
    return dict(force=force, energy=np.asarray(energy), per_entry=per_entry)


def spawned(bonds0, events, types, reg3, reg4):
    """What the topology manager spawns.  bonds0: id pairs that exist before the first event; events: (step, id_a, id_b) of
    the bonds made, in log order; types: type by id - 1 AT THE TIME the tuple is matched -- a callable (step) -> array, or one
    array; reg3 / reg4: the registered type tuples.  Returns (triples, their steps, quadruples, their steps), each tuple in the
    orientation that matched (forwards first), in spawn order, the bonds of one step linked before the first of them spawns."""
    graph = {}

    def link(a, b):
        graph.setdefault(a, set()).add(b); graph.setdefault(b, set()).add(a)
    for a, b in np.asarray(bonds0, dtype=np.int64).reshape(-1, 2).tolist():
        link(a, b)
    out = {3: ([], [], set()), 4: ([], [], set())}

    def spawn(t, step, ty):
        reg = reg3 if len(t) == 3 else reg4
        tt = tuple(int(ty[i - 1]) for i in t)
        for key in reg:
            fwd, rev = tuple(key) == tt, tuple(key) == tt[::-1]
            if not (fwd or rev):
                continue
            t = tuple(t) if fwd else tuple(t[::-1])
            rows, steps, seen = out[len(t)]
            if frozenset((t, t[::-1])) not in seen:
                seen.add(frozenset((t, t[::-1])))
                rows.append(t); steps.append(step)
            return
    steps = sorted({e[0] for e in events})
    for s in steps:
        batch = [(a, b) for st, a, b in events if st == s]
        ty = types(s) if callable(types) else types
        for a, b in batch:
            link(a, b)
        for a, b in batch:
            na, nb = sorted(graph[a] - {b}), sorted(graph[b] - {a})
            for n1 in na:
                spawn((n1, a, b), s, ty)
            for m in nb:
                spawn((a, b, m), s, ty)
            for n1 in na:
                for n2 in sorted(graph[n1] - {a, b}):
                    spawn((n2, n1, a, b), s, ty)
                for m in nb:
                    if m != n1:
                        spawn((n1, a, b, m), s, ty)
            for m in nb:
                for m2 in sorted(graph[m] - {a, b}):
                    spawn((a, b, m, m2), s, ty)
    return (np.asarray(out[3][0], dtype=np.int64).reshape(-1, 3), np.asarray(out[3][1], dtype=np.int64),
            np.asarray(out[4][0], dtype=np.int64).reshape(-1, 4), np.asarray(out[4][1], dtype=np.int64))


# ---- the system of the GPU tests (also evaluated on the CPU by tests/test_hybrid_tuples_ref.py) -------------------------------------
# Six sites per axis in a box of edge 14 (rc 2.5 + skin 0.3: five cells per axis, the tile path), the first layer 0.15 behind the
# low faces, so molecules straddle the periodic boundary, cell and tile borders.  Every site carries one chain of beads 0.8 apart
# (pre-bonded, plain list) with one or two GAPS of 0.70 / 0.75 that a reaction closes; the type-1 bead sits on the site:
#   A  n a | b m          types 3 0 | 1 3        R0 (0 + 1) bonds a - b: triples (n a b), (a b m), quadruple (n a b m)
#   B  n c | b m          types 3 2 | 1 3        R1 (2 + 1), opened later: a second cohort in the same lists
#   C  n a | b | c k      types 3 0 | 1 | 2 3    R0, later R1 on the same b: the angle (a b c) is spawned around the older bond a - b
#   D  q p n a | b m      types 3 3 3 0 | 1 3    R0; (q p n), (p n a) are plain triples and (q p n a) a plain quadruple from the start:
#                                                the row of `a` holds a pair, a plain triple, two hybrid triples, a plain quadruple and
#                                                two hybrid quadruples, interleaved in list order
# in the order A B C D A: 216 sites, 993 particles.  Bending angles are drawn from 80..140 degrees, dihedrals from -170..170, so
# every angle is well inside 60..150 degrees and no three members are closer than sin(40 deg) = 0.64 to collinear.  A reactive bead
# of type 0 or 2 is at most 0.75 from its site, type 1 on it; sites are 14/6 = 2.33 apart and jittered by at most 0.05 per axis
# (0.09), so a foreign partner is at least 2.33 - 0.75 - 0.18 = 1.40 away: only the intended pairs lie inside the reaction cutoff
# 0.85 (asserted).  Beads of different molecules keep 0.45 between them (placement is retried with another orientation).
import math

from bonded_ref import _place, _rotation

SCENE_BOX, SCENE_RC, SCENE_SKIN, REACT_CUT = 14.0, 2.5, 0.3, 0.85
KINDS = {"A": ([3, 0, 1, 3], [1]), "B": ([3, 2, 1, 3], [1]), "C": ([3, 0, 1, 2, 3], [1, 2]), "D": ([3, 3, 3, 0, 1, 3], [3])}   # types, gaps (after position k)
REG3 = [(3, 0, 1), (0, 1, 3), (3, 2, 1), (2, 1, 3), (0, 1, 2), (1, 2, 3)]
REG4 = [(3, 0, 1, 3), (3, 2, 1, 3), (3, 0, 1, 2), (0, 1, 2, 3), (3, 3, 0, 1)]


def _chain(rng, k, gaps):
    length = [(0.70 if rng.integers(2) else 0.75) if j in gaps else 0.8 for j in range(k - 1)]
    th = np.radians(rng.uniform(80.0, 140.0, k))
    p = [np.zeros(3), np.array([length[0], 0.0, 0.0])]
    p.append(p[1] + length[1] * np.array([-math.cos(th[1]), math.sin(th[1]), 0.0]))
    for j in range(3, k):
        p.append(_place(p[j - 3], p[j - 2], p[j - 1], length[j - 1], th[j - 1], math.radians(rng.uniform(-170.0, 170.0))))
    return np.stack(p)


def scene(box=(SCENE_BOX,) * 3, order="ABCDA", seed=7, dt=1e-4):
    """Returns a dict: the particle arrays, `bonds0` / `angles0` / `dihedrals0` (the plain tuples that exist from the start, ids),
    `exclusions`, and the expected reacting pairs r0, r1 as ids (partner, type-1 bead)."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, dtype=np.float64)
    ns = np.rint(box / (SCENE_BOX / 6)).astype(int)
    sites = np.stack(np.meshgrid(*[np.arange(m) for m in ns], indexing="ij"), -1).reshape(-1, 3)
    centre = sites * (box / ns) + 0.15 + rng.uniform(-0.05, 0.05, sites.shape)
    pos, types, mol, bonds0, angles0, dihedrals0, excl, r0, r1 = np.zeros((0, 3)), [], [], [], [], [], [], [], []
    for s in range(len(sites)):
        kind = order[s % len(order)]
        ty, gaps = KINDS[kind]
        k = len(ty)
        for attempt in range(400):
            x = _chain(rng, k, gaps) @ _rotation(rng).T
            x = x - x[ty.index(1)] + centre[s]
            others = np.concatenate([pos, np.delete(centre, s, axis=0)])      # (no bead on a site that is not its own either)
            d = x[:, None, :] - others[None, :, :]
            d -= box * np.rint(d / box)
            if np.sqrt((d * d).sum(2)).min() > 0.45:
                break
        else:
            raise AssertionError("no room for molecule %d" % s)
        i0 = len(pos) + 1
        pos = np.concatenate([pos, x]); types += ty; mol += [s] * k
        for j in range(k - 1):
            if j in gaps:
                (r0 if 0 in (ty[j], ty[j + 1]) else r1).append((i0 + j, i0 + j + 1) if ty[j + 1] == 1 else (i0 + j + 1, i0 + j))
            else:
                bonds0.append((i0 + j, i0 + j + 1)); excl.append((i0 + j, i0 + j + 1))
        if kind == "D":
            angles0 += [(i0, i0 + 1, i0 + 2), (i0 + 1, i0 + 2, i0 + 3)]
            dihedrals0.append((i0, i0 + 1, i0 + 2, i0 + 3))
            excl += [(i0, i0 + 2), (i0 + 1, i0 + 3), (i0, i0 + 3)]
    n = len(pos)
    out = dict(n=n, box=box.tolist(), rc=SCENE_RC, skin=SCENE_SKIN, dt=dt, ids=np.arange(1, n + 1), types=np.asarray(types, np.int32), pos=pos,
               vel=np.zeros((n, 3)), mass=np.ones(n), state=np.zeros(n, np.int32), res_id=np.arange(1, n + 1, dtype=np.int32), mol=np.asarray(mol),
               kT=1.0, gamma=0.0, seed=1, rebuild_criterion=1)
    L = box
    x = out["pos"] - np.floor(out["pos"] / L) * L
    s32 = L / 2147483648.0          # positions both precisions of the engine represent exactly (workloads.snap_to_grid, restated)
    q = np.rint((x - 0.5 * L) / s32)
    q = np.where(q >= 2 ** 30, q - 2 ** 31, q)
    out["pos"] = q * s32 + 0.5 * L
    out.update(bonds0=np.asarray(bonds0, np.int64), angles0=np.asarray(angles0, np.int64).reshape(-1, 3), dihedrals0=np.asarray(dihedrals0, np.int64).reshape(-1, 4),
               exclusions=np.asarray(sorted(excl), np.int64), r0=sorted(r0), r1=sorted(r1))
    # isolation: within the reaction cutoff of a type-1 bead lie exactly its own partners
    ty = out["types"]
    ones = np.nonzero(ty == 1)[0]
    for t, want in ((0, out["r0"]), (2, out["r1"])):
        part = np.nonzero(ty == t)[0]
        d = out["pos"][part][:, None, :] - out["pos"][ones][None, :, :]
        d -= box * np.rint(d / box)
        r = np.sqrt((d * d).sum(2))
        assert np.abs(r - REACT_CUT).min() > 1e-3
        assert sorted((int(part[i]) + 1, int(ones[j]) + 1) for i, j in zip(*np.nonzero(r < REACT_CUT))) == want
    return out


def geometry_ok(pos, box, triples, quadruples):
    """every bending angle of the tuples (the two of a quadruple included) within 60..150 degrees: the members of a dihedral are
    then at least sin(30 deg) = 0.5 > 0.1 off collinear"""
    t3 = np.concatenate([np.asarray(triples, np.int64).reshape(-1, 3), np.asarray(quadruples, np.int64).reshape(-1, 4)[:, :3], np.asarray(quadruples, np.int64).reshape(-1, 4)[:, 1:]])
    if len(t3) == 0:
        return True
    box = np.asarray(box, dtype=np.float64)
    x = np.asarray(pos)
    r1, r2 = x[t3[:, 0] - 1] - x[t3[:, 1] - 1], x[t3[:, 2] - 1] - x[t3[:, 1] - 1]
    r1 -= box * np.rint(r1 / box); r2 -= box * np.rint(r2 / box)
    th = np.degrees(np.arctan2(np.linalg.norm(np.cross(r1, r2), axis=1), (r1 * r2).sum(1)))
    return bool(th.min() > 60.0 and th.max() < 150.0)
