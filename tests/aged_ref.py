"""Forces from a neighbour list that has aged: the reference, the rebuild rule and the constructions of
tests/test_aged_ref.py (CPU) and tests/test_gpu_aged_lists.py (device).  No engine and no oracle in here.

The invariant     at any step of an NVE run the forces an engine holds equal the exact sum over all non-excluded pairs inside
                  their cutoff at the engine's own positions -- however old the list is that the force kernel walked.
exact_pairs       that sum in fp64: pairs from a periodic k-d tree (no cells, no skin, no list), minimum image, every type pair
                  with helpers.pair_params / helpers.pair_eval at its own cutoff.
rule_rebuilds     the rebuild rule restated from the unfolded positions of every step (md_oracle.cpp run(), k_rebuild_decide):
                  criterion 1 rebuilds when max_i |x_s - x_build| > skin / 2, criterion 0 adds max_i |x_s - x_(s-1)| to an
                  accumulator, rebuilds when that exceeds skin / 2 and starts again from zero.
tight_closing_pairs   the isolated pairs of react_ref.closing_pairs, started just inside the list radius (rc + 0.99 skin) and
                  brought just inside the cutoff while every partner travels 0.498 skin -- 0.002 skin short of the rebuild.
                  A list radius 1 % too small loses them, and a rebuild decided 20 % late leaves out the one that falls due on the
                  step after.  Six more pairs lie off-centre across a slab boundary, one partner rc + 0.986 skin deep in the cell
                  layer the neighbour sends: a ghost layer 2 % of the skin thinner than the list radius would not hold it.
                  (A thermal melt does not reach that far: of the pairs inside rc at an oldest-list step of the melts below, none
                  was farther than rc + 0.55 skin when the list was built -- measured on the oracle's trajectories.)"""
import struct

import numpy as np

import helpers as H
from react_ref import _DIRS

SHELL = 2e-6            # the shell of helpers.force_error_without_cutoff_flips
UNDECIDABLE = 1e-5      # |compared value - skin / 2| below which fp32 and fp64 may decide a rebuild differently


def fold(pos, L):
    x = np.asarray(pos, dtype=np.float64)
    x = x - np.floor(x / L) * L
    return np.where(x >= L, 0.0, x)


def exact_pairs(spec, pos, types=None, exclusions=None):
    """dict(f = forces in spec order, epot_lj, epot_tab, virial_nb = sum of ff r^2, shell_pairs = pairs within SHELL of their
    cutoff, jump = the smallest |F(rc)| over the active type pairs: what one missed pair changes, fmax, npairs).
    types / exclusions (id pairs) default to the spec's."""
    from scipy.spatial import cKDTree
    L = np.asarray(spec["box"], dtype=np.float64)
    x = fold(pos, L)
    types = np.asarray(spec["types"] if types is None else types)
    ids = np.asarray(spec["ids"], dtype=np.int64)
    exclusions = spec.get("exclusions") if exclusions is None else exclusions
    prm = H.pair_params(spec)
    n = len(x)
    out = dict(f=np.zeros((n, 3)), epot_lj=0.0, epot_tab=0.0, virial_nb=0.0, shell_pairs=0, npairs=0)
    out["jump"] = min(abs(float(H.pair_eval(p, H.pair_cutoff(p) ** 2, cut=False)[0])) * H.pair_cutoff(p) for p in prm.values())
    ij = cKDTree(x, boxsize=L).query_pairs(max(H.pair_cutoff(p) for p in prm.values()) + SHELL, output_type="ndarray")
    if exclusions is not None and len(exclusions):
        ex = np.sort(np.asarray(exclusions, dtype=np.int64).reshape(-1, 2), 1)
        key = np.minimum(ids[ij[:, 0]], ids[ij[:, 1]]) * (ids.max() + 1) + np.maximum(ids[ij[:, 0]], ids[ij[:, 1]])
        ij = ij[~np.isin(key, ex[:, 0] * (ids.max() + 1) + ex[:, 1])]
    d = x[ij[:, 0]] - x[ij[:, 1]]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(1)
    ta, tb = types[ij[:, 0]], types[ij[:, 1]]
    for (a, b), p in prm.items():
        if a > b:
            continue
        m = np.nonzero(((ta == a) & (tb == b)) | ((ta == b) & (tb == a)))[0]
        ff, e = H.pair_eval(p, r2[m])
        fij = ff[:, None] * d[m]
        np.add.at(out["f"], ij[m, 0], fij)
        np.subtract.at(out["f"], ij[m, 1], fij)
        out["epot_lj" if p[0] == "lj" else "epot_tab"] += float(e.sum())
        out["virial_nb"] += float((ff * r2[m]).sum())
        out["shell_pairs"] += int((np.abs(np.sqrt(r2[m]) - H.pair_cutoff(p)) < SHELL).sum())
        out["npairs"] += int((r2[m] <= H.pair_cutoff(p) ** 2).sum())
    out["fmax"] = float(np.abs(out["f"]).max())
    return out


def rule_rebuilds(x_per_step, half_skin, criterion, follow=None):
    """x_per_step[s]: unfolded positions after step s (s = 0: where the list was first built).  Returns (steps s >= 1 whose
    positions call for a rebuild, steps at which the compared value lies within UNDECIDABLE of half_skin).  follow: the
    steps an engine rebuilt at; at an undecidable step the rule takes the engine's decision and goes on from there."""
    x = np.asarray(x_per_step, dtype=np.float64)
    built, acc = x[0], 0.0
    steps, unsure = [], []
    for s in range(1, len(x)):
        if criterion == 1:
            val = np.sqrt(((x[s] - built) ** 2).sum(1).max())
        else:
            acc += np.sqrt(((x[s] - x[s - 1]) ** 2).sum(1).max())
            val = acc
        need = val > half_skin
        if abs(val - half_skin) < UNDECIDABLE:
            unsure.append(s)
            if follow is not None:
                need = s in follow
        if need:
            steps.append(s)
            built, acc = x[s], 0.0
    return steps, unsure


def increments(counts):
    """Steps s >= 1 at which a counter recorded after every step (counts[0]: before the first) went up."""
    c = np.asarray(counts)
    return [int(s) for s in np.nonzero(np.diff(c) > 0)[0] + 1]


def header_list_skin(harness, spec, list_skin, dd=0, P=1):
    """pick_list_skin of chem_geom_host.hpp for the spec under option list_skin (tile path, fused rebuild), asked of the
    header itself through tests/host/geometry_harness.cpp; 0: the workload's skin stays."""
    line = "skin " + " ".join(H.dbits(v) for v in list(spec["box"]) + [spec["rc"], spec["skin"], list_skin])
    line += " %d 1 1 %d %d %d" % (spec.get("rebuild_criterion", 0), dd, P, len(spec["ids"]))
    out = H.run_harness(harness, [line])[0]
    return struct.unpack("<d", struct.pack("<Q", int(out[1])))[0]


def effective_skin(harness, spec, list_skin=0.0, dd=0, P=1):
    s = header_list_skin(harness, spec, list_skin, dd, P) if list_skin > 0 else 0.0
    return s if s > spec["skin"] else spec["skin"]


# ---- closing pairs at the edge of the list radius -----------------------------------------------------------------------------

TIGHT_RC, TIGHT_SKIN, TIGHT_DT, TIGHT_M, TIGHT_BOX = 1.5, 0.3, 0.001, 10, 32.0
START, TRAVEL = 0.99, 0.498               # in units of the effective skin: first separation beyond rc, path of each partner
RECEDE_START, RECEDE_TRAVEL = 0.25, 0.4   # receding pairs: rc - 0.25 apart, each partner leaves by 0.4 skin_eff
DEEP_NEAR = 0.004                         # off-centre pairs: how far inside its own slab the near partner starts


def slab_boundaries(nzg, P):
    """First cell layer of the ranks 1 .. P-1 (helpers.slab_capacities reads only box, rc, skin and the positions)."""
    spec = dict(box=[1.0, 1.0, float(nzg)], rc=0.75, skin=0.25, n=1, pos=np.zeros((1, 3)))
    return [c["z0"] for c in H.slab_capacities(spec, P)[1:]]


def _put_pair(acc, c, skin_eff):
    """The next pair of a construction, centred on c: direction, x shift, receding or closing and the types follow from its
    number (react_ref.closing_pairs)."""
    pos, vel, typ, closing = acc
    slot = len(closing)
    c = np.array(c, dtype=np.float64)
    c[0] += 0.1 * (slot % 4 - 1)
    u = np.array(_DIRS[slot % 13], dtype=np.float64)
    u /= np.sqrt(u @ u)
    recede = 13 <= slot < 26
    sep = TIGHT_RC - RECEDE_START if recede else TIGHT_RC + START * skin_eff
    v = (RECEDE_TRAVEL if recede else TRAVEL) * skin_eff / (TIGHT_M * TIGHT_DT)
    sgn = 1.0 if recede else -1.0
    pos.extend([c - 0.5 * sep * u, c + 0.5 * sep * u]); vel.extend([-sgn * v * u, sgn * v * u])
    typ.extend([slot % 2, 1 - slot % 2]); closing.append(not recede)


def _tight_spec(acc, box, skin_eff):
    """The spec of the pairs collected in acc; asserts that they are isolated: no particle of another pair comes within the list
    radius + 0.5 of a pair, at the start or at the end (free flight)."""
    rc, M, dt = TIGHT_RC, TIGHT_M, TIGHT_DT
    pos, vel = np.asarray(acc[0]), np.asarray(acc[1])
    n = len(pos)
    L = np.asarray(box, dtype=np.float64)
    spec = dict(name="tight_closing_pairs", n=n, box=[float(b) for b in box], rc=rc, skin=TIGHT_SKIN, dt=dt, ids=np.arange(1, n + 1),
                types=np.asarray(acc[2], dtype=np.int32), pos=fold(pos, L), vel=vel, mass=np.ones(n), state=np.zeros(n, np.int32),
                res_id=np.arange(1, n + 1, dtype=np.int32), lj=[(0, 0, 1.0, 1.0, rc), (0, 1, 1.0, 1.0, rc), (1, 1, 1.0, 1.0, rc)],
                kT=0.0, gamma=0.0, seed=1, rebuild_criterion=0, closing=np.asarray(acc[3]), M=M, skin_eff=skin_eff)
    for x in (pos, pos + M * dt * vel):
        xf = fold(x, L)
        for a in range(0, n, 2):
            for b in (a, a + 1):
                d = xf - xf[b]
                d -= L * np.rint(d / L)
                r = np.sqrt((d * d).sum(1))
                r[a] = r[a + 1] = np.inf
                assert r.min() > rc + skin_eff + 0.5, (a, r.min())
    return spec


def tight_closing_pairs(skin_eff, cell_edge):
    """64 + 6 isolated pairs, 140 particles, LJ eps = sigma = 1 cut at rc = 1.5 on all three type pairs, no reactions.  Centres on
    corners of the cell grid: along x and y the corners nearest to the points of an 8-grid (index 0: the periodic face), along z
    the periodic face, the boundary between two slabs, one between three slabs and a layer in the bulk -- whole cells from where
    react_ref.closing_pairs puts them, at least three cells apart.  The 13 directions, the x shifts (-0.1 .. 0.2) and the receding
    pairs (slots 13 .. 25) are those of closing_pairs.  A closing pair starts rc + 0.99 skin_eff apart; each partner travels
    0.498 skin_eff towards the other in M = 10 steps.  spec["closing"]: per pair; particles 2k and 2k + 1 are pair k;
    spec["deep"]: the six off-centre pairs (below)."""
    rc, M, dt, Lb = TIGHT_RC, TIGHT_M, TIGHT_DT, TIGHT_BOX
    nzg = int(np.floor(Lb / (rc + skin_eff)))
    assert abs(Lb / nzg - cell_edge) < 1e-12 * cell_edge, (nzg, cell_edge)
    b2, b3 = slab_boundaries(nzg, 2), slab_boundaries(nzg, 3)
    zlayers = [0, 4, b2[0], b3[1]]
    assert np.all(np.diff(zlayers + [nzg]) >= 3), zlayers
    pos, vel, typ, closing = acc = [], [], [], []
    for i in range(4):
        for j in range(4):
            for k in range(4):
                _put_pair(acc, np.array([np.rint(i * 8.0 / cell_edge), np.rint(j * 8.0 / cell_edge), zlayers[k]]) * cell_edge, skin_eff)
    # the pairs above sit astride their corner: no partner is deeper than half a separation in a neighbour's boundary layer.
    # Six more closing pairs along z lie off-centre across a slab boundary (the periodic face, the one of two slabs, one of three
    # slabs; once from either side): one partner DEEP_NEAR skin_eff inside its slab, the other rc + (START - DEEP_NEAR) skin_eff
    # deep in the neighbour's layer -- inside the cell layer a slab imports, outside one that is 2 % of the skin thinner.
    deep = []
    for zl in (0, b2[0], b3[1]):
        for side in (1.0, -1.0):
            sep, v = rc + START * skin_eff, TRAVEL * skin_eff / (M * dt)
            c = np.array([(2 if side > 0 else 6) * cell_edge, 2 * cell_edge, zl * cell_edge + side * DEEP_NEAR * skin_eff])
            u = np.array([0.0, 0.0, side])
            assert sep - DEEP_NEAR * skin_eff < cell_edge
            pos.extend([c, c - sep * u]); vel.extend([-v * u, v * u])
            typ.extend([len(closing) % 2, 1 - len(closing) % 2]); deep.append(len(closing)); closing.append(True)
    spec = _tight_spec(acc, [Lb] * 3, skin_eff)
    pos = np.asarray(pos)
    # a closing pair across the boundary of two slabs, of three slabs, and across the periodic z face
    z0, z1 = pos[0::2, 2], pos[1::2, 2]
    lay = lambda z: np.floor(np.mod(z, Lb) * nzg / Lb).astype(int)      # noqa: E731
    owner = lambda z, P: np.searchsorted(np.array(slab_boundaries(nzg, P)), lay(z), side="right")      # noqa: E731
    cl = spec["closing"]
    spec["straddle"] = dict(P2=int((cl & (owner(z0, 2) != owner(z1, 2)) & (np.minimum(z0, z1) > 1.0)).sum()),
                            P3=int((cl & (owner(z0, 3) != owner(z1, 3)) & (np.minimum(z0, z1) > 1.0)).sum()),
                            face=int((cl & (np.minimum(z0, z1) < 0.0) & (np.maximum(z0, z1) > 0.0)).sum()))
    assert min(spec["straddle"].values()) >= 1, spec["straddle"]
    # the off-centre pairs: the far partner deeper than rc + 0.98 skin_eff beyond the boundary its partner sits on, inside the cell layer
    spec["deep"] = np.asarray(deep)
    for q, k in enumerate(deep):
        zb = (0, b2[0], b3[1])[q // 2] * cell_edge
        depth = [abs(z0[k] - zb), abs(z1[k] - zb)]
        assert depth[0] < 0.005 * skin_eff and rc + 0.98 * skin_eff < depth[1] < cell_edge and (z0[k] - zb) * (z1[k] - zb) < 0, (k, depth)
    return spec


def tight_closing_pairs_flat(skin_eff):
    """The same pairs in a box of 32 x 32 x 5: under three cells along z, so no cells at all and the brute-force list.  36 pairs
    (72 particles) on a 6 x 6 grid in x and y, centred on the periodic z face and on the middle of the box in turn."""
    Lz = 5.0
    assert 2.0 * (TIGHT_RC + skin_eff) < Lz < 3.0 * (TIGHT_RC + skin_eff)
    acc = [], [], [], []
    for i in range(6):
        for j in range(6):
            _put_pair(acc, [i * TIGHT_BOX / 6, j * TIGHT_BOX / 6, 0.5 * Lz * ((i + j) % 2)], skin_eff)
    spec = _tight_spec(acc, [TIGHT_BOX, TIGHT_BOX, Lz], skin_eff)
    z0, z1 = np.asarray(acc[0])[0::2, 2], np.asarray(acc[0])[1::2, 2]
    spec["straddle"] = dict(face=int((spec["closing"] & (np.minimum(z0, z1) < 0.0) & (np.maximum(z0, z1) > 0.0)).sum()))
    assert spec["straddle"]["face"] >= 1
    return spec


def pair_separations(spec, pos):
    """Minimum-image distance of every pair (particles 2k, 2k + 1) at `pos`."""
    L = np.asarray(spec["box"], dtype=np.float64)
    x = np.asarray(pos, dtype=np.float64)
    d = x[0::2] - x[1::2]
    d -= L * np.rint(d / L)
    return np.sqrt((d * d).sum(1))


TIGHT_VARIANTS = {       # name: (rebuild criterion, option list_skin, cells per axis)
    "crit0": (0, 0.0, 17), "crit1": (1, 0.0, 17), "list_skin": (0, 0.5, 16),
}


def tight_variant(name, harness, dd=0, P=1, flat=False):
    """(spec, engine options) of a variant; the effective skin comes from the header.  flat: the box of the brute-force list."""
    crit, ls, ncell = TIGHT_VARIANTS[name]
    if flat:
        assert ls == 0.0
        return dict(tight_closing_pairs_flat(TIGHT_SKIN), rebuild_criterion=crit), {}
    probe = dict(box=[TIGHT_BOX] * 3, rc=TIGHT_RC, skin=TIGHT_SKIN, ids=np.arange(140), rebuild_criterion=crit)
    se = effective_skin(harness, probe, ls, dd, P)
    assert (se == TIGHT_SKIN) == (ls == 0.0), (name, se)
    spec = tight_closing_pairs(se, TIGHT_BOX / ncell)
    spec["rebuild_criterion"] = crit
    return spec, ({"list_skin": ls} if ls > 0 else {})


# ---- the melts ------------------------------------------------------------------------------------------------------------------

MELT_STEPS, MELT_KT, MELT_DT = 80, 1.5, 0.004
MAX_SHELL = 8


def melt(n):
    from chemlab_amd import workloads as W
    return W.lj_melt(n=n, seed=31, jitter=0.05, kT=MELT_KT, dt=MELT_DT)


def _unit_masses(spec, seed):
    """The configuration with unit masses, Maxwell velocities at MELT_KT (zero total momentum) and dt = MELT_DT."""
    from chemlab_amd import workloads as W
    n = len(spec["ids"])
    m = np.ones(n)
    out = dict(spec, mass=m, vel=W._maxwell(np.random.default_rng(seed), n, MELT_KT, m), dt=MELT_DT, kT=MELT_KT, gamma=0.0)
    out.setdefault("state", np.zeros(n, np.int32))
    out.setdefault("res_id", np.arange(1, n + 1, dtype=np.int32))
    return out


def small_box_melt():
    """The 343-particle box of mass_ref.small_box_config (under three cells per axis: the brute-force list; ids that are not
    the tags; two exclusions)."""
    import mass_ref
    return _unit_masses(mass_ref.small_box_config(), 81)


def slab_melt():
    """The elongated box of mass_ref.slab_config (5 x 5 x 12 cells, about 3100 particles; fits two and three slabs)."""
    import mass_ref
    return _unit_masses(mass_ref.slab_config(), 82)


MELTS = {"melt8788": lambda: melt(8788), "melt2197": lambda: melt(2197), "small_box": small_box_melt, "slab": slab_melt}
_MELT_CACHE = {}


def melt_spec(name, criterion):
    if name not in _MELT_CACHE:
        _MELT_CACHE[name] = MELTS[name]()
    return dict(_MELT_CACHE[name], rebuild_criterion=criterion)


def check_steps(list_counts):
    """The steps of a recorded run at which the forces are compared: every step whose successor built a list (the list at its
    oldest), every step that built one, step 1 and the last.  Also returns the oldest-list steps alone."""
    inc = increments(list_counts)
    last = len(list_counts) - 1
    oldest = sorted({s - 1 for s in inc if s - 1 >= 1})
    return sorted(set(oldest) | set(inc) | {1, last}), oldest


def guards(ref):
    """The conditions under which a missed pair cannot hide: few pairs on the cutoff, and the fp32 force tolerance (2e-5 of
    the largest force) a quarter of what one pair at its cutoff carries, at the most."""
    return ref["shell_pairs"] <= MAX_SHELL and 2e-5 * ref["fmax"] < ref["jump"] / 4
