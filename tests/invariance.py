"""Two symmetries of a `workloads` spec, in plain numpy: the names of the particles and the orientation of the box.  Nothing of the
engine or the oracle is imported here; a helper maps a spec to another spec of the same physical system and returns what maps
the results back (tests/test_invariance_ref.py on the CPU, tests/test_gpu_invariance.py on the device).

relabel        particle ids[k] becomes new_ids[k] wherever an id occurs, and the particle rows are handed over in row_order.
               An engine works on tags (the rank of a particle by id) and meets ids only at its boundary: a relabelling that
               keeps the ORDER of the ids keeps every tag, so the engine must compute the same bits; one that changes the order
               changes the tags (random streams, summation order, tie-breaks), so only deterministic results to rounding.
permute_axes   new axis a is old axis perm[a]: box, positions, velocities, region slabs.
reflect        x -> L - x along one axis (folded back into [0, L)), v -> -v.

Keys of a spec that carry ids: "ids", "lists"[*]["ids"], "exclusions", and the keys the scenes of the invariance tests add:
"restrict" [(reaction, id pairs)], "fix" [dict(pairs=id pairs, ...)], "modify" [(id, what, value)], "lam_set" (ids, lambda),
"add" dict(ids=..., per-row arrays) -- the particles of add_particles, whose ids belong to the domain of the map (behind the
spec's own).  Per-row keys: types pos vel mass state res_id q lam.  res_id is a label, not an id: it stays."""
import numpy as np

ROW_KEYS = ("types", "pos", "vel", "mass", "state", "res_id", "q", "lam")
VECTOR_KEYS = ("pos", "vel")
TENSOR = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # xx yy zz xy xz yz


class IdMap:
    """old id -> new id, both ways, on arrays of any shape"""

    def __init__(self, old, new):
        old, new = np.asarray(old, dtype=np.int64), np.asarray(new, dtype=np.int64)
        assert old.shape == new.shape and len(np.unique(old)) == len(old) and len(np.unique(new)) == len(new)
        self.old, self.new = old, new
        self._so, self._sn = np.argsort(old), np.argsort(new)

    @staticmethod
    def _map(a, src, order, dst):
        a = np.asarray(a, dtype=np.int64)
        if a.size == 0:
            return a.copy()
        k = np.searchsorted(src[order], a)
        assert np.all(k < len(src)) and np.all(src[order][k] == a), "an id outside the map"
        return dst[order][k]

    def fwd(self, a):
        return self._map(a, self.old, self._so, self.new)

    def inv(self, a):
        return self._map(a, self.new, self._sn, self.old)

    def inverse(self):
        return IdMap(self.new, self.old)

    def keeps_order(self):
        return bool(np.all(np.diff(self.new[self._so]) > 0))


def all_ids(spec):
    ids = np.asarray(spec["ids"], dtype=np.int64)
    return np.concatenate([ids, np.asarray(spec["add"]["ids"], dtype=np.int64)]) if spec.get("add") else ids


def relabel(spec, new_ids, row_order=None):
    """(spec under the new names with the rows in row_order, IdMap).  new_ids[k] names all_ids(spec)[k]; row_order permutes the
    rows of the spec itself (the particles of "add" keep their order)."""
    m = IdMap(all_ids(spec), new_ids)
    n = len(spec["ids"])
    order = np.arange(n) if row_order is None else np.asarray(row_order)
    assert sorted(order.tolist()) == list(range(n))
    out = dict(spec)
    out["ids"] = m.fwd(spec["ids"])[order]
    for k in ROW_KEYS:
        if spec.get(k) is not None:
            out[k] = np.asarray(spec[k])[order]
    if spec.get("lists") is not None:
        out["lists"] = [dict(l, ids=m.fwd(l["ids"])) for l in spec["lists"]]
    if spec.get("exclusions") is not None:
        out["exclusions"] = m.fwd(spec["exclusions"])
    if spec.get("restrict") is not None:
        out["restrict"] = [(r, m.fwd(p)) for r, p in spec["restrict"]]
    if spec.get("fix") is not None:
        out["fix"] = [dict(f, pairs=m.fwd(f["pairs"])) for f in spec["fix"]]
    if spec.get("modify") is not None:
        out["modify"] = [(int(m.fwd(np.array([i]))[0]), w, v) for i, w, v in spec["modify"]]
    if spec.get("lam_set") is not None:
        out["lam_set"] = (m.fwd(spec["lam_set"][0]), spec["lam_set"][1])
    if spec.get("add"):
        out["add"] = dict(spec["add"], ids=m.fwd(spec["add"]["ids"]))
    return out, m


class AxisMap:
    """new = S o P (old): new component a is sign[a] times old component perm[a].  back_*: from the new frame to the old one."""

    def __init__(self, perm, sign=(1.0, 1.0, 1.0)):
        self.perm, self.sign = tuple(int(p) for p in perm), np.asarray(sign, dtype=np.float64)
        assert sorted(self.perm) == [0, 1, 2]

    def vec(self, v):
        v = np.asarray(v)
        return v[..., list(self.perm)] * self.sign.astype(v.dtype) if v.dtype.kind == "f" else v[..., list(self.perm)]

    def back_vec(self, v):
        v = np.asarray(v)
        out = np.empty_like(v)
        for a, p in enumerate(self.perm):
            out[..., p] = v[..., a] * (self.sign[a] if v.dtype.kind == "f" else 1)
        return out

    def tensor6(self, t):
        """six components (xx yy zz xy xz yz) of the old frame as the new frame sees them"""
        t = np.asarray(t, dtype=np.float64)
        old = {}
        for c, (a, b) in enumerate(TENSOR):
            old[(a, b)] = old[(b, a)] = t[..., c]
        return np.stack([self.sign[a] * self.sign[b] * old[(self.perm[a], self.perm[b])] for a, b in TENSOR], -1)

    def back_tensor6(self, t):
        t = np.asarray(t, dtype=np.float64)
        out = np.empty_like(t)
        for c, (a, b) in enumerate(TENSOR):
            pa, pb = self.perm[a], self.perm[b]
            out[..., TENSOR.index((min(pa, pb), max(pa, pb)))] = self.sign[a] * self.sign[b] * t[..., c]
        return out


def _fold(x, L):
    x = x - np.floor(x / L) * L
    return np.where(x >= L, 0.0, x)


def _transform(spec, am, reflect_axis=None):
    L0 = np.asarray(spec["box"], dtype=np.float64)
    L = L0[list(am.perm)]

    def pos(x):
        x = np.asarray(x, dtype=np.float64)[:, list(am.perm)]
        if reflect_axis is not None:
            x = x.copy()
            x[:, reflect_axis] = _fold(L[reflect_axis] - _fold(x[:, reflect_axis], L[reflect_axis]), L[reflect_axis])
        return x

    def rows(d):
        d = dict(d)
        if d.get("pos") is not None:
            d["pos"] = pos(d["pos"])
        if d.get("vel") is not None:
            d["vel"] = am.vec(np.asarray(d["vel"], dtype=np.float64))
        return d
    out = rows(spec)
    out["box"] = [float(v) for v in L]
    if spec.get("add"):
        out["add"] = rows(spec["add"])
    if spec.get("regions") is not None:
        regs = []
        for r in spec["regions"]:
            lo, hi = np.asarray(r["lo"], dtype=np.float64)[list(am.perm)], np.asarray(r["hi"], dtype=np.float64)[list(am.perm)]
            if reflect_axis is not None:
                a = reflect_axis
                lo[a], hi[a] = L[a] - hi[a], L[a] - lo[a]      # [lo, hi) becomes (L - hi, L - lo]: no particle of a test sits on a face of a slab
            regs.append(dict(r, lo=lo.tolist(), hi=hi.tolist()))
        out["regions"] = regs
    return out


def permute_axes(spec, perm):
    """(spec whose axis a is the old axis perm[a], AxisMap)"""
    am = AxisMap(perm)
    return _transform(spec, am), am


def reflect(spec, axis):
    """(spec mirrored along `axis`: x -> L - x folded into [0, L), v -> -v; AxisMap)"""
    sign = [1.0, 1.0, 1.0]
    sign[axis] = -1.0
    am = AxisMap((0, 1, 2), sign)
    return _transform(spec, am, reflect_axis=axis), am


CYCLIC = ((1, 2, 0), (2, 0, 1))
ORIENTATIONS = [("id", None)] + [("perm%d%d%d" % p, p) for p in CYCLIC] + [("mirror_%s" % "xyz"[a], a) for a in range(3)]


def orient(spec, how):
    """the spec in one of ORIENTATIONS (by name) and its AxisMap"""
    arg = dict(ORIENTATIONS)[how]
    if arg is None:
        return dict(spec), AxisMap((0, 1, 2))
    return permute_axes(spec, arg) if isinstance(arg, tuple) else reflect(spec, arg)


def gapped_ids(n, seed, base=7):
    """ascending ids with gaps of 0 .. 7 between neighbours: 7 + cumsum(integers(1, 9))"""
    return base + np.cumsum(np.random.default_rng(seed).integers(1, 9, n)).astype(np.int64)
