"""Engine -- thin object wrapper over one C-ABI context (include/chem_mi355.h).

One Engine == one `chem_ctx` == one GPU.  All arrays cross the boundary as plain
pointers + sizes (numpy buffers); nothing here computes physics.
"""
import ctypes as C
import os

import numpy as np

from . import _capi


class ChemError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("chem error %d: %s" % (code, msg))
        self.code = code


def _ptr(a, typ):
    return a.ctypes.data_as(C.POINTER(typ)) if a is not None else None


def comm_unique_id():
    """RCCL unique id (128 bytes) for chem_comm_init; call on rank 0 and broadcast."""
    api = _capi.load()
    buf = C.create_string_buffer(128)
    rc = api.comm_unique_id(buf)
    if rc < 0:
        raise ChemError(rc, (api.last_error(None) or b"").decode())
    return buf.raw


def rdf_edges(r_max, nbins):
    """The bin edges of the rule set: e[k] = k * (r_max / nbins) in fp64."""
    return np.arange(nbins + 1, dtype=np.float64) * (np.float64(r_max) / np.float64(nbins))


def rdf_result(r_max, counts, frames, pairs, density):
    """The dict Engine.rdf() returns, from the raw integers and normalisers of chem_rdf_get (the division is done here)."""
    counts = np.asarray(counts, dtype=np.uint64)
    nsel, parts, nbins = counts.shape
    edges = rdf_edges(r_max, nbins)
    shell = (4.0 * np.pi / 3.0) * (edges[1:] ** 3 - edges[:-1] ** 3)
    g = np.zeros(counts.shape, dtype=np.float64)
    for s in range(nsel):
        if density[s] > 0:
            g[s] = counts[s].astype(np.float64) / (density[s] * shell)
    return dict(r=0.5 * (edges[1:] + edges[:-1]), edges=edges, counts=counts, g=g, frames=int(frames), pairs=np.asarray(pairs),
                density=np.asarray(density), r_max=float(r_max), nbins=nbins, split=parts == 2)


def sq_nvec(nmax):
    """The number of kept wave vectors: the canonical half of |n_a| <= nmax without n = 0."""
    return ((2 * int(nmax) + 1) ** 3 - 1) // 2


def sq_vectors(nmax):
    """The integer triples n of the rule set in index order, (nvec, 3) int64: |n_a| <= nmax, the half with nx > 0, or nx = 0 and
    ny > 0, or nx = ny = 0 and nz > 0, lexicographic in (nx, ny, nz) -- sq_vec of chem_sq_host.hpp."""
    nmax = int(nmax)
    r = np.arange(-nmax, nmax + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)      # lexicographic in (nx, ny, nz)
    keep = (n[:, 0] > 0) | ((n[:, 0] == 0) & (n[:, 1] > 0)) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] > 0))
    return n[keep].astype(np.int64)


def sq_result(nmax, sums, frames, na, nb, box_sum):
    """The dict Engine.sq() returns, from the raw sums and books of chem_sq_get (the division is done here): n (nvec, 3), sums
    [npairs][nvec], S = sums / sqrt(na nb) (zeros before the first frame or for an empty set), q = |q(n)| at the mean box,
    the shell average over bins of width 2 pi / max(mean box) -- shell_q (mean |q| of the shell's vectors), shell_count,
    shell_S [npairs][shells], empty shells left out --, frames, na, nb, box_sum, box (the mean box), nmax, nvec."""
    sums = np.asarray(sums, dtype=np.float64)
    nsel, nvec = sums.shape
    n = sq_vectors(nmax)
    assert n.shape[0] == nvec == sq_nvec(nmax)
    na, nb, box_sum = np.asarray(na, dtype=np.float64), np.asarray(nb, dtype=np.float64), np.asarray(box_sum, dtype=np.float64)
    S = np.zeros(sums.shape, dtype=np.float64)
    for s in range(nsel):
        if na[s] > 0 and nb[s] > 0:
            S[s] = sums[s] / np.sqrt(na[s] * nb[s])
    frames = int(frames)
    box = box_sum / frames if frames > 0 else np.zeros(3)
    if frames > 0:
        q = 2.0 * np.pi * np.sqrt(((n / box) ** 2).sum(axis=1))
        dq = 2.0 * np.pi / box.max()
        sh = np.floor(q / dq + 0.5).astype(np.int64)
        ids = np.unique(sh)
        shell_count = np.array([(sh == i).sum() for i in ids], dtype=np.int64)
        shell_q = np.array([q[sh == i].mean() for i in ids])
        shell_S = np.array([[S[s][sh == i].mean() for i in ids] for s in range(nsel)]).reshape(nsel, len(ids))
    else:
        q, shell_count, shell_q, shell_S = np.zeros(nvec), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros((nsel, 0))
    return dict(n=n, sums=sums, S=S, q=q, shell_q=shell_q, shell_count=shell_count, shell_S=shell_S, frames=frames, na=na, nb=nb,
                box_sum=box_sum, box=box, nmax=int(nmax), nvec=nvec)


class Engine:
    def __init__(self, device=0, precision=32, api=None, ctx=None):
        """precision: 32 (fp32 arrays, fp64 bonded/reaction distance) or 64 (all fp64)."""
        if api is None:
            api = _capi.load()
            ctx = api.create(int(device), int(precision))
            if not ctx:
                raise ChemError(_capi.EDEVICE, (api.last_error(None) or b"chem_create failed").decode())
        self.api, self.ctx = api, ctx
        self.precision = precision
        self._lists = {}  # handle -> arity

    def close(self):
        if self.ctx:
            self.api.destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise ChemError(rc, (self.api.last_error(self.ctx) or b"").decode())
        return rc

    # ---- set-up ----
    def set_box(self, L):
        L = np.ascontiguousarray(L, dtype=np.float64)
        self._ck(self.api.set_box(self.ctx, _ptr(L, C.c_double)))

    def set_cutoff(self, max_cutoff, skin):
        self._ck(self.api.set_cutoff(self.ctx, float(max_cutoff), float(skin)))

    def set_dt(self, dt):
        self._ck(self.api.set_dt(self.ctx, float(dt)))

    def set_particles(self, ids, types, pos, mass, vel=None, q=None, state=None, res_id=None):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = ids.shape[0]
        types = np.ascontiguousarray(types, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(n, 3)
        mass = np.ascontiguousarray(np.broadcast_to(np.asarray(mass, dtype=np.float64), (n,)))
        vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float64).reshape(n, 3)
        q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        state = None if state is None else np.ascontiguousarray(state, dtype=np.int32)
        res_id = None if res_id is None else np.ascontiguousarray(res_id, dtype=np.int32)
        self._ck(self.api.set_particles(
            self.ctx, n, _ptr(ids, C.c_int64), _ptr(types, C.c_int32), _ptr(pos, C.c_double),
            _ptr(vel, C.c_double), _ptr(mass, C.c_double), _ptr(q, C.c_double),
            _ptr(state, C.c_int32), _ptr(res_id, C.c_int32)))

    def modify_particle(self, pid, what, value):
        if what.upper() == "LAMBDA":
            self._res_entry("set_resolution")
        self._ck(self.api.modify_particle(self.ctx, int(pid), _capi.STATE[what.upper()], float(value)))

    def set_exclusions(self, pairs):
        p = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        self._ck(self.api.set_exclusions(self.ctx, p.shape[0], _ptr(p, C.c_int64)))

    def nb_lj(self, t1, t2, eps, sig, rc, shift_auto=True):
        self._ck(self.api.nb_lj(self.ctx, t1, t2, eps, sig, rc, 1 if shift_auto else 0))

    def _interp_entry(self, name, itype):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("Tabulated itype %r: the CPU checker has linear tables (itype=1) only" % (itype,))
        return fn

    def nb_table(self, t1, t2, r0, dr, e, f, rc, itype=1):
        """itype: 1 linear, 2 Akima, 3 natural cubic spline (include/chem_mi355.h, chem_nb_table_interp)."""
        e = np.ascontiguousarray(e, dtype=np.float64)
        f = np.ascontiguousarray(f, dtype=np.float64)
        assert e.shape == f.shape
        if itype == 1:
            self._ck(self.api.nb_table(self.ctx, t1, t2, e.shape[0], r0, dr, _ptr(e, C.c_double),
                                       _ptr(f, C.c_double), rc))
        else:
            self._ck(self._interp_entry("nb_table_interp", itype)(self.ctx, t1, t2, e.shape[0], r0, dr, _ptr(e, C.c_double),
                                                                  _ptr(f, C.c_double), rc, int(itype)))

    def nb_coulomb(self, t1, t2, prefactor, rc):
        """Truncated Coulomb term U = prefactor q_i q_j / r for r <= rc on the type pair, on top of its LJ / table
        (include/chem_mi355.h, chem_nb_coulomb); prefactor = 0 removes it.  One (prefactor, rc) for all pairs."""
        fn = getattr(self.api, "nb_coulomb", None)
        if fn is None:
            raise NotImplementedError("CoulombTruncated: the CPU checker has no Coulomb term")
        self._ck(fn(self.ctx, int(t1), int(t2), float(prefactor), float(rc)))

    def get_coulomb(self):
        """(energy, sum over pairs of r.F) of the Coulomb term at the current positions."""
        fn = getattr(self.api, "get_coulomb", None)
        if fn is None:
            raise NotImplementedError("CoulombTruncated: the CPU checker has no Coulomb term")
        e, v = C.c_double(0.0), C.c_double(0.0)
        self._ck(fn(self.ctx, C.byref(e), C.byref(v)))
        return e.value, v.value

    # ---- per-particle resolution lambda (include/chem_mi355.h, chem_nb_resolution ff.) ----
    def _res_entry(self, name):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("resolution: the CPU checker has no per-particle lambda")
        return fn

    def nb_resolution(self, t1, t2, on=True, max_force=0.0):
        """Mark (or unmark) the LJ / table of the type pair as scaled by lambda_i lambda_j, capped at max_force (> 0)."""
        self._ck(self._res_entry("nb_resolution")(self.ctx, int(t1), int(t2), 1 if on else 0, float(max_force)))

    def resolution_rate(self, type_id, alpha, new_type=-1, new_mass=0.0, new_q=0.0, new_state=-1):
        """BasicDynamicResolution {type: alpha}; with new_type >= 0 the property change when lambda reaches 1.  alpha <= 0
        removes the entry."""
        self._ck(self._res_entry("resolution_rate")(self.ctx, int(type_id), float(alpha), int(new_type), float(new_mass), float(new_q), int(new_state)))

    def set_resolution(self, ids, lam):
        """lambda of the particles `ids` (lambda_adr), stamped at the current step; a scalar is broadcast."""
        fn = self._res_entry("set_resolution")
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), ids.shape))
        self._ck(fn(self.ctx, ids.shape[0], _ptr(ids, C.c_int64), _ptr(lam, C.c_double)))

    def reaction_set_resolution(self, reaction, role, lam):
        """On every event of `reaction` the particle of `role` ('type_1' | 'type_2' | 1 | 2) gets lambda `lam`; negative removes."""
        ro = {"type_1": 1, "type_2": 2}.get(role, role)
        self._ck(self._res_entry("reaction_set_resolution")(self.ctx, int(reaction), int(ro), float(lam)))

    def nb_cap(self, t1, t2, caprad):
        """Cap the LJ / table of the type pair at the radius caprad: inside it the pair is evaluated at r = caprad
        (include/chem_mi355.h, chem_nb_cap); caprad <= 0 removes the cap."""
        fn = getattr(self.api, "nb_cap", None)
        if fn is None:
            raise NotImplementedError("capped pair potentials: the CPU checker has no cap radius")
        self._ck(fn(self.ctx, int(t1), int(t2), float(caprad)))

    # ---- fixed distances / by-product release (include/chem_mi355.h, chem_fix_create ff.) ----
    def _fix_entry(self, name):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("FixDistances: the CPU checker has no fixed distances")
        return fn

    def add_particles(self, ids, types, pos, mass, vel=None, q=None, state=None, res_id=None):
        """Append particles (ids above the largest present one) at step 0, before the first run; lists, exclusions,
        stamps and reactions are kept."""
        fn = self._fix_entry("add_particles")
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        n = ids.shape[0]
        types = np.ascontiguousarray(types, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(n, 3)
        mass = np.ascontiguousarray(np.broadcast_to(np.asarray(mass, dtype=np.float64), (n,)))
        vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float64).reshape(n, 3)
        q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        state = None if state is None else np.ascontiguousarray(state, dtype=np.int32)
        res_id = None if res_id is None else np.ascontiguousarray(res_id, dtype=np.int32)
        self._ck(fn(self.ctx, n, _ptr(ids, C.c_int64), _ptr(types, C.c_int32), _ptr(pos, C.c_double), _ptr(vel, C.c_double),
                    _ptr(mass, C.c_double), _ptr(q, C.c_double), _ptr(state, C.c_int32), _ptr(res_id, C.c_int32)))

    def fix_create(self, anchor_type=-1, target_type=-1):
        """A new set of fixed distances; with types, an entry leaves when its anchor or target no longer has that type."""
        return self._ck(self._fix_entry("fix_create")(self.ctx, int(anchor_type), int(target_type)))

    def fix_add(self, h, pairs, dist):
        """Entries (anchor id, target id) at distance `dist`."""
        p = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        self._ck(self._fix_entry("fix_add")(self.ctx, int(h), p.shape[0], _ptr(p, C.c_int64), float(dist)))

    def fix_postprocess(self, h, old_type, new_type=-1, new_mass=0.0, new_q=0.0, new_state=-1, lam=-1.0):
        """What becomes of a released target of type old_type; lam in [0, 1] stamps its resolution, negative leaves it."""
        self._ck(self._fix_entry("fix_postprocess")(self.ctx, int(h), int(old_type), int(new_type), float(new_mass), float(new_q), int(new_state), float(lam)))

    def reaction_release(self, reaction, role, h, count=1):
        """PostProcessReleaseParticles(fd, count) on role 'type_1' | 'type_2' | 'both' of `reaction`."""
        for ro in {"type_1": (1,), "type_2": (2,), "both": (1, 2), 1: (1,), 2: (2,)}[role]:
            self._ck(self._fix_entry("reaction_release")(self.ctx, int(reaction), ro, int(h), int(count)))

    def fix_count(self, h):
        return self._ck(self._fix_entry("fix_count")(self.ctx, int(h)))

    def fix_get(self, h):
        """(pairs (n, 2) int64, dist (n,)) of the live entries in insertion order."""
        fn = self._fix_entry("fix_get")
        n = self._ck(fn(self.ctx, int(h), None, None, 0))
        ids, d = np.empty((n, 2), dtype=np.int64), np.empty(n, dtype=np.float64)
        if n:
            self._ck(fn(self.ctx, int(h), _ptr(ids, C.c_int64), _ptr(d, C.c_double), n))
        return ids, d

    def fix_log(self):
        """Release records (step, set, anchor_id, target_id, cause) ordered by (step, set, insertion index)."""
        fn = self._fix_entry("fix_log")
        n = self._ck(fn(self.ctx, None, 0))
        buf = (_capi.FixRecord * max(n, 1))()
        if n:
            self._ck(fn(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("anchor_id", "i8"), ("target_id", "i8"), ("set", "i4"), ("cause", "i4")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def supports(self, name):
        """Whether this engine's library exports the entry point `name` (without the prefix), e.g. 'reaction_join': the CPU
        checker lacks what only the product has."""
        if name == "checkpoint":
            name = "checkpoint_save"
        if name == "region":
            name = "region_add"
        if name == "rdf":
            name = "rdf_init"
        if name == "sq":
            name = "sq_init"
        return getattr(self.api, name, None) is not None

    # ---- region rules: FreezeRegion, ChangeParticleType (include/chem_mi355.h, chem_region_add ff.) ----
    REGION_MODES = dict(all=0, prob=1, num=2, fraction=3)

    def _region_entry(self, name, what="region rules"):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("%s: the CPU checker has no region rules" % what)
        return fn

    def region_add(self, lo, hi, target_type, new_type, interval=1, mode="all", value=0.0, num=0, new_mass=-1.0, new_q=0.0,
                   reset_velocity=False, reset_force=False, seed=0, what="region rules"):
        """A region rule over the box [lo, hi) (folded coordinates): every `interval` steps the selected particles of
        target_type inside become new_type.  mode 'all' | 'prob' (value) | 'num' (num) | 'fraction' (value); new_mass < 0 keeps
        mass and charge.  Returns the rule index; the rule is off until region_enable."""
        fn = self._region_entry("region_add", what)
        d = _capi.RegionDesc()
        for k in range(3):
            d.lo[k], d.hi[k] = float(lo[k]), float(hi[k])
        d.target_type, d.new_type, d.new_mass, d.new_q = int(target_type), int(new_type), float(new_mass), float(new_q)
        d.interval, d.mode, d.value, d.num = int(interval), int(self.REGION_MODES.get(mode, mode)), float(value), int(num)
        d.reset_velocity, d.reset_force, d.seed = int(bool(reset_velocity)), int(bool(reset_force)), int(seed) & (2 ** 64 - 1)
        return self._ck(fn(self.ctx, C.byref(d)))

    def region_enable(self, rule, on=True):
        self._ck(self._region_entry("region_enable")(self.ctx, int(rule), 1 if on else 0))

    def region_changes(self):
        """Every change (step, id, rule), ordered by step, then rule, then id."""
        fn = self._region_entry("region_get_changes")
        n = self._ck(fn(self.ctx, None, 0))
        buf = (_capi.RegionChange * max(n, 1))()
        if n:
            self._ck(fn(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("id", "i8"), ("rule", "i4"), ("pad", "i4")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def region_stats(self):
        """One row (step, rule, candidates, changed) per firing of a rule that changed something."""
        fn = self._region_entry("region_get_stats")
        n = self._ck(fn(self.ctx, None, 0))
        buf = (_capi.RegionStats * max(n, 1))()
        if n:
            self._ck(fn(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("rule", "i8"), ("candidates", "i8"), ("changed", "i8")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def region_counters(self):
        """(firing steps, host synchronisations the rules caused) since the context was created."""
        f, s = C.c_int64(0), C.c_int64(0)
        self._ck(self._region_entry("region_counters")(self.ctx, C.byref(f), C.byref(s)))
        return int(f.value), int(s.value)

    # ---- radial distribution functions accumulated on the device (include/chem_mi355.h, chem_rdf_init ff.) ----
    def _rdf_entry(self, name):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("rdf: the CPU checker has no pair histogram")
        return fn

    def rdf_init(self, r_max, nbins, type_pairs=((-1, -1),), split_molecules=False):
        """Configure (and reset) the pair histograms: `nbins` bins up to r_max <= max_cutoff, one per unordered type pair of
        `type_pairs` (-1 = any type; at most 8), two (intra, inter molecule) with split_molecules.  No pairs switches it off."""
        fn = self._rdf_entry("rdf_init")
        tp = np.ascontiguousarray(type_pairs, dtype=np.int32).reshape(-1, 2)
        self._ck(fn(self.ctx, float(r_max), int(nbins), tp.shape[0], _ptr(tp, C.c_int32) if tp.shape[0] else None,
                    1 if split_molecules else 0))

    def rdf_sample(self):
        """One frame of the current positions (the preconditions of observe())."""
        self._ck(self._rdf_entry("rdf_sample")(self.ctx))

    def rdf_sample_every(self, every):
        """A frame inside run() at every step s with s % every == 0, without a host round trip; every <= 0: off."""
        self._ck(self._rdf_entry("rdf_sample_every")(self.ctx, int(every)))

    def rdf_reset(self):
        """Zero the accumulators, keep the configuration."""
        self._ck(self._rdf_entry("rdf_reset")(self.ctx))

    def rdf(self):
        """The accumulated histograms: dict of r (bin centres), edges, counts [npairs][parts][nbins] (exact integers), g (the
        same shape: counts / (density * shell volume), zeros before the first frame), frames, pairs and density per selector,
        r_max, nbins, split.  parts = 2 (intra, inter) with the molecule split, else 1."""
        fn = self._rdf_entry("rdf_get")
        res = _capi.RdfResult()
        self._ck(fn(self.ctx, C.byref(res), None, 0))
        nsel, parts, nbins = int(res.npairs), 1 + int(res.split), int(res.nbins)
        counts = np.zeros((nsel, parts, nbins), dtype=np.uint64)
        self._ck(fn(self.ctx, C.byref(res), _ptr(counts, C.c_uint64), counts.size))
        return rdf_result(float(res.r_max), counts, int(res.frames), np.array(res.pairs[:nsel], dtype=np.uint64),
                          np.array(res.density[:nsel], dtype=np.float64))

    # ---- static structure factor accumulated on the device (include/chem_mi355.h, chem_sq_init ff.) ----
    def _sq_entry(self, name):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("sq: the CPU checker has no structure factor")
        return fn

    def sq_init(self, nmax, type_pairs=((-1, -1),)):
        """Configure (and reset) the structure-factor sums: the wave vectors 2 pi n / L with |n_a| <= nmax <= 16 (canonical half,
        sq_vectors(nmax)), one set of sums per unordered type pair of `type_pairs` (-1 = any type; at most 4).  No pairs
        switches it off."""
        fn = self._sq_entry("sq_init")
        tp = np.ascontiguousarray(type_pairs, dtype=np.int32).reshape(-1, 2)
        self._ck(fn(self.ctx, int(nmax), tp.shape[0], _ptr(tp, C.c_int32) if tp.shape[0] else None))

    def sq_sample(self):
        """One frame of the current positions (the preconditions of observe())."""
        self._ck(self._sq_entry("sq_sample")(self.ctx))

    def sq_sample_every(self, every):
        """A frame inside run() at every step s with s % every == 0, without a host round trip; every <= 0: off."""
        self._ck(self._sq_entry("sq_sample_every")(self.ctx, int(every)))

    def sq_reset(self):
        """Zero the accumulators, keep the configuration."""
        self._ck(self._sq_entry("sq_reset")(self.ctx))

    def sq(self):
        """The accumulated structure factor: the dict of sq_result()."""
        fn = self._sq_entry("sq_get")
        res = _capi.SqResult()
        self._ck(fn(self.ctx, C.byref(res), None, 0))
        nsel, nvec = int(res.npairs), int(res.nvec)
        sums = np.zeros((nsel, nvec), dtype=np.float64)
        self._ck(fn(self.ctx, C.byref(res), _ptr(sums, C.c_double), sums.size))
        return sq_result(int(res.nmax), sums, int(res.frames), np.array(res.na[:nsel]), np.array(res.nb[:nsel]), np.array(res.box_sum[:3]))

    # ---- checkpoint and exact restart (include/chem_mi355.h, chem_checkpoint_save / chem_checkpoint_load) ----
    def _ckpt_entry(self, name):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("checkpoint: the CPU checker has no checkpoint")
        return fn

    def checkpoint_save(self, path=None):
        """The state of the context as bytes; with `path` it is written there instead (to a temporary name beside it, then
        renamed: a job that is killed while it writes leaves the last complete file) and the byte count is returned.  A set-up
        repeated on a fresh engine followed by checkpoint_load goes on bit for bit; the call is a list-build point."""
        fn = self._ckpt_entry("checkpoint_save")
        need = self._ck(fn(self.ctx, None, 0))
        buf = C.create_string_buffer(need)
        got = self._ck(fn(self.ctx, C.cast(buf, C.c_void_p), need))
        blob = buf.raw[:got]
        if path is None:
            return blob
        path = os.fspath(path)
        tmp = "%s.tmp.%d" % (path, os.getpid())
        with open(tmp, "wb") as f:
            f.write(blob)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
        return got

    def checkpoint_load(self, path_or_bytes):
        """Put back what checkpoint_save wrote (bytes, or the path of a file), after the set-up calls of the saved engine."""
        fn = self._ckpt_entry("checkpoint_load")
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            blob = bytes(path_or_bytes)
        else:
            with open(os.fspath(path_or_bytes), "rb") as f:
                blob = f.read()
        buf = C.create_string_buffer(max(len(blob), 1))
        C.memmove(buf, blob, len(blob))
        self._ck(fn(self.ctx, C.cast(buf, C.c_void_p), len(blob)))

    # ---- reverse reactions (include/chem_mi355.h, chem_reaction_remove_bond / chem_reaction_join) ----
    def _reverse_entry(self, name, what):
        fn = getattr(self.api, name, None)
        if fn is None:
            raise NotImplementedError("%s: the CPU checker has no reverse reactions" % what)
        return fn

    def reaction_remove_bond(self, reaction, invoke_on, anchor_type, nb_level, type_1, type_2, unexclude=False):
        """PostProcessRemoveNeighbourBond.add_bond_to_remove(anchor_type, nb_level, type_1, type_2) on the events of `reaction`:
        invoke_on 'type_1' | 'type_2' | 'both'."""
        fn = self._reverse_entry("reaction_remove_bond", "RemoveNeighboursBonds")
        io = {"type_1": 1, "type_2": 2, "both": 3}.get(invoke_on, invoke_on)
        r = _capi.NbRemove(int(reaction), int(io), int(anchor_type), int(nb_level), int(type_1), int(type_2), 1 if unexclude else 0, 0)
        self._ck(fn(self.ctx, C.byref(r)))

    def reaction_removed(self):
        """Removal records (step, id_near, id_far, list, reaction): one per (bond, list), by step, then visit order."""
        fn = self._reverse_entry("reaction_removed", "RemoveNeighboursBonds")
        n = self._ck(fn(self.ctx, None, 0))
        buf = (_capi.BondRecord * max(n, 1))()
        if n:
            self._ck(fn(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("id_near", "i8"), ("id_far", "i8"), ("list", "i4"), ("reaction", "i4")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def reaction_join(self, reaction, role, h, dist):
        """PostProcessJoinParticles(fd, dist): the reactant in `role` ('type_1' | 'type_2') anchors the other one in set `h`."""
        fn = self._reverse_entry("reaction_join", "JoinMolecule")
        self._ck(fn(self.ctx, int(reaction), {"type_1": 1, "type_2": 2}.get(role, role), int(h), float(dist)))

    def fix_joins(self):
        """Join records (step, anchor_id, target_id, set, cause): cause 3 = joined, 4 = refused, in visit order."""
        fn = self._reverse_entry("fix_joins", "JoinMolecule")
        n = self._ck(fn(self.ctx, None, 0))
        buf = (_capi.FixRecord * max(n, 1))()
        if n:
            self._ck(fn(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("anchor_id", "i8"), ("target_id", "i8"), ("set", "i4"), ("cause", "i4")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def list_create(self, arity, kind, by_types=False):
        kind = _capi.POT[kind] if isinstance(kind, str) else kind
        if kind == _capi.POT["COULOMB_BOND"] and getattr(self.api, "nb_coulomb", None) is None:
            raise NotImplementedError("1-4 Coulomb pairs: the CPU checker has no Coulomb term")
        h = self._ck(self.api.list_create(self.ctx, arity, kind, 1 if by_types else 0))
        self._lists[h] = arity
        return h

    def list_add(self, h, ids):
        a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1, self._lists[h])
        if a.shape[0]:
            self._ck(self.api.list_add(self.ctx, h, a.shape[0], _ptr(a, C.c_int64)))

    def list_set_params(self, h, params, types=None):
        p = np.ascontiguousarray(params, dtype=np.float64)
        t = list(types) if types is not None else []
        t = t + [-1] * (4 - len(t))
        self._ck(self.api.list_set_params(self.ctx, h, t[0], t[1], t[2], t[3], _ptr(p, C.c_double), p.shape[0]))

    def get_list(self, h):
        n = self._ck(self.api.get_list(self.ctx, h, None, 0))
        out = np.empty((n, self._lists[h]), dtype=np.int64)
        if n:
            self._ck(self.api.get_list(self.ctx, h, _ptr(out, C.c_int64), n))
        return out

    def list_set_hybrid(self, h, lambda0, rate):
        """Make the (still empty) pair list `h` hybrid: every entry acts with lambda = min(1, lambda0 + rate * (step - birth
        step)) on its force and energy (include/chem_mi355.h, chem_list_set_hybrid)."""
        fn = getattr(self.api, "list_set_hybrid", None)
        if fn is None:
            raise NotImplementedError("hybrid bonds: the CPU checker has no FixedPairListLambda")
        self._ck(fn(self.ctx, int(h), float(lambda0), float(rate)))

    def list_set_hybrid_tuples(self, h, lambda0, rate):
        """Make the (still empty) triple or quadruple list `h` hybrid: the same ramp as list_set_hybrid, on the angles and
        dihedrals that are added from now on (include/chem_mi355.h, chem_list_set_hybrid_tuples)."""
        fn = getattr(self.api, "list_set_hybrid_tuples", None)
        if fn is None:
            raise NotImplementedError("hybrid angles and dihedrals: the CPU checker has no FixedTripleListLambda / FixedQuadrupleListLambda")
        self._ck(fn(self.ctx, int(h), float(lambda0), float(rate)))

    def list_get_lambda(self, h):
        """lambda of every entry of list `h` at the current step, in the order of get_list."""
        fn = getattr(self.api, "list_get_lambda", None)
        if fn is None:
            raise NotImplementedError("hybrid bonds: the CPU checker has no FixedPairListLambda")
        n = self._ck(fn(self.ctx, int(h), None, 0))
        out = np.empty(n, dtype=np.float64)
        if n:
            self._ck(fn(self.ctx, int(h), _ptr(out, C.c_double), n))
        return out

    def thermostat_langevin(self, kT, gamma, seed=0):
        self._ck(self.api.thermostat_langevin(self.ctx, float(kT), float(gamma), int(seed)))

    def thermostat_langevin_types(self, types):
        """Thermal groups (LangevinThermostat.add_valid_types): thermalise only these particle types; [] = all."""
        t = np.ascontiguousarray(list(types), dtype=np.int32)
        self._ck(self.api.thermostat_langevin_types(self.ctx, t.shape[0], _ptr(t, C.c_int32)))

    def table_create(self, r0, dr, e, f, itype=1):
        """Bond table (rows of a .pot file); returns the handle to pass as list_set_params(h, [handle]).  itype as nb_table."""
        e = np.ascontiguousarray(e, dtype=np.float64); f = np.ascontiguousarray(f, dtype=np.float64)
        assert e.shape == f.shape
        if itype != 1:
            return self._ck(self._interp_entry("table_create_interp", itype)(self.ctx, e.shape[0], float(r0), float(dr), _ptr(e, C.c_double),
                                                                             _ptr(f, C.c_double), int(itype)))
        return self._ck(self.api.table_create(self.ctx, e.shape[0], float(r0), float(dr), _ptr(e, C.c_double), _ptr(f, C.c_double)))

    def thermostat_rescale(self, kind, kT, param):
        """kind: 'berendsen' (param = tau), 'isokinetic' (param = coupling steps) or None/0 (off)."""
        k = {None: 0, 0: 0, "berendsen": 1, 1: 1, "isokinetic": 2, 2: 2}[kind]
        self._ck(self.api.thermostat_rescale(self.ctx, k, float(kT), float(param)))

    def thermostat_svr(self, kT, coupling, seed=0):
        """StochasticVelocityRescaling: kT, coupling time (same units as dt); coupling <= 0 switches it off."""
        self._ck(self.api.thermostat_svr(self.ctx, float(kT), float(coupling), int(seed)))

    def cap_force(self, max_force):
        self._ck(self.api.cap_force(self.ctx, float(max_force)))

    def reaction_init(self, interval, nearest=True, max_per_interval=0, seed=0):
        self._ck(self.api.reaction_init(self.ctx, int(interval), 1 if nearest else 0, int(max_per_interval), int(seed)))

    def reaction_add(self, type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2,
                     max_state_2, rate, cutoff, bond_list=-1, min_cutoff=0.0, intramolecular=False,
                     intraresidual=False, is_virtual=False, active=True, new_type_1=-1, new_type_2=-1,
                     new_mass_1=0.0, new_mass_2=0.0, new_q_1=0.0, new_q_2=0.0):
        d = _capi.ReactionDesc(type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2,
                               max_state_2, rate, cutoff, min_cutoff, int(bool(intramolecular)),
                               int(bool(intraresidual)), int(bool(is_virtual)), int(bool(active)),
                               bond_list, new_type_1, new_type_2, new_mass_1, new_mass_2, new_q_1, new_q_2)
        return self._ck(self.api.reaction_add(self.ctx, C.byref(d)))

    def dissociation_add(self, type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2, max_state_2,
                         diss_rate, cutoff, bond_list, unexclude=True, active=True, new_type_1=-1, new_type_2=-1,
                         new_mass_1=0.0, new_mass_2=0.0, new_q_1=0.0, new_q_2=0.0):
        """Dissociation reaction on the pair list `bond_list`: a bond breaks when it is longer than `cutoff` (> 0) or with
        probability diss_rate * dt * interval (rule set: include/chem_mi355.h).  Returns the reaction index, which shares
        the index space of reaction_add."""
        d = _capi.DissociationDesc(type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2, max_state_2,
                                   float(diss_rate), float(cutoff), int(bond_list), int(bool(unexclude)), int(bool(active)),
                                   new_type_1, new_type_2, 0, new_mass_1, new_mass_2, new_q_1, new_q_2)
        return self._ck(self.api.dissociation_add(self.ctx, C.byref(d)))

    def reaction_neighbour_change(self, reaction, invoke_on, old_type, nb_level, new_type, new_mass, new_q=0.0, new_state=None,
                                  incr_state=None, state_window=None):
        """PostProcessChangeNeighboursProperty rule for the events of `reaction` (index from reaction_add):
        invoke_on 'type_1' | 'type_2' | 'both'; new_state None keeps the chemical state, incr_state adds to it;
        state_window (min, max): only neighbours whose state is in [min, max)."""
        io = {"type_1": 1, "type_2": 2, "both": 3, 1: 1, 2: 2, 3: 3}[invoke_on]
        mode, val = (2, int(incr_state)) if incr_state is not None else ((1, int(new_state)) if new_state is not None else (0, 0))
        lo, hi = (0, 0) if state_window is None else (int(state_window[0]), int(state_window[1]))
        r = _capi.NbChange(int(reaction), io, int(old_type), int(nb_level), int(new_type), mode, val, 0, float(new_mass), float(new_q), lo, hi)
        self._ck(self.api.reaction_neighbour_change(self.ctx, C.byref(r)))

    def reaction_constraint(self, reaction, role, nb_type, min_state, max_state):
        """ReactionConstraintNeighbourState on role 'type_1' | 'type_2' of `reaction` (reaction_setup.py:203-204)."""
        ro = {"type_1": 1, "type_2": 2, 1: 1, 2: 2}[role]
        self._ck(self.api.reaction_constraint(self.ctx, int(reaction), ro, int(nb_type), int(min_state), int(max_state)))

    def reaction_restrict(self, reaction, id_pairs):
        """RestrictReaction.define_connection: only these unordered id pairs may react in `reaction` (index from reaction_add)."""
        p = np.ascontiguousarray(id_pairs, dtype=np.int64).reshape(-1, 2)
        self._ck(self.api.reaction_restrict(self.ctx, int(reaction), p.shape[0], _ptr(p, C.c_int64)))

    def atrp_init(self, interval, num_particles, ratio_activator, ratio_deactivator, delta_catalyst, k_activate, k_deactivate,
                  select_from_all=True, seed=0):
        """integrator.ATRPActivator(system, interval, num_particles, ...) (reaction_post_process.py:380-426)."""
        d = _capi.AtrpDesc(int(interval), int(num_particles), 1 if select_from_all else 0, 0, float(ratio_activator), float(ratio_deactivator),
                           float(delta_catalyst), float(k_activate), float(k_deactivate), int(seed))
        self._ck(self.api.atrp_init(self.ctx, C.byref(d)))

    def atrp_disconnect(self):
        self._ck(self.api.atrp_init(self.ctx, None))

    def atrp_add_center(self, type_id, state, is_activator, new_type, new_mass, new_q=0.0, delta_state=0):
        self._ck(self.api.atrp_add_center(self.ctx, int(type_id), int(state), 1 if is_activator else 0, int(new_type), float(new_mass), float(new_q), int(delta_state)))

    def atrp_stats(self):
        n = self._ck(self.api.atrp_get_stats(self.ctx, None, 0))
        buf = (_capi.AtrpStats * max(n, 1))()
        if n:
            self._ck(self.api.atrp_get_stats(self.ctx, buf, n))
        return [{k: getattr(buf[i], k) for k, _ in _capi.AtrpStats._fields_} for i in range(n)]

    def topology_register(self, h, types):
        t = np.ascontiguousarray(types, dtype=np.int32)
        self._ck(self.api.topology_register(self.ctx, t.shape[0], h, _ptr(t, C.c_int32)))

    def reactions_enable(self, on=True):
        self._ck(self.api.reactions_enable(self.ctx, 1 if on else 0))

    def reaction_set_rate(self, r, rate):
        self._ck(self.api.reaction_set_rate(self.ctx, r, float(rate)))

    # ---- hot call ----
    def run(self, nsteps):
        self._ck(self.api.run(self.ctx, int(nsteps)))

    # ---- read-back ----
    @property
    def n(self):
        return self.api.num_particles(self.ctx)

    @property
    def step(self):
        return self.api.get_step(self.ctx)

    def get_state(self, what):
        w = _capi.STATE[what.upper()]
        if what.upper() == "LAMBDA":
            self._res_entry("set_resolution")
        n = self.n
        if what.upper() in ("POS", "VEL", "FORCE", "POS_UNFOLDED"):
            out = np.empty((n, 3), dtype=np.float64)
        elif what.upper() == "IMAGE":
            out = np.empty((n, 3), dtype=np.int32)
        elif what.upper() in ("MASS", "CHARGE", "LAMBDA"):
            out = np.empty(n, dtype=np.float64)
        elif what.upper() == "ID":
            out = np.empty(n, dtype=np.int64)
        else:
            out = np.empty(n, dtype=np.int32)
        self._ck(self.api.get_state(self.ctx, w, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def get_events(self):
        n = self._ck(self.api.get_events(self.ctx, None, 0))
        buf = (_capi.Event * max(n, 1))()
        if n:
            self._ck(self.api.get_events(self.ctx, buf, n))
        dt = np.dtype([("step", "i8"), ("id_a", "i8"), ("id_b", "i8"), ("reaction", "i4"), ("pad", "i4"), ("r2", "f8")])
        return np.frombuffer(buf, dtype=dt, count=n).copy()

    def get_exclusions(self):
        n = self._ck(self.api.get_exclusions(self.ctx, None, 0))
        out = np.empty((n, 2), dtype=np.int64)
        if n:
            self._ck(self.api.get_exclusions(self.ctx, _ptr(out, C.c_int64), n))
        return out

    def get_verlet_pairs(self):
        n = self._ck(self.api.get_verlet_pairs(self.ctx, None, 0))
        out = np.empty((n, 2), dtype=np.int64)
        if n:
            self._ck(self.api.get_verlet_pairs(self.ctx, _ptr(out, C.c_int64), n))
        return out

    def debug_force_list(self, tag):
        """Diagnostic (tests): partner tags of the 16-bit force list of particle `tag`, in list order."""
        lib = self.api.lib
        lib.chem_debug_force_list.restype = C.c_int64
        buf = np.zeros(1024, dtype=np.int32)
        m = lib.chem_debug_force_list(C.c_void_p(self.ctx), C.c_int32(int(tag)), buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.size))
        if m < 0:
            raise ChemError(int(m), "force list not available (no LDS tiles)")
        return buf[:m].copy()

    def debug_row_order(self, tile):
        """Diagnostic (tests): stored order of the force-list rows of tile descriptor `tile` (option row_order):
        (entries of the row at every position, home -- index in the tile's cell-run order -- of every position)."""
        lib = self.api.lib
        lib.chem_debug_row_order.restype = C.c_int64
        nh = lib.chem_debug_row_order(C.c_void_p(self.ctx), C.c_int32(int(tile)), None, C.c_int64(0))
        if nh < 0:
            raise ChemError(int(nh), "row order not available (no LDS tiles)")
        buf = np.zeros(2 * max(int(nh), 1), dtype=np.int32)
        m = lib.chem_debug_row_order(C.c_void_p(self.ctx), C.c_int32(int(tile)), buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.size))
        if m != nh:
            raise ChemError(int(m), "row order read-back failed")
        return buf[:nh].copy(), buf[nh:2 * nh].copy()

    def observe(self):
        o = _capi.Obs()
        self._ck(self.api.observe(self.ctx, C.byref(o)))
        nl = len(self._lists)
        return dict(step=o.step, npart=o.npart, ekin=o.ekin, temperature=o.temperature,
                    epot_lj=o.epot_lj, epot_tab=o.epot_tab, epot_list=list(o.epot_list)[:nl],
                    list_size=list(o.list_size)[:nl], momentum=list(o.momentum), virial_nb=o.virial_nb)

    # ---- pressure, Berendsen barostat, current box (include/chem_mi355.h "pressure and barostat") ----
    def pressure(self):
        """P = (sum m v^2 + W) / (3 V) at the current state, with its parts: volume, mv2, virial_nb, virial_list, virial."""
        fn = getattr(self.api, "get_pressure", None)
        if fn is None:
            raise NotImplementedError("Pressure: the CPU checker has no virial of the bonded lists")
        p = _capi.Pressure()
        self._ck(fn(self.ctx, C.byref(p)))
        return dict(pressure=p.pressure, volume=p.volume, mv2=p.mv2, virial_nb=p.virial_nb,
                    virial_list=list(p.virial_list)[:len(self._lists)], virial=p.virial)

    def pressure_tensor(self):
        """Pi_ab = (K_ab + W_ab) / V at the current state, components in the order xx, yy, zz, xy, xz, yz: dict(volume,
        kinetic[6], virial_nb[6], virial_list[lists, 6], virial[6], tensor[6]) of numpy arrays."""
        fn = getattr(self.api, "get_pressure_tensor", None)
        if fn is None:
            raise NotImplementedError("PressureTensor: the CPU checker has no virial tensor")
        p = _capi.PressureTensor()
        self._ck(fn(self.ctx, C.byref(p)))
        nl = len(self._lists)
        return dict(volume=p.volume, kinetic=np.array(p.kinetic, dtype=np.float64), virial_nb=np.array(p.virial_nb, dtype=np.float64),
                    virial_list=np.array([list(p.virial_list[l]) for l in range(nl)], dtype=np.float64).reshape(nl, 6),
                    virial=np.array(p.virial, dtype=np.float64), tensor=np.array(p.tensor, dtype=np.float64))

    def barostat_berendsen(self, pressure, tau):
        """Isotropic Berendsen barostat on every step; tau <= 0 switches it off."""
        fn = getattr(self.api, "barostat_berendsen", None)
        if fn is None:
            raise NotImplementedError("BerendsenBarostat: the CPU checker has no barostat (its box is fixed)")
        self._ck(fn(self.ctx, float(pressure), float(tau)))

    def barostat_langevin(self, pressure, mass, gammaP, kT, seed=0):
        """Langevin piston barostat (isotropic) on every step; mass <= 0 switches it off and resets the piston momentum."""
        fn = getattr(self.api, "barostat_langevin", None)
        if fn is None:
            raise NotImplementedError("LangevinBarostat: the CPU checker has no barostat (its box is fixed)")
        self._ck(fn(self.ctx, float(pressure), float(mass), float(gammaP), float(kT), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def barostat_state(self):
        """dict(kind, pressure_last, momentum, eps_dot, mu_next, sv_next): kind 0 off, 1 Berendsen, 2 Langevin piston."""
        fn = getattr(self.api, "barostat_state_get", None)
        if fn is None:
            raise NotImplementedError("LangevinBarostat: the CPU checker has no barostat (its box is fixed)")
        s = _capi.BarostatState()
        self._ck(fn(self.ctx, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _capi.BarostatState._fields_}

    def box(self):
        """The current box edges (they move while a barostat is on)."""
        fn = getattr(self.api, "get_box", None)
        if fn is None:
            raise NotImplementedError("box: the CPU checker has no read-back of the box (it is fixed: what set_box was given)")
        L = np.zeros(3)
        self._ck(fn(self.ctx, _ptr(L, C.c_double)))
        return L

    def timers(self):
        t = _capi.Timers()
        self._ck(self.api.get_timers(self.ctx, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _capi.Timers._fields_}

    # ---- product-only knobs ----
    def set_option(self, name, value):
        self._ck(self.api.set_option(self.ctx, name.encode(), float(value)))

    def set_nlist_capacity(self, n):
        self._ck(self.api.set_nlist_capacity(self.ctx, int(n)))

    def comm_init(self, nranks, rank, uid):
        """Join the slab decomposition (node grid (1,1,nranks)); uid from comm_unique_id() on rank 0."""
        grid = (C.c_int * 3)(1, 1, nranks)
        self._ck(self.api.comm_init(self.ctx, nranks, rank, grid, uid))

    def comm_init_ipc(self, nranks, rank, shm_name):
        """One process per rank over hipIpc handles (ranks may share a device); shm_name: same fresh name on all ranks."""
        self._ck(self.api.comm_init_ipc(self.ctx, nranks, rank, shm_name.encode()))

    def comm_init_local(self, nranks, rank, hub_id):
        self._ck(self.api.comm_init_local(self.ctx, nranks, rank, hub_id))

    def sync(self):
        self._ck(self.api.device_sync(self.ctx))
