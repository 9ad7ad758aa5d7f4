"""py3 `espressopp`-shaped shim over the C ABI (include/chem_mi355.h).

ChemLab reaches its hot path through Boost.Python objects of the external module `espressopp`
(`import espressopp`, /root/reference/src/start_simulation.py:20).  This module exposes the subset
of that surface the in-scope driver logic touches, with the same names, argument
meaning and error behaviour, implemented on one `chemlab_amd.engine.Engine` per `System`.
Everything outside the hot-path scope raises NotImplementedError naming the symbol.

    import chemlab_amd.espp as espressopp
    system = espressopp.System()
    ...
    integrator.run(n)          # -> chem_run(ctx, n)

The engine factory is replaceable (`set_engine_factory`) so that tests can drive the very same
driver code with the CPU oracle.
"""
import math
import types

import numpy as np

from ..engine import Engine
from .. import rank as _rank

_factory = [lambda: Engine(device=0, precision=32)]


def set_engine_factory(fn):
    """fn() -> Engine-like object (tests: the CPU oracle)."""
    _factory[0] = fn


class Real3D(object):
    def __init__(self, x=0.0, y=None, z=None):
        if y is None:
            v = list(x) if hasattr(x, "__len__") else [x, x, x]
            x, y, z = v
        self.v = np.array([x, y, z], dtype=np.float64)

    def __getitem__(self, i):
        return self.v[i]

    def __len__(self):
        return 3

    def __iter__(self):
        return iter(self.v)

    def __mul__(self, s):
        return Real3D(*(self.v * s))

    def __repr__(self):
        return "Real3D(%g, %g, %g)" % tuple(self.v)


class Int3D(Real3D):
    pass


def _unsupported(name):
    def ctor(*a, **k):
        raise NotImplementedError("espressopp.%s is outside the MI355X hot-path scope (SURVEY.md 8b)" % name)
    return ctor


# --------------------------------------------------------------------------------------------
class System(object):
    """espressopp.System(): .rng .skin .bc .storage .integrator (start_simulation.py:148-163)."""

    def __init__(self):
        self.engine = _factory[0]()
        self.rng = None
        self.skin = 0.0
        self.bc = None
        self.storage = None
        self.integrator = None
        self.topology_manager = None
        self._interactions = []     # (interaction, name)
        self.max_cutoff = None

    def addInteraction(self, interaction, name=None):
        self._interactions.append((interaction, name if name is not None else "interaction_%d" % len(self._interactions)))

    def getAllInteractions(self):
        return {name: i for i, name in self._interactions}

    def getNumberOfInteractions(self):
        return len(self._interactions)

    def getInteraction(self, k):
        return self._interactions[k][0]

    def getNameOfInteraction(self, k):
        return self._interactions[k][1]


class _RNG(object):
    def __init__(self, seed=0):
        self._seed = int(seed)

    def seed(self, s):
        self._seed = int(s)

    def get_seed(self):
        return self._seed


class _OrthorhombicBC(object):
    def __init__(self, rng, boxL):
        self.rng = rng
        self._boxL = Real3D(*[float(b) for b in boxL])
        self._engine = None      # set by the storage: from then on the box is the engine's (a barostat moves it)

    @property
    def boxL(self):
        """The box as it is now: read from the engine at every access, so that every writer prints the current one."""
        if self._engine is not None:
            try:
                self._boxL = Real3D(*[float(b) for b in self._engine.box()])
            except NotImplementedError:      # the CPU checker: the box it was given
                pass
        return self._boxL


class _Particle(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _DomainDecomposition(object):
    """storage.DomainDecomposition(system, nodeGrid, cellGrid): addParticles/decompose/getParticle/
    modifyParticle (start_simulation.py:163-171; examples/atrp_lj/hooks.py:63-65)."""

    def __init__(self, system, nodeGrid=None, cellGrid=None):
        self.system = system
        self.nodeGrid, self.cellGrid = nodeGrid, cellGrid
        self._pending = []
        self._props = None
        self._uploaded = False
        system.engine.set_box(list(system.bc.boxL))
        system.bc._engine = system.engine

    def addParticles(self, plist, *props):
        if self._uploaded:          # the particle set is on the engine: the new ones are appended (chem_add_particles)
            self._append(list(plist), list(props))
            return
        self._props = list(props)
        self._pending.extend(plist)

    def _append(self, plist, pr):
        """addParticles after the upload (the dummies of ReleaseMolecule, reaction_post_process.py:262): ids above every
        present one; lists, exclusions, lambda stamps and reactions of the engine are kept."""
        if not plist:
            return
        col = lambda name, default=None: [p[pr.index(name)] for p in plist] if name in pr else default
        n = len(plist)
        ids = np.array(col("id"), dtype=np.int64)
        vel = np.array([list(p) for p in col("v")], dtype=np.float64) if "v" in pr else None
        self.system.engine.add_particles(ids, np.array(col("type", [0] * n), dtype=np.int32), np.array([list(p) for p in col("pos")], dtype=np.float64),
                                         np.array(col("mass", [1.0] * n), dtype=np.float64), vel=vel, q=np.array(col("q", [0.0] * n), dtype=np.float64),
                                         state=np.array(col("state", [0] * n), dtype=np.int32), res_id=np.array(col("res_id", list(ids)), dtype=np.int32))
        if "lambda_adr" in pr:
            lam = np.array(col("lambda_adr"), dtype=np.float64)
            if np.any(lam != 1.0):
                self.system.engine.set_resolution(ids, lam)
        self._ids = np.concatenate([self._ids, ids])

    def addParticle(self, pid, pos):
        self._props = ["id", "pos"]
        self._pending.append([pid, pos])

    def decompose(self):
        if self._uploaded or not self._pending:
            return
        pr = self._props
        col = lambda name, default=None: [p[pr.index(name)] for p in self._pending] if name in pr else default
        n = len(self._pending)
        ids = np.array(col("id"), dtype=np.int64)
        pos = np.array([list(p) for p in col("pos")], dtype=np.float64)
        types = np.array(col("type", [0] * n), dtype=np.int32)
        mass = np.array(col("mass", [1.0] * n), dtype=np.float64)
        q = np.array(col("q", [0.0] * n), dtype=np.float64)
        res_id = np.array(col("res_id", list(ids)), dtype=np.int32)
        state = np.array(col("state", [0] * n), dtype=np.int32)
        vel = None
        if "v" in pr:
            vel = np.array([list(p) for p in col("v")], dtype=np.float64)
        self.system.engine.set_particles(ids, types, pos, mass, vel=vel, q=q, state=state, res_id=res_id)
        if "lambda_adr" in pr:          # per-particle resolution (1 unless given): nothing is sent while every value is 1
            lam = np.array(col("lambda_adr"), dtype=np.float64)
            if np.any(lam != 1.0):
                self.system.engine.set_resolution(ids, lam)
        self._uploaded = True
        self._ids = ids
        self._pending = []

    def particleExists(self, pid):
        return bool(np.any(self._ids == pid))

    def getParticle(self, pid):
        e = self.system.engine
        k = int(np.searchsorted(np.sort(self._ids), pid))
        g = lambda w: e.get_state(w)[k]
        # (the CPU checker keeps no charges: an engine without the Coulomb entry points reports 0, as before)
        q = float(g("CHARGE")) if getattr(getattr(e, "api", None), "nb_coulomb", None) is not None else 0.0
        # (nor a resolution: every particle is at full resolution there)
        lam = float(g("LAMBDA")) if getattr(getattr(e, "api", None), "set_resolution", None) is not None else 1.0
        return _Particle(lambda_adr=lam, id=pid, pos=Real3D(*g("POS")), v=Real3D(*g("VEL")), f=Real3D(*g("FORCE")), type=int(g("TYPE")),
                         mass=float(g("MASS")), state=int(g("STATE")), res_id=int(g("RESID")), imageBox=Int3D(*g("IMAGE")), q=q)

    def modifyParticle(self, pid, prop, value):
        self.system.engine.modify_particle(pid, {"type": "TYPE", "state": "STATE", "mass": "MASS", "res_id": "RESID", "q": "CHARGE", "lambda_adr": "LAMBDA"}[prop], value)


def _node_grid(n, *a, **k):
    """tools.decomp.nodeGrid(MPI size): this build decomposes along z only (multigpu.node_grid)."""
    return Int3D(1, 1, int(n))


def _cell_grid(box, node_grid, rc, skin, *a, **k):
    """tools.decomp.cellGrid(box, nodeGrid, max_cutoff, skin): cells of edge >= rc+skin per node;
    known answer examples/atrp_lj/single:39 -> (6, 6, 6) for box 13.40248, rc 2.0, skin 0.1."""
    rl = rc + skin
    ng = list(node_grid)
    g = [int(math.floor(float(box[d]) / (rl * ng[d]))) for d in range(3)]
    if min(g) < 1:
        raise RuntimeError("local box too small for the cutoff + skin")
    return Int3D(*g)


class DynamicExcludeList(object):
    """espressopp.DynamicExcludeList(integrator, pairs) (start_simulation.py:189); the device list
    observes every Fixed*List by construction, observe_* only record the request."""

    def __init__(self, integrator, exclusions=None):
        self.system = integrator.system
        self.exclusions = [tuple(p) for p in (exclusions or [])]
        if self.exclusions:
            self.system.engine.set_exclusions(self.exclusions)
        self.observed = []

    def exclude(self, a, b):
        self.exclusions.append((a, b))
        self.system.engine.set_exclusions(self.exclusions)

    def observe_tuple(self, fpl):
        self.observed.append(fpl)

    observe_triple = observe_quadruple = observe_tuple

    def get_list(self):
        return [tuple(p) for p in self.system.engine.get_exclusions().tolist()]

    @property
    def size(self):
        return len(self.system.engine.get_exclusions())


class VerletList(object):
    """espressopp.VerletList(system, cutoff, exclusionlist) (start_simulation.py:193-197)."""

    def __init__(self, system, cutoff, exclusionlist=None):
        self.system, self.cutoff, self.exclusionlist = system, cutoff, exclusionlist
        system.max_cutoff = cutoff
        system.engine.set_cutoff(cutoff, system.skin)

    def totalSize(self):
        return len(self.system.engine.get_verlet_pairs())

    def get_timers(self):
        return []


# ---- fixed lists ---------------------------------------------------------------------------
class _FixedList(object):
    """One espressopp list object may carry interactions of several kinds (the 1-4 pairs: LennardJones and CoulombTruncated on
    the same FixedPairList, gromacs_topology.py:1391-1409); a library list has one kind.  So there is one library handle per
    kind: `handle` is the first (what reactions, the topology manager and getAll* see), a bind with another kind creates a
    further library list with the entries added through this object so far, and later additions go to all of them."""
    arity = 2

    def __init__(self, storage):
        self.system = storage.system
        self.handle = None
        self._handles = {}      # kind -> library handle, in the order of binding
        self._pending = []
        self._entries = []      # everything _add has seen (what a further kind starts with)

    def _add(self, entries):
        entries = [tuple(int(x) for x in e) for e in entries]
        self._entries.extend(entries)
        if self.handle is None:
            self._pending.extend(entries)
        elif entries:
            for h in self._handles.values():
                self.system.engine.list_add(h, entries)

    def _create(self, kind, by_types):
        return self.system.engine.list_create(self.arity, kind, by_types)

    def _bind(self, kind, by_types):
        if kind in self._handles:
            return self._handles[kind]
        h = self._create(kind, by_types)
        if self._entries:
            self.system.engine.list_add(h, self._entries)
        if self.handle is None:
            self.handle = h
            self._pending = []
        self._handles[kind] = h
        return h

    def _all(self):
        if self.handle is None:
            return list(self._pending)
        return [tuple(r) for r in self.system.engine.get_list(self.handle).tolist()]

    def totalSize(self):
        return len(self._all())

    size = totalSize


class FixedPairList(_FixedList):
    arity = 2

    def addBonds(self, bonds):
        self._add(bonds)

    def add(self, a, b):
        self._add([(a, b)])

    def getAllBonds(self):
        return self._all()

    getBonds = getAllBonds


class FixedPairListLambda(FixedPairList):
    """espressopp.FixedPairListLambda(storage, init_lambda) (reaction_setup.py:444-467): a pair list whose entries act with
    lambda = min(1, init_lambda + rate * (step - birth step)); the rate comes from
    integrator.FixedListDynamicResolution.register_pair_list (include/chem_mi355.h, chem_list_set_hybrid)."""

    def __init__(self, storage, init_lambda=0.0):
        FixedPairList.__init__(self, storage)
        self.init_lambda, self.rate = float(init_lambda), 0.0

    def _create(self, kind, by_types):      # (hybrid before the first entry: the engine refuses it on a list that has entries)
        e = self.system.engine
        h = e.list_create(self.arity, kind, by_types)
        e.list_set_hybrid(h, self.init_lambda, self.rate)
        return h

    def _set_rate(self, rate):
        self.rate = float(rate)
        for h in self._handles.values():
            self.system.engine.list_set_hybrid(h, self.init_lambda, self.rate)

    def getAllLambda(self):
        """lambda of every bond at the current step, in the order of getAllBonds."""
        if self.handle is None:
            return [self.init_lambda] * len(self._pending)
        return self.system.engine.list_get_lambda(self.handle).tolist()


class FixedTripleList(_FixedList):
    arity = 3

    def addTriples(self, t):
        self._add(t)

    def getAllTriples(self):
        return self._all()


class FixedQuadrupleList(_FixedList):
    arity = 4

    def addQuadruples(self, t):
        self._add(t)

    def getAllQuadruples(self):
        return self._all()


class _LambdaTuples(object):
    """What FixedTripleListLambda and FixedQuadrupleListLambda add to their plain lists: entries act with lambda = min(1,
    init_lambda + rate * (step - birth step)); the rate comes from integrator.FixedListDynamicResolution.register_triple_list /
    register_quadruple_list (include/chem_mi355.h, chem_list_set_hybrid_tuples)."""

    def _create(self, kind, by_types):      # (hybrid before the first entry: the engine refuses it on a list that has entries)
        e = self.system.engine
        h = e.list_create(self.arity, kind, by_types)
        e.list_set_hybrid_tuples(h, self.init_lambda, self.rate)
        return h

    def _set_rate(self, rate):
        self.rate = float(rate)
        for h in self._handles.values():
            self.system.engine.list_set_hybrid_tuples(h, self.init_lambda, self.rate)

    def getAllLambda(self):
        """lambda of every entry at the current step, in the order of getAllTriples / getAllQuadruples."""
        if self.handle is None:
            return [self.init_lambda] * len(self._pending)
        return self.system.engine.list_get_lambda(self.handle).tolist()


class FixedTripleListLambda(_LambdaTuples, FixedTripleList):
    """espressopp.FixedTripleListLambda(storage, init_lambda): the angles of a hybrid triple list."""

    def __init__(self, storage, init_lambda=0.0):
        FixedTripleList.__init__(self, storage)
        self.init_lambda, self.rate = float(init_lambda), 0.0


class FixedQuadrupleListLambda(_LambdaTuples, FixedQuadrupleList):
    """espressopp.FixedQuadrupleListLambda(storage, init_lambda): the dihedrals of a hybrid quadruple list."""

    def __init__(self, storage, init_lambda=0.0):
        FixedQuadrupleList.__init__(self, storage)
        self.init_lambda, self.rate = float(init_lambda), 0.0


# ---- potentials (parameter holders) -----------------------------------------------------------
class _Pot(object):
    kind = None

    def params(self):
        raise NotImplementedError


class _LennardJones(_Pot):
    def __init__(self, epsilon=1.0, sigma=1.0, cutoff=2.5, shift="auto"):
        self.epsilon, self.sigma, self.cutoff, self.shift = epsilon, sigma, cutoff, shift


class _Tabulated(_Pot):
    """interaction.Tabulated(itype, filename, cutoff): rows `r e f` of an ESPResSo++ .pot file; itype 1 linear, 2 Akima,
    3 natural cubic spline (rule set: include/chem_mi355.h, chem_nb_table_interp)."""

    def __init__(self, itype=1, filename=None, cutoff=None):
        if itype not in (1, 2, 3):
            raise NotImplementedError("Tabulated itype %r (1 linear, 2 Akima, 3 cubic spline)" % (itype,))
        self.itype, self.filename, self.cutoff = itype, filename, cutoff
        tab = np.loadtxt(filename)
        self.r, self.e, self.f = tab[:, 0], tab[:, 1], tab[:, 2]
        self.r0, self.dr = float(self.r[0]), float(self.r[1] - self.r[0])


def _interp_kw(pot):
    """Keyword for Engine.nb_table / table_create: none for linear tables, so that an engine with linear tables only (the
    CPU checker) is driven exactly as before; a spline kind there is refused by Engine, never evaluated linearly."""
    return {} if pot.itype == 1 else {"itype": pot.itype}


class _MixedTabulated(_Pot):
    """interaction.MixedTabulated(itype, table1, table2, chemical_conversion=None, cutoff=None, mix_value=None)
    (gromacs_topology.py:756-790, nonbond_params func 10 / 12): U = x * table1 + (1 - x) * table2 with x the value of a
    ChemicalConversion observable (func 10: followed whenever the observable is computed) or a constant (func 12).
    Linear interpolation is linear in the rows, so the mixture IS one table: x * rows1 + (1 - x) * rows2 -- re-sent to the
    engine (chem_nb_table) when x changes; the kernels see an ordinary tabulated pair potential."""

    def __init__(self, itype=1, table1=None, table2=None, chemical_conversion=None, cutoff=None, mix_value=None):
        if itype != 1:
            raise NotImplementedError("MixedTabulated itype %r (only linear interpolation, itype=1, is in scope)" % itype)
        a, b = np.loadtxt(table1), np.loadtxt(table2)
        if a.shape != b.shape or not np.allclose(a[:, 0], b[:, 0], rtol=0, atol=1e-12):
            raise ValueError("MixedTabulated: %s and %s are not on the same r grid" % (table1, table2))
        self.table1, self.table2, self.cutoff = table1, table2, cutoff
        self.r, self._e, self._f = a[:, 0], (a[:, 1], b[:, 1]), (a[:, 2], b[:, 2])
        self.r0, self.dr = float(self.r[0]), float(self.r[1] - self.r[0])
        self.observable = chemical_conversion
        self.mix_value = 0.0 if mix_value is None else float(mix_value)

    def rows(self, x):
        return x * self._e[0] + (1.0 - x) * self._e[1], x * self._f[0] + (1.0 - x) * self._f[1]


class _TabulatedAngular(_Tabulated):
    """interaction.TabulatedAngular(itype, filename): rows `theta U -dU/dtheta` (radians) of a table_a<N>.pot file."""


class _TabulatedDihedral(_Tabulated):
    """interaction.TabulatedDihedral(itype, filename): rows `phi U -dU/dphi` (radians, [-pi, pi]) of a table_d<N>.pot file."""


class _Harmonic(_Pot):
    kind = "HARMONIC"

    def __init__(self, K=1.0, r0=0.0, cutoff=None, shift=0.0):
        self.K, self.r0 = K, r0

    def params(self):
        return [self.K, self.r0]


class _FENE(_Pot):
    kind = "FENE"

    def __init__(self, K=1.0, r0=0.0, rMax=1.0, cutoff=None, shift=0.0):
        self.K, self.r0, self.rMax = K, r0, rMax

    def params(self):
        return [self.K, self.r0, self.rMax]


class _FENELennardJones(_Pot):
    """interaction.FENELennardJones(K, r0, rMax, sigma, epsilon) (bond func 9, gromacs_topology.py:935-942)."""
    kind = "FENE_LJ"

    def __init__(self, K=1.0, r0=0.0, rMax=1.0, sigma=1.0, epsilon=1.0, cutoff=None, shift=0.0):
        self.K, self.r0, self.rMax, self.sigma, self.epsilon = K, r0, rMax, sigma, epsilon

    def params(self):
        return [self.K, self.r0, self.rMax, self.sigma, self.epsilon]


class _LJBond(_Pot):
    """LennardJones as the potential of a FixedPairListLennardJones (1-4 pairs, gromacs_topology.py:1314-1411)."""
    kind = "LJ_BOND"


class _DihedralHarmonic(_Pot):
    """interaction.DihedralHarmonic(K, phi0) (dihedral func 12, gromacs_topology.py:1199-1202)."""
    kind = "DIH_HARMONIC"

    def __init__(self, K=0.0, phi0=0.0):
        self.K, self.phi0 = K, phi0

    def params(self):
        return [self.K, self.phi0]


class _AngularHarmonic(_Pot):
    kind = "ANG_HARMONIC"

    def __init__(self, K=1.0, theta0=0.0):
        self.K, self.theta0 = K, theta0

    def params(self):
        return [self.K, self.theta0]


class _Cosine(_Pot):
    kind = "ANG_COSINE"

    def __init__(self, K=1.0, theta0=0.0):
        self.K, self.theta0 = K, theta0

    def params(self):
        return [self.K, self.theta0]


class _DihedralHarmonicNCos(_Pot):
    kind = "DIH_NCOS"

    def __init__(self, K=0.0, phi0=0.0, multiplicity=1):
        self.K, self.phi0, self.n = K, phi0, multiplicity

    def params(self):
        return [self.K, self.phi0, float(self.n)]


class _DihedralRB(_Pot):
    kind = "DIH_RB"

    def __init__(self, K0=0.0, K1=0.0, K2=0.0, K3=0.0, K4=0.0, K5=0.0):
        self.C = [K0, K1, K2, K3, K4, K5]

    def params(self):
        return list(self.C)


# ---- interactions ----------------------------------------------------------------------------
class _VerletListInteraction(object):
    def __init__(self, vl):
        self.vl, self.system = vl, vl.system
        self._pots = {}

    def getPotential(self, t1, t2):
        return self._pots[(min(t1, t2), max(t1, t2))]

    def getAllPotentials(self):
        return dict(self._pots)


class _VerletListLennardJones(_VerletListInteraction):
    label = "lj"

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential
        self.system.engine.nb_lj(type1, type2, potential.epsilon, potential.sigma, potential.cutoff, potential.shift == "auto")


class _VerletListTabulated(_VerletListInteraction):
    label = "tab"

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential
        self.system.engine.nb_table(type1, type2, potential.r0, potential.dr, potential.e, potential.f, potential.cutoff, **_interp_kw(potential))


class _VerletListDynamicResolution(_VerletListInteraction):
    """interaction.VerletListDynamicResolutionLennardJones / ...Tabulated(vl, cg_potential) (gromacs_topology.py:584-600,
    819-862): the pair potential times lambda_i lambda_j, the scaled force capped at max_force (setMaxForce; rule set:
    include/chem_mi355.h, chem_nb_resolution).  cg_potential = True (weight 1 - lambda_i lambda_j) is not built."""

    def __init__(self, vl, cg_potential=False):
        if cg_potential:
            raise NotImplementedError("VerletListDynamicResolution*(cg_potential=True): the coarse-grained weight 1 - lambda_i lambda_j is outside the hot-path scope")
        _VerletListInteraction.__init__(self, vl)
        self.max_force = -1.0

    def _send(self, type1, type2, potential):
        raise NotImplementedError

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential
        self._send(type1, type2, potential)
        self.system.engine.nb_resolution(type1, type2, True, max(float(self.max_force), 0.0))

    def setMaxForce(self, max_force):
        self.max_force = float(max_force)
        for t1, t2 in self._pots:
            self.system.engine.nb_resolution(t1, t2, True, max(self.max_force, 0.0))


class _VerletListDynamicResolutionLennardJones(_VerletListDynamicResolution):
    label = "lj_dynres"

    def _send(self, type1, type2, potential):
        self.system.engine.nb_lj(type1, type2, potential.epsilon, potential.sigma, potential.cutoff, potential.shift == "auto")


class _VerletListDynamicResolutionTabulated(_VerletListDynamicResolution):
    label = "tab_dynres"

    def _send(self, type1, type2, potential):
        self.system.engine.nb_table(type1, type2, potential.r0, potential.dr, potential.e, potential.f, potential.cutoff, **_interp_kw(potential))


class _LennardJonesCapped(_LennardJones):
    """interaction.LennardJonesCapped(epsilon, sigma, cutoff, caprad, shift): LJ evaluated at r = caprad inside caprad
    (rule set: include/chem_mi355.h, chem_nb_cap)."""

    def __init__(self, epsilon=1.0, sigma=1.0, cutoff=2.5, caprad=0.0, shift="auto"):
        _LennardJones.__init__(self, epsilon, sigma, cutoff, shift)
        self.caprad = caprad


class _TabulatedCapped(_Tabulated):
    """interaction.TabulatedCapped(itype, filename, cutoff, caprad) (gromacs_topology.py:684-695, nonbond_params func 13):
    the table evaluated at r = caprad inside caprad (rule set: include/chem_mi355.h, chem_nb_cap)."""

    def __init__(self, itype=1, filename=None, cutoff=None, caprad=0.0):
        _Tabulated.__init__(self, itype, filename, cutoff)
        self.caprad = caprad


class _VerletListCapped(_VerletListInteraction):
    """interaction.VerletListLennardJonesCapped / VerletListTabulatedCapped(vl): the potential is sent as for the uncapped
    interaction, then its cap radius.  The energy is the engine's LJ / tabulated accumulator, shared with the uncapped pairs."""
    energy_key = None

    def _send(self, type1, type2, potential):
        raise NotImplementedError

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential
        self._send(type1, type2, potential)
        self.system.engine.nb_cap(type1, type2, float(potential.caprad))

    def computeEnergy(self):
        return self.system.engine.observe()[self.energy_key]


class _VerletListLennardJonesCapped(_VerletListCapped):
    label = "lj_cap"
    energy_key = "epot_lj"

    def _send(self, type1, type2, potential):
        self.system.engine.nb_lj(type1, type2, potential.epsilon, potential.sigma, potential.cutoff, potential.shift == "auto")


class _VerletListTabulatedCapped(_VerletListCapped):
    label = "tab_cap"
    energy_key = "epot_tab"

    def _send(self, type1, type2, potential):
        self.system.engine.nb_table(type1, type2, potential.r0, potential.dr, potential.e, potential.f, potential.cutoff, **_interp_kw(potential))


class _CoulombTruncated(_Pot):
    """interaction.CoulombTruncated(prefactor, cutoff): U = prefactor q_i q_j / r inside the cutoff, unshifted
    (rule set: include/chem_mi355.h, chem_nb_coulomb)."""

    def __init__(self, prefactor=1.0, cutoff=None):
        self.prefactor, self.cutoff = prefactor, cutoff


class _VerletListCoulombTruncated(_VerletListInteraction):
    """interaction.VerletListCoulombTruncated(vl).setPotential(type1, type2, CoulombTruncated(...)) (gromacs_topology.py:866-878)."""
    label = "coulomb"

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential
        self.system.engine.nb_coulomb(type1, type2, potential.prefactor, potential.cutoff)


class _VerletListMixedTabulated(_VerletListInteraction):
    """interaction.VerletListMixedTabulated(vl).setPotential(type1, type2, MixedTabulated(...)) (gromacs_topology.py:756-790)."""
    label = "mix_tab"

    def setPotential(self, type1, type2, potential):
        self._pots[(min(type1, type2), max(type1, type2))] = potential

        def push(x, t1=type1, t2=type2, pot=potential):
            x = min(max(float(x), 0.0), 1.0)
            if getattr(pot, "_sent", {}).get((t1, t2)) == x:
                return
            e, f = pot.rows(x)
            self.system.engine.nb_table(t1, t2, pot.r0, pot.dr, e, f, pot.cutoff)
            pot.__dict__.setdefault("_sent", {})[(t1, t2)] = x
            pot.mix_value = x
        if potential.observable is not None:
            potential.observable.connect(push)
            push(potential.observable.compute() if self.system.engine.n else 0.0)
        else:
            push(potential.mix_value)


class _FixedListInteraction(object):
    by_types = False

    def _kp(self, pot):
        """(kind, parameter list) of a potential object; a Tabulated bond potential (func 8,
        gromacs_topology.py:919-925) registers its rows once per engine and passes the table handle."""
        if isinstance(pot, _Tabulated):
            kind = "ANG_TABULATED" if isinstance(pot, _TabulatedAngular) else ("DIH_TABULATED" if isinstance(pot, _TabulatedDihedral) else "TABULATED")
            eng = self.system.engine
            cache = pot.__dict__.setdefault("_handles", {})
            if id(eng) not in cache:
                cache[id(eng)] = eng.table_create(pot.r0, pot.dr, pot.e, pot.f, **_interp_kw(pot))
            return kind, [float(cache[id(eng)])]
        if isinstance(pot, _LennardJones):      # FixedPairList[Types]LennardJones: 1-4 pairs
            return "LJ_BOND", [pot.epsilon, pot.sigma, pot.cutoff if pot.cutoff is not None else 1e30]
        if isinstance(pot, _CoulombTruncated):  # FixedPairList[Types]CoulombTruncated: 1-4 pairs (CHEM_POT_COULOMB_BOND)
            return "COULOMB_BOND", [pot.prefactor, pot.cutoff]
        return pot.kind, pot.params()

    def __init__(self, system, flist, potential=None):
        self.system, self.flist = system, flist
        self.potential = potential
        self._typed = {}
        self.handle = None      # the library list of THIS interaction's kind (the list object may carry several)
        if potential is not None:
            kind, par = self._kp(potential)
            h = self.handle = flist._bind(kind, False)
            system.engine.list_set_params(h, par)

    def setPotential(self, *args, **kw):
        # (the reference also spells the arguments out: setPotential(type1=.., type2=.., potential=..), gromacs_topology.py:1408)
        args = args + tuple(kw[k] for k in ("type1", "type2", "type3", "type4", "potential") if k in kw)
        pot = args[-1]
        types = tuple(int(t) for t in args[:-1])
        kind, par = self._kp(pot)
        if not self.by_types:
            self.potential = pot
            h = self.handle = self.flist._bind(kind, False)
            self.system.engine.list_set_params(h, par)
            return
        h = self.handle = self.flist._bind(kind, True)
        self._typed[types] = pot
        self.system.engine.list_set_params(h, par, types=types)

    def getFixedPairList(self):
        return self.flist

    getFixedTripleList = getFixedQuadrupleList = getFixedPairList


class _FixedListTypesInteraction(_FixedListInteraction):
    by_types = True

    def __init__(self, system, flist):
        self.system, self.flist = system, flist
        self.potential = None
        self._typed = {}
        self.handle = None


class _FixedListLambdaInteraction(_FixedListInteraction):
    """interaction.FixedPairListLambda<Potential>(system, fpl, potential): the potential's force and energy times the lambda of
    each bond of a FixedPairListLambda."""

    def __init__(self, system, flist, potential=None):
        if not isinstance(flist, FixedPairListLambda):
            raise TypeError("interaction.FixedPairListLambda*: the list must be an espressopp.FixedPairListLambda")
        _FixedListInteraction.__init__(self, system, flist, potential)


def _lambda_tuple_interaction(base, list_cls, name):
    """interaction.Fixed{Triple,Quadruple}List[Types]Lambda<Potential>: the plain interaction of that shape, on a list of the
    Lambda kind only (as _FixedListLambdaInteraction)."""
    class _Inter(base):
        def __init__(self, system, flist, *potential):
            if not isinstance(flist, list_cls):
                raise TypeError("interaction.%s*: the list must be an espressopp.%s" % (name, list_cls.__name__))
            base.__init__(self, system, flist, *potential)
    _Inter.__name__ = "_" + name + "Interaction"
    return _Inter


_FixedTripleListLambdaInteraction = _lambda_tuple_interaction(_FixedListInteraction, FixedTripleListLambda, "FixedTripleListLambda")
_FixedTripleListTypesLambdaInteraction = _lambda_tuple_interaction(_FixedListTypesInteraction, FixedTripleListLambda, "FixedTripleListTypesLambda")
_FixedQuadrupleListLambdaInteraction = _lambda_tuple_interaction(_FixedListInteraction, FixedQuadrupleListLambda, "FixedQuadrupleListLambda")
_FixedQuadrupleListTypesLambdaInteraction = _lambda_tuple_interaction(_FixedListTypesInteraction, FixedQuadrupleListLambda, "FixedQuadrupleListTypesLambda")


def _ns(**kw):
    return types.SimpleNamespace(**kw)


interaction = _ns(
    LennardJones=_LennardJones, Tabulated=_Tabulated, Harmonic=_Harmonic, FENE=_FENE,
    AngularHarmonic=_AngularHarmonic, Cosine=_Cosine, DihedralHarmonicNCos=_DihedralHarmonicNCos, DihedralRB=_DihedralRB,
    VerletListLennardJones=_VerletListLennardJones, VerletListTabulated=_VerletListTabulated,
    FixedPairListHarmonic=_FixedListInteraction, FixedPairListFENE=_FixedListInteraction,
    FixedPairListTypesHarmonic=_FixedListTypesInteraction, FixedPairListTypesFENE=_FixedListTypesInteraction,
    FixedTripleListAngularHarmonic=_FixedListInteraction, FixedTripleListCosine=_FixedListInteraction,
    FixedTripleListTypesAngularHarmonic=_FixedListTypesInteraction, FixedTripleListTypesCosine=_FixedListTypesInteraction,
    FixedQuadrupleListDihedralHarmonicNCos=_FixedListInteraction, FixedQuadrupleListDihedralRB=_FixedListInteraction,
    FixedQuadrupleListTypesDihedralHarmonicNCos=_FixedListTypesInteraction, FixedQuadrupleListTypesDihedralRB=_FixedListTypesInteraction,
    FENELennardJones=_FENELennardJones, DihedralHarmonic=_DihedralHarmonic,
    FixedPairListFENELennardJones=_FixedListInteraction, FixedPairListTypesFENELennardJones=_FixedListTypesInteraction,
    FixedPairListLennardJones=_FixedListInteraction, FixedPairListTypesLennardJones=_FixedListTypesInteraction,
    FixedQuadrupleListDihedralHarmonic=_FixedListInteraction, FixedQuadrupleListTypesDihedralHarmonic=_FixedListTypesInteraction,
    CoulombTruncated=_CoulombTruncated, VerletListCoulombTruncated=_VerletListCoulombTruncated,
    FixedPairListCoulombTruncated=_FixedListInteraction, FixedPairListTypesCoulombTruncated=_FixedListTypesInteraction,
    TabulatedAngular=_TabulatedAngular, TabulatedDihedral=_TabulatedDihedral,
    FixedQuadrupleListTabulatedDihedral=_FixedListInteraction, FixedQuadrupleListTypesTabulatedDihedral=_FixedListTypesInteraction,
    FixedPairListTabulated=_FixedListInteraction, FixedPairListTypesTabulated=_FixedListTypesInteraction,
    FixedTripleListTabulatedAngular=_FixedListInteraction, FixedTripleListTypesTabulatedAngular=_FixedListTypesInteraction,
    FixedPairListLambdaHarmonic=_FixedListLambdaInteraction, FixedPairListLambdaFENE=_FixedListLambdaInteraction,
    FixedPairListLambdaFENELennardJones=_FixedListLambdaInteraction, FixedPairListLambdaTabulated=_FixedListLambdaInteraction,
    # hybrid angles and dihedrals: one class per angle / dihedral potential, plain and by types
    **{"FixedTripleList%sLambda%s" % (ty, pot): (_FixedTripleListTypesLambdaInteraction if ty else _FixedTripleListLambdaInteraction)
       for ty in ("", "Types") for pot in ("AngularHarmonic", "Cosine", "TabulatedAngular")},
    **{"FixedQuadrupleList%sLambda%s" % (ty, pot): (_FixedQuadrupleListTypesLambdaInteraction if ty else _FixedQuadrupleListLambdaInteraction)
       for ty in ("", "Types") for pot in ("DihedralHarmonicNCos", "DihedralRB", "DihedralHarmonic", "TabulatedDihedral")},
    VerletListDynamicResolutionLennardJones=_VerletListDynamicResolutionLennardJones,
    VerletListDynamicResolutionTabulated=_VerletListDynamicResolutionTabulated,
    MixedTabulated=_MixedTabulated, VerletListMixedTabulated=_VerletListMixedTabulated, MultiTabulated=_unsupported("interaction.MultiTabulated"),
    LennardJonesCapped=_LennardJonesCapped, VerletListLennardJonesCapped=_VerletListLennardJonesCapped,
    TabulatedCapped=_TabulatedCapped, VerletListTabulatedCapped=_VerletListTabulatedCapped,
    # (nonbond_params func 16: what the force does inside the cap of the energy-capped variant is not pinned down, and no example uses it)
    LennardJonesEnergyCapped=_unsupported("interaction.LennardJonesEnergyCapped"),
    VerletListLennardJonesEnergyCapped=_unsupported("interaction.VerletListLennardJonesEnergyCapped"),
)


# ---- integrator + extensions -------------------------------------------------------------------
class _VelocityVerlet(object):
    """integrator.VelocityVerlet(system): .dt .step run(n) addExtension getTimers
    (start_simulation.py:165-167,780)."""

    def __init__(self, system):
        self.system = system
        system.integrator = self
        self._dt = None
        self._ext = []

    @property
    def dt(self):
        return self._dt

    @dt.setter
    def dt(self, value):
        self._dt = float(value)
        self.system.engine.set_dt(value)

    @property
    def step(self):
        return self.system.engine.step

    def addExtension(self, ext):
        self._ext.append(ext)
        if hasattr(ext, "_connect"):
            ext._connect(self)

    def getNumberOfExtensions(self):
        return len(self._ext)

    def getExtension(self, k):
        return self._ext[k]

    def run(self, nsteps):
        # ExtAnalyze observers fire every `interval` steps (aftIntV): split the call at those boundaries
        e = self.system.engine
        if self.system.storage is not None:
            self.system.storage.decompose()
        ana = [x for x in self._ext if isinstance(x, _ExtAnalyze)]
        done = 0
        while done < nsteps:
            chunk = nsteps - done
            for a in ana:
                chunk = min(chunk, a.interval - (e.step % a.interval))
            e.run(chunk)
            done += chunk
            for a in ana:
                if e.step % a.interval == 0:
                    a.perform()
        if nsteps == 0:
            e.run(0)

    def getTimers(self):
        t = self.system.engine.timers()
        return [("Run", t["run_wall_s"]), ("Reaction", t["reaction_wall_s"]), ("Resort", t["rebuild_wall_s"])]


class _LangevinThermostat(object):
    """integrator.LangevinThermostat(system): .temperature (= T*kb), .gamma (start_simulation.py:330-336)."""

    def __init__(self, system):
        self.system = system
        self.temperature = 0.0
        self.gamma = 0.0
        self.valid_types = None

    def add_valid_types(self, types_):
        """Thermal groups (start_simulation.py:312-336): only particles whose current type is listed are thermalised;
        an empty list (no --thermal_groups / --table_groups) leaves every type thermalised."""
        self.valid_types = sorted(set(int(t) for t in types_ if t is not None))
        if getattr(self, "_connected", False):
            self.system.engine.thermostat_langevin_types(self.valid_types)

    def _connect(self, integrator):
        seed = self.system.rng.get_seed() if self.system.rng is not None else 0
        self.system.engine.thermostat_langevin(self.temperature, self.gamma, seed)
        self.system.engine.thermostat_langevin_types(self.valid_types or [])
        self._connected = True


class _BerendsenThermostat(object):
    """integrator.BerendsenThermostat(system): .temperature (= T*kb), .tau (start_simulation.py:341-344)."""

    def __init__(self, system):
        self.system, self.temperature, self.tau = system, 0.0, 1.0

    def _connect(self, integrator):
        self.system.engine.thermostat_rescale("berendsen", self.temperature, self.tau)

    def disconnect(self):
        self.system.engine.thermostat_rescale(None, 1.0, 1.0)


class _BerendsenBarostat(object):
    """integrator.BerendsenBarostat(system, pressure): .tau, .pressure (start_simulation.py:356-376): isotropic, on every step
    (include/chem_mi355.h chem_barostat_berendsen).  Attributes set after addExtension reach the engine at once."""

    def __init__(self, system, pressure=1.0):
        # (the driver hands the analysis.Pressure observable here and sets the target through .pressure afterwards)
        p0 = float(pressure) if isinstance(pressure, (int, float)) else 1.0
        self.__dict__.update(system=system, _pressure=p0, _tau=1.0, _connected=False)

    def _push(self):
        if self._connected:
            self.system.engine.barostat_berendsen(self._pressure, self._tau)

    pressure = property(lambda self: self._pressure)
    tau = property(lambda self: self._tau)

    @pressure.setter
    def pressure(self, v):
        self.__dict__["_pressure"] = float(v)
        self._push()

    @tau.setter
    def tau(self, v):
        self.__dict__["_tau"] = float(v)
        self._push()

    def _connect(self, integrator):
        self.__dict__["_connected"] = True
        self._push()

    def disconnect(self):
        self.__dict__["_connected"] = False
        self.system.engine.barostat_berendsen(0.0, 0.0)


class _LangevinBarostat(object):
    """integrator.LangevinBarostat(system, rng, temperature): .gammaP, .mass, .pressure (start_simulation.py:361-367): the
    Langevin piston of include/chem_mi355.h chem_barostat_langevin.  `temperature` is kT (the driver passes T * kb); the seed of
    the piston's noise is the rng's.  Attributes set after addExtension reach the engine at once."""

    def __init__(self, system, rng, temperature):
        if system is None or rng is None:
            raise NotImplementedError("integrator.LangevinBarostat needs a system and its rng")
        self.__dict__.update(system=system, rng=rng, temperature=float(temperature), _pressure=1.0, _mass=0.0, _gammaP=0.0, _connected=False)

    def _push(self):
        if self._connected:
            self.system.engine.barostat_langevin(self._pressure, self._mass, self._gammaP, self.temperature, self.rng.get_seed())

    pressure = property(lambda self: self._pressure)
    mass = property(lambda self: self._mass)
    gammaP = property(lambda self: self._gammaP)

    @pressure.setter
    def pressure(self, v):
        self.__dict__["_pressure"] = float(v)
        self._push()

    @mass.setter
    def mass(self, v):
        self.__dict__["_mass"] = float(v)
        self._push()

    @gammaP.setter
    def gammaP(self, v):
        self.__dict__["_gammaP"] = float(v)
        self._push()

    def _connect(self, integrator):
        self.__dict__["_connected"] = True
        self._push()

    def disconnect(self):
        self.__dict__["_connected"] = False
        self.system.engine.barostat_langevin(0.0, 0.0, 0.0, 0.0, 0)


class _Isokinetic(object):
    """integrator.Isokinetic(system): .temperature, .coupling = rescale every `coupling` steps (start_simulation.py:345-348)."""

    def __init__(self, system):
        self.system, self.temperature, self.coupling = system, 0.0, 1

    def _connect(self, integrator):
        self.system.engine.thermostat_rescale("isokinetic", self.temperature, int(self.coupling))

    def disconnect(self):
        self.system.engine.thermostat_rescale(None, 1.0, 1.0)


class _StochasticVelocityRescaling(object):
    """integrator.StochasticVelocityRescaling(system): .temperature (= T*kb), .coupling (start_simulation.py:337-340)."""

    def __init__(self, system):
        self.system, self.temperature, self.coupling = system, 0.0, 1.0

    def _connect(self, integrator):
        seed = self.system.rng.get_seed() if self.system.rng is not None else 0
        self.system.engine.thermostat_svr(self.temperature, self.coupling, seed)

    def disconnect(self):
        self.system.engine.thermostat_svr(1.0, 0.0, 0)


class _CapForce(object):
    """integrator.CapForce(system, max_force) (start_simulation.py:320-324): conservative force of a particle
    rescaled to |f| = max_force where it exceeds it, before the thermostat's terms."""

    def __init__(self, system, capForce, particleGroup=None):
        if particleGroup is not None:
            raise NotImplementedError("CapForce on a particle group is outside the hot-path scope")
        if not isinstance(capForce, (int, float)):
            raise NotImplementedError("CapForce with a Real3D cap is outside the hot-path scope (ChemLab passes a scalar)")
        self.system = system
        self.capForce = float(capForce)

    def _connect(self, integrator):
        self.system.engine.cap_force(self.capForce)

    def disconnect(self):
        self.system.engine.cap_force(0.0)


class _TopologyParticleProperties(object):
    """integrator.TopologyParticleProperties(type=, mass=, q=, state=, incr_state=) + set_min_max_state(min, max)
    (reaction_setup.py:245-249: the neighbour changes only while its state is in [min, max), and its state is incremented)."""

    def __init__(self, type=None, mass=None, q=None, state=None, incr_state=None, lambda_adr=None, **kw):
        self.type, self.mass, self.q, self.state, self.incr_state = type, mass, q, state, incr_state
        self.lambda_adr = lambda_adr        # honoured on the reactants of a Reaction / DissociationReaction (chem_reaction_set_resolution)
        self.min_state = self.max_state = None

    def set_min_max_state(self, min_state, max_state):
        self.min_state, self.max_state = int(min_state), int(max_state)


class _ReactionConstraintNeighbourState(object):
    """integrator.ReactionConstraintNeighbourState(type_id, min_state, max_state): the constrained reactant must have a
    bonded neighbour of that type in that state window (reaction_setup.py:203-204)."""

    def __init__(self, type_id, min_state, max_state):
        self.type_id, self.min_state, self.max_state = int(type_id), int(min_state), int(max_state)


class _ATRPActivator(object):
    """integrator.ATRPActivator(system, interval, num_particles, ratio_activator, ratio_deactivator, delta_catalyst,
    k_activate, k_deactivate): .stats_filename, .select_from_all, add_reactive_center(type_id, state, is_activator,
    new_property, delta_state) (reaction_post_process.py:380-426).  Bound to chem_atrp_* when added to the integrator."""

    def __init__(self, system, interval, num_particles, ratio_activator, ratio_deactivator, delta_catalyst, k_activate, k_deactivate):
        self.system = system
        self.interval, self.num_particles = int(interval), int(num_particles)
        self.ratio_activator, self.ratio_deactivator = float(ratio_activator), float(ratio_deactivator)
        self.delta_catalyst, self.k_activate, self.k_deactivate = float(delta_catalyst), float(k_activate), float(k_deactivate)
        self.stats_filename = None
        self.select_from_all = 1
        self._centers = []
        self._connected = False

    def add_reactive_center(self, type_id, state, is_activator, new_property, delta_state):
        c = (int(type_id), int(state), bool(is_activator), int(new_property.type), float(new_property.mass), float(new_property.q or 0.0), int(delta_state))
        self._centers.append(c)
        if self._connected:
            self.system.engine.atrp_add_center(*c)

    def _connect(self, integrator):
        e = self.system.engine
        seed = self.system.rng.get_seed() if self.system.rng is not None else 0
        if not self._connected:
            for c in self._centers:
                e.atrp_add_center(*c)
        e.atrp_init(self.interval, self.num_particles, self.ratio_activator, self.ratio_deactivator, self.delta_catalyst,
                    self.k_activate, self.k_deactivate, select_from_all=bool(int(self.select_from_all)), seed=seed)
        self._connected = True

    def disconnect(self):
        self.system.engine.atrp_disconnect()

    def save_stats(self, filename=None):
        """One row per firing: step, activator and deactivator fractions, flips (the reference's `stats_file`)."""
        filename = filename or self.stats_filename
        rows = self.system.engine.atrp_stats()
        if filename:
            with _rank.wopen(filename, "w") as f:
                f.write("# step ratio_activator ratio_deactivator activated deactivated candidates selected\n")
                for r in rows:
                    f.write("%d %.10g %.10g %d %d %d %d\n" % (r["step"], r["ratio_activator"], r["ratio_deactivator"], r["activated"],
                                                              r["deactivated"], r["candidates"], r["selected"]))
        return rows


class _PostProcessChangeNeighboursProperty(object):
    """integrator.PostProcessChangeNeighboursProperty(topology_manager).add_change_property(old_type, props, nb_level)
    (reaction_post_process.py:76-115): attached to a reaction with add_postprocess(pp, 'type_1' | 'type_2' | 'both')."""

    def __init__(self, topology_manager=None):
        self.rules = []     # (old_type, TopologyParticleProperties, nb_level) in insertion order

    def add_change_property(self, type_id, prop, nb_level):
        self.rules.append((int(type_id), prop, int(nb_level)))


class _PostProcessChangeProperty(object):
    """integrator.PostProcessChangeProperty() and PostProcessChangePropertyByTopologyManager(tm) (reaction_setup.py:225-236):
    both change type / mass / charge of the reactant itself; here they are the same thing (new_type_* of chem_reaction_desc)."""

    def __init__(self, *args):
        """() | (topology_manager) : the reaction's form, changes added with add_change_property;
        (type_id, TopologyParticleProperties): BasicDynamicResolution's form (reaction_setup.py:332-333), one change given at once"""
        self.changes = {}
        if len(args) == 2 and isinstance(args[1], _TopologyParticleProperties):
            type_id, prop = args
            self.add_change_property(type_id, prop)
        elif len(args) > 1:
            raise TypeError("PostProcessChangeProperty([topology_manager]) or PostProcessChangeProperty(type_id, TopologyParticleProperties)")

    def add_change_property(self, type_id, prop):
        self.changes[int(type_id)] = prop


class _ReactionCutoff(object):
    def __init__(self, cutoff):
        self.cutoff = cutoff
        self.min_cutoff = 0.0


class _Reaction(object):
    """integrator.Reaction(type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2,
    max_state_2, rate, fpl, cutoff) (reaction_setup.py:81-92)."""

    def __init__(self, type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2, max_state_2, rate, fpl, cutoff):
        self.__dict__.update(type_1=type_1, type_2=type_2, delta_1=delta_1, delta_2=delta_2, min_state_1=min_state_1,
                             max_state_1=max_state_1, min_state_2=min_state_2, max_state_2=max_state_2, rate=rate, fpl=fpl)
        self._cut = _ReactionCutoff(cutoff)
        self.intramolecular = False
        self.intraresidual = False
        self.is_virtual = False
        self.active = True
        self._pp = {}
        self._nb_pp = []
        self._release = []
        self._remove = []
        self._join = []
        self._constraints = []
        self._index = None
        self._system = None

    def add_constraint(self, constraint, which="type_1"):
        if not isinstance(constraint, _ReactionConstraintNeighbourState):
            raise NotImplementedError("reaction constraint %s is outside the hot-path scope" % type(constraint).__name__)
        self._constraints.append((constraint, which))

    @property
    def cutoff(self):
        return self._cut.cutoff

    def get_reaction_cutoff(self):
        return self._cut

    def set_reaction_cutoff(self, rc):
        raise NotImplementedError("ReactionCutoffRandom is outside the hot-path scope")

    def add_postprocess(self, pp, which="type_1"):
        if isinstance(pp, _PostProcessChangeNeighboursProperty):
            self._nb_pp.append((pp, which))
            return
        if isinstance(pp, _PostProcessReleaseParticles):
            self._release.append((pp, which))
            return
        if isinstance(pp, _PostProcessRemoveNeighbourBond):
            self._remove.append((pp, which))
            return
        if isinstance(pp, _PostProcessJoinParticles):
            self._join.append((pp, which))
            return
        if not isinstance(pp, _PostProcessChangeProperty):
            raise NotImplementedError("post-process %s is outside the hot-path scope" % type(pp).__name__)
        self._pp[which] = pp

    def __setattr__(self, k, v):
        object.__setattr__(self, k, v)
        if k == "rate" and getattr(self, "_index", None) is not None:
            self._system.engine.reaction_set_rate(self._index, v)


class _RestrictReaction(_Reaction):
    """integrator.RestrictReaction(...): a Reaction that only accepts the id pairs given by define_connection(b1, b2)
    (group option `connectivity_map`, reaction_setup.py:75-78,115-128)."""

    def __init__(self, *a, **kw):
        _Reaction.__init__(self, *a, **kw)
        object.__setattr__(self, "_connections", [])
        object.__setattr__(self, "revert", False)

    def define_connection(self, b1, b2):
        self._connections.append((int(b1), int(b2)))
        if self._index is not None:
            self._system.engine.reaction_restrict(self._index, [(int(b1), int(b2))])


class _DissociationReaction(_Reaction):
    """integrator.DissociationReaction(type_1, type_2, delta_1, delta_2, min_state_1, max_state_1, min_state_2, max_state_2,
    rate, fpl, cutoff) + .diss_rate (reaction_setup.py:257-356): breaks bonds of `fpl` that are longer than `cutoff` or,
    with probability diss_rate * dt * interval, any of them (chem_dissociation_add; rule set in include/chem_mi355.h).
    `unexclude` (this shim's own attribute, default True): a broken pair interacts through the pair potential again.
    A PostProcessChangeProperty with a type acts at once; one with TopologyParticleProperties(lambda_adr=...) alone sets the
    reactant's resolution, and BasicDynamicResolution then carries the delayed type change (reaction_setup.py:319-354)."""

    def __init__(self, *a, **kw):
        _Reaction.__init__(self, *a, **kw)
        object.__setattr__(self, "diss_rate", 0.0)
        object.__setattr__(self, "unexclude", True)

    def add_postprocess(self, pp, which="type_1"):
        if not isinstance(pp, _PostProcessChangeProperty):
            raise NotImplementedError("post-process %s of a DissociationReaction is outside the hot-path scope" % type(pp).__name__)
        self._pp[which] = pp

    def __setattr__(self, k, v):
        object.__setattr__(self, k, v)
        if k == "diss_rate" and getattr(self, "_index", None) is not None:
            self._system.engine.reaction_set_rate(self._index, v)


class _ChemicalReaction(object):
    """integrator.ChemicalReaction(system, vl, storage, topology_manager, interval): nearest_mode,
    max_per_interval, add_reaction, disconnect (reaction_setup.py:416-427,506)."""

    def __init__(self, system, vl, storage, topology_manager, interval):
        self.system, self.interval = system, int(interval)
        self.nearest_mode = False
        self.max_per_interval = -1
        self._reactions = []
        self._initialised = False

    def add_reaction(self, r):
        self._reactions.append(r)

    def _flush(self):
        e = self.system.engine
        if not self._initialised:
            seed = self.system.rng.get_seed() if self.system.rng is not None else 0
            e.reaction_init(self.interval, bool(self.nearest_mode), max(int(self.max_per_interval), 0), seed)
            self._initialised = True
        for r in self._reactions:
            if r._index is not None:
                continue
            kw = {}
            for which, k in (("type_1", 1), ("type_2", 2)):
                pp = r._pp.get(which)
                old = getattr(r, which)
                if pp is not None and old in pp.changes and pp.changes[old].type is not None:
                    ch = pp.changes[old]
                    kw["new_type_%d" % k] = int(ch.type)
                    kw["new_mass_%d" % k] = float(ch.mass)
                    kw["new_q_%d" % k] = float(ch.q or 0.0)
            if isinstance(r, _DissociationReaction):
                if r._constraints or r.fpl is None or r.fpl.handle is None:
                    raise RuntimeError("DissociationReaction: needs a FixedPairList with an interaction attached and takes no constraints")
                r._index = e.dissociation_add(r.type_1, r.type_2, r.delta_1, r.delta_2, r.min_state_1, r.max_state_1, r.min_state_2,
                                              r.max_state_2, r.diss_rate, r.cutoff, r.fpl.handle, unexclude=r.unexclude, active=r.active, **kw)
                r._system = self.system
                self._lambda_rules(r)
                continue
            bond_list = -1
            if not r.is_virtual:
                if r.fpl.handle is None:
                    raise RuntimeError("Reaction: the FixedPairList has no interaction (potential) attached")
                bond_list = r.fpl.handle
            r._index = e.reaction_add(r.type_1, r.type_2, r.delta_1, r.delta_2, r.min_state_1, r.max_state_1, r.min_state_2,
                                      r.max_state_2, r.rate, r.cutoff, bond_list=bond_list, min_cutoff=r._cut.min_cutoff,
                                      intramolecular=r.intramolecular, intraresidual=r.intraresidual, is_virtual=r.is_virtual,
                                      active=r.active, **kw)
            r._system = self.system
            self._lambda_rules(r)
            if isinstance(r, _RestrictReaction):
                if r.revert:
                    raise NotImplementedError("RestrictReaction.revert (dissociation along a connectivity map) is outside the hot-path scope")
                e.reaction_restrict(r._index, r._connections)
            for rel, which in r._release:         # PostProcessReleaseParticles(fd, count): the FixDistances extension is connected first
                if rel.fd.handle is None:
                    raise RuntimeError("PostProcessReleaseParticles: add its FixDistances to the integrator before the reactions")
                e.reaction_release(r._index, which, rel.fd.handle, rel.count)
            for cons, which in r._constraints:
                e.reaction_constraint(r._index, which, cons.type_id, cons.min_state, cons.max_state)
            for pp, which in r._nb_pp:
                for old_type, prop, nb_level in pp.rules:
                    window = None if getattr(prop, "min_state", None) is None else (prop.min_state, prop.max_state)
                    e.reaction_neighbour_change(r._index, which, old_type, nb_level, int(prop.type), float(prop.mass),
                                                float(prop.q or 0.0), None if prop.state is None else int(prop.state),
                                                incr_state=getattr(prop, "incr_state", None), state_window=window)
            # the reverse direction (chem_reaction_remove_bond, chem_reaction_join): behind the neighbour changes, as the engine orders them
            for pp, which in r._remove:
                for anchor_type, nb_level, t1, t2 in pp.rules:
                    e.reaction_remove_bond(r._index, which, anchor_type, nb_level, t1, t2, pp.unexclude)
            for pp, which in r._join:
                if pp.fd.handle is None:
                    raise RuntimeError("PostProcessJoinParticles: add its FixDistances to the integrator before the reactions")
                for role in {"type_1": ("type_1",), "type_2": ("type_2",), "both": ("type_1", "type_2")}[which]:
                    e.reaction_join(r._index, role, pp.fd.handle, pp.eq_length)

    def _lambda_rules(self, r):
        """TopologyParticleProperties(lambda_adr=...) of the reaction's PostProcessChangeProperty: the reactant's resolution"""
        for which, k in (("type_1", 1), ("type_2", 2)):
            pp = r._pp.get(which)
            ch = pp.changes.get(getattr(r, which)) if pp is not None else None
            if ch is not None and getattr(ch, "lambda_adr", None) is not None:
                self.system.engine.reaction_set_resolution(r._index, k, float(ch.lambda_adr))

    def _connect(self, integrator):
        self._flush()
        self.system.engine.reactions_enable(True)

    def disconnect(self):
        self.system.engine.reactions_enable(False)

    def connect(self):
        self.system.engine.reactions_enable(True)

    def get_timers(self):
        return []

    def save_reaction_counters(self, filename):
        """events per reaction index (start_simulation.py:1028)"""
        ev = self.system.engine.get_events()
        with _rank.wopen(filename, "w") as f:
            for r in range(len(self._reactions)):
                f.write("%d %d\n" % (r, int((ev["reaction"] == r).sum())))

    def save_intra_inter_counter(self, filename):
        """events between particles of the same / of different bonded clusters at the time of the event, per reaction
        (start_simulation.py:1034); needs engine option count_intra_inter (the driver sets it)."""
        ev = self.system.engine.get_events()
        with _rank.wopen(filename, "w") as f:
            f.write("# reaction intra inter\n")
            for r in range(len(self._reactions)):
                m = ev["reaction"] == r
                f.write("%d %d %d\n" % (r, int((ev["pad"][m] == 1).sum()), int((ev["pad"][m] == 0).sum())))


class _TopologyManager(object):
    """integrator.TopologyManager(system): observe_tuple, register_tuple/triplet/quadruplet,
    initialize_topology (start_simulation.py:211-212,395-440).  The bond graph itself lives in the
    library (chem_host.hpp); this object only forwards the registrations."""

    def __init__(self, system):
        self.system = system
        self._fpls = []

    def observe_tuple(self, fpl):
        if getattr(fpl, "arity", 2) == 2 and fpl not in self._fpls:
            self._fpls.append(fpl)

    def observe_triple(self, ftl):
        pass

    observe_quadruple = observe_triple

    # end-of-run dumps (start_simulation.py:1004-1006); layout: chemlab/outputs.py write_topology_dumps
    def _dump(self, filename, suffix):
        from ..chemlab import outputs
        import os, shutil, tempfile
        tmp = tempfile.mkdtemp()
        try:
            outputs.write_topology_dumps(os.path.join(tmp, "x"), self.system, self._fpls)
            if not _rank.is_root():      # (the dump above gathers collectively: every rank makes it, rank 0 keeps the file)
                return
            d = os.path.dirname(filename)
            if d and not os.path.isdir(d):
                os.makedirs(d)
            shutil.move(os.path.join(tmp, "x" + suffix), filename)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    def save_topology(self, filename):
        self._dump(filename, "_topology.dat")

    def save_res_topology(self, filename):
        self._dump(filename, "_res_topology.dat")

    def save_residues(self, filename):
        self._dump(filename, "_residue_list.dat")

    def register_tuple(self, fpl, t1, t2):
        pass   # bonds never spawn from other bonds

    def register_triplet(self, ftl, t1, t2, t3):
        if ftl.handle is None:
            raise RuntimeError("register_triplet: the FixedTripleList has no interaction attached")
        self.system.engine.topology_register(ftl.handle, [t1, t2, t3])

    def register_quadruplet(self, fql, t1, t2, t3, t4):
        if fql.handle is None:
            raise RuntimeError("register_quadruplet: the FixedQuadrupleList has no interaction attached")
        self.system.engine.topology_register(fql.handle, [t1, t2, t3, t4])

    def initialize_topology(self):
        pass

    def _connect(self, integrator):
        pass

    def get_timers(self):
        return []


class _ExtAnalyze(object):
    def __init__(self, obj, interval):
        self.obj, self.interval = obj, max(1, int(interval))

    def perform(self):
        if hasattr(self.obj, "perform_action"):
            self.obj.perform_action()
        elif hasattr(self.obj, "perform"):
            self.obj.perform()

    def _connect(self, integrator):
        pass


class _FixedListDynamicResolution(object):
    """integrator.FixedListDynamicResolution(system) + register_pair_list(fpl, rate) (start_simulation.py:289-293), and
    register_triple_list(ftl, rate) / register_quadruple_list(fql, rate): every entry of the list gains `rate` of lambda per
    MD step up to 1.  Nothing runs per step here: the engine evaluates lambda from the step counter and the entry's birth step."""

    def __init__(self, system):
        self.system = system
        self.pair_lists, self.triple_lists, self.quadruple_lists = [], [], []

    def register_pair_list(self, fpl, rate):
        if not isinstance(fpl, FixedPairListLambda):
            raise TypeError("FixedListDynamicResolution.register_pair_list: needs an espressopp.FixedPairListLambda")
        fpl._set_rate(rate)
        self.pair_lists.append((fpl, float(rate)))

    def register_triple_list(self, ftl, rate):
        if not isinstance(ftl, FixedTripleListLambda):
            raise TypeError("FixedListDynamicResolution.register_triple_list: needs an espressopp.FixedTripleListLambda")
        ftl._set_rate(rate)
        self.triple_lists.append((ftl, float(rate)))

    def register_quadruple_list(self, fql, rate):
        if not isinstance(fql, FixedQuadrupleListLambda):
            raise TypeError("FixedListDynamicResolution.register_quadruple_list: needs an espressopp.FixedQuadrupleListLambda")
        fql._set_rate(rate)
        self.quadruple_lists.append((fql, float(rate)))

    def _connect(self, integrator):
        pass


class _BasicDynamicResolution(object):
    """integrator.BasicDynamicResolution(system, {type: alpha}) + add_postprocess(PostProcessChangeProperty(type, props))
    (reaction_setup.py:322-354): every particle of such a type with lambda < 1 gains alpha per MD step; when it reaches 1
    the post-process of its type changes type, mass, charge (and state).  Nothing runs per step here: the engine evaluates
    lambda from the step counter and the particle's stamp and splits its runs at the completion steps (chem_resolution_rate)."""

    def __init__(self, system, type2alpha=None):
        self.system = system
        self.type2alpha = {int(t): float(a) for t, a in (type2alpha or {}).items()}
        self._pp = []

    def add_postprocess(self, pp):
        if not isinstance(pp, _PostProcessChangeProperty):
            raise NotImplementedError("post-process %s of BasicDynamicResolution is outside the hot-path scope" % type(pp).__name__)
        self._pp.append(pp)

    def _connect(self, integrator):
        if self.system.storage is not None:
            self.system.storage.decompose()
        for t, alpha in sorted(self.type2alpha.items()):
            ch = None
            for pp in self._pp:
                ch = pp.changes.get(t, ch)
            if ch is None or ch.type is None:
                self.system.engine.resolution_rate(t, alpha)
            else:
                self.system.engine.resolution_rate(t, alpha, new_type=int(ch.type), new_mass=float(ch.mass), new_q=float(ch.q or 0.0),
                                                   new_state=-1 if ch.state is None else int(ch.state))

    def disconnect(self):
        for t in sorted(self.type2alpha):
            self.system.engine.resolution_rate(t, 0.0)


class _FixDistances(object):
    """integrator.FixDistances(system, fix_list[, anchor_type, target_type]) + add_triplet, add_postprocess(
    PostProcessChangeProperty), get_all_triplets (reaction_post_process.py:269-289): every (anchor, target, distance) keeps
    the target at that distance from its anchor on every MD step, on the device (chem_fix_create / chem_fix_add); with types,
    an entry leaves when its anchor or target no longer has that type.  The post-process says what a released target becomes."""

    def __init__(self, system, fix_list=None, anchor_type=None, target_type=None):
        self.system = system
        self._list = [(int(a), int(t), float(d)) for a, t, d in (fix_list or [])]
        self.anchor_type = -1 if anchor_type is None else int(anchor_type)
        self.target_type = -1 if target_type is None else int(target_type)
        self._pp = []
        self.handle = None

    def add_triplet(self, anchor, target, dist):
        if self.handle is None:
            self._list.append((int(anchor), int(target), float(dist)))
        else:
            self.system.engine.fix_add(self.handle, [(int(anchor), int(target))], float(dist))

    def add_postprocess(self, pp):
        if not isinstance(pp, _PostProcessChangeProperty):
            raise NotImplementedError("post-process %s of FixDistances is outside the hot-path scope" % type(pp).__name__)
        self._pp.append(pp)
        if self.handle is not None:
            self._send_postprocess(pp)

    def _send_postprocess(self, pp):
        for old, ch in sorted(pp.changes.items()):
            self.system.engine.fix_postprocess(self.handle, old, new_type=-1 if ch.type is None else int(ch.type),
                                               new_mass=float(ch.mass) if ch.mass is not None else 0.0, new_q=float(ch.q or 0.0),
                                               new_state=-1 if ch.state is None else int(ch.state),
                                               lam=-1.0 if getattr(ch, "lambda_adr", None) is None else float(ch.lambda_adr))

    def _connect(self, integrator):
        if self.handle is not None:
            return
        if self.system.storage is not None:
            self.system.storage.decompose()
        e = self.system.engine
        self.handle = e.fix_create(self.anchor_type, self.target_type)
        k = 0
        while k < len(self._list):          # one call per run of equal distances, insertion order kept
            m = k
            while m < len(self._list) and self._list[m][2] == self._list[k][2]:
                m += 1
            e.fix_add(self.handle, [(a, t) for a, t, _ in self._list[k:m]], self._list[k][2])
            k = m
        for pp in self._pp:
            self._send_postprocess(pp)

    def get_all_triplets(self):
        if self.handle is None:
            return list(self._list)
        ids, dist = self.system.engine.fix_get(self.handle)
        return [(int(a), int(t), float(d)) for (a, t), d in zip(ids.tolist(), dist.tolist())]

    def totalSize(self):
        return len(self._list) if self.handle is None else int(self.system.engine.fix_count(self.handle))


class _PostProcessReleaseParticles(object):
    """integrator.PostProcessReleaseParticles(fd, count) (reaction_post_process.py:278): attached to a Reaction with
    add_postprocess(pp, 'type_1' | 'type_2' | 'both'), every bond-forming event releases up to `count` entries of `fd` whose
    anchor is that reactant (chem_reaction_release)."""

    def __init__(self, fd, count=1):
        if not isinstance(fd, _FixDistances):
            raise TypeError("PostProcessReleaseParticles(FixDistances, count)")
        self.fd, self.count = fd, int(count)


class _PostProcessRemoveNeighbourBond(object):
    """integrator.PostProcessRemoveNeighbourBond(topology_manager).add_bond_to_remove(anchor_type, nb_level, type_1, type_2)
    (reaction_post_process.py:117-137), attached to a Reaction with add_postprocess(pp, 'type_1' | 'type_2' | 'both'): the bonds
    type_1 - type_2 found nb_level bonds from a reactant of type anchor_type are taken out (chem_reaction_remove_bond).
    `unexclude` (this shim's own attribute, default True, as DissociationReaction's): the freed pair interacts through the pair
    potential again.  The argument defaults to None and a call without it is refused: the reference's constructor takes the
    topology manager, and a bare call is how callers ask whether the post-process exists at all."""

    def __init__(self, topology_manager=None):
        if topology_manager is None:
            raise NotImplementedError("integrator.PostProcessRemoveNeighbourBond needs the topology manager")
        self.rules = []     # (anchor_type, nb_level, type_1, type_2) in insertion order
        self.unexclude = True

    def add_bond_to_remove(self, anchor_type, nb_level, type_1, type_2):
        self.rules.append((int(anchor_type), int(nb_level), int(type_1), int(type_2)))


class _PostProcessJoinParticles(object):
    """integrator.PostProcessJoinParticles(fd, eq_length) (reaction_post_process.py:351), attached to a Reaction with
    add_postprocess(pp, 'type_1'): on every event that reactant becomes the anchor and the other one the target of a new
    entry of `fd` at eq_length (chem_reaction_join).  Both arguments default to None and a call without them is refused, as
    for PostProcessRemoveNeighbourBond."""

    def __init__(self, fd=None, eq_length=None):
        if fd is None or eq_length is None:
            raise NotImplementedError("integrator.PostProcessJoinParticles needs a FixDistances and a length")
        if not isinstance(fd, _FixDistances):
            raise TypeError("PostProcessJoinParticles(FixDistances, eq_length)")
        self.fd, self.eq_length = fd, float(eq_length)


class ParticleRegion(object):
    """espressopp.ParticleRegion(storage, integrator, lo, hi) + add_type_id (reaction_post_process.py:186-191): the particles of
    the listed types inside the box [lo, hi) of folded coordinates.  Nothing is tracked here: the engine tests the box on the
    device at every firing of the rule that uses the region (chem_region_add)."""

    def __init__(self, storage, integrator, lo, hi):
        self.storage, self.integrator = storage, integrator
        self.lo, self.hi = [float(v) for v in lo], [float(v) for v in hi]
        self.type_ids = []

    def add_type_id(self, type_id):
        if int(type_id) not in self.type_ids:
            self.type_ids.append(int(type_id))


class _RegionExtension(object):
    """what ChangeInRegion and ChangeParticleType share: rules sent once, enabled by _connect, disabled by disconnect"""

    def _rules(self):
        raise NotImplementedError

    def _connect(self, integrator):
        e = self.system.engine
        if self._handles is None:
            if self.system.storage is not None:
                self.system.storage.decompose()
            seed = self.system.rng.get_seed() if self.system.rng is not None else 0
            self._handles = [e.region_add(seed=seed, what=type(self).__name__.lstrip("_"), **kw) for kw in self._rules()]
        for h in self._handles:
            e.region_enable(h, True)

    def disconnect(self):
        for h in self._handles or []:
            self.system.engine.region_enable(h, False)


class _ChangeInRegion(_RegionExtension):
    """integrator.ChangeInRegion(system, region, prob=, p_num=, p_num_percentage=) + set_particle_properties(type,
    TopologyParticleProperties), set_flags(type, reset_velocity, reset_force, remove_particle), stats_filename
    (reaction_post_process.py:193-199): on every step the selected particles of the region's types that lie inside it get the
    new properties.  Selection: prob, else p_num, else p_num_percentage (the order the reference names them); with none of them
    every candidate.  One region rule per type that has properties (chem_region_add), on when the extension is added to the
    integrator.  Removing particles is not served."""

    def __init__(self, system, region, prob=None, p_num=None, p_num_percentage=None):
        if not isinstance(region, ParticleRegion):
            raise TypeError("ChangeInRegion(system, ParticleRegion, ...)")
        self.system, self.region = system, region
        self.prob, self.p_num, self.p_num_percentage = prob, p_num, p_num_percentage
        self.stats_filename = None
        self._props, self._flags, self._handles = {}, {}, None
        regs = getattr(system, "_region_extensions", None)
        if regs is None:
            regs = system._region_extensions = []
        regs.append(self)

    def set_particle_properties(self, type_id, props):
        if props.type is None:
            raise ValueError("ChangeInRegion.set_particle_properties: the properties name no type")
        self._props[int(type_id)] = props

    def set_flags(self, type_id, reset_velocity=False, reset_force=False, remove_particle=False):
        if remove_particle:
            raise NotImplementedError("ChangeInRegion.set_flags(remove_particle=True): the engine cannot remove particles")
        self._flags[int(type_id)] = (bool(reset_velocity), bool(reset_force))

    def _selection(self):
        if self.prob is not None:
            return dict(mode="prob", value=float(self.prob))
        if self.p_num is not None:
            return dict(mode="num", num=int(self.p_num))
        if self.p_num_percentage is not None:
            return dict(mode="fraction", value=float(self.p_num_percentage))
        return dict(mode="all")

    def _rules(self):
        out = []
        for t in self.region.type_ids:
            p = self._props.get(t)
            if p is None:
                continue
            rv, rf = self._flags.get(t, (False, False))
            kw = dict(lo=self.region.lo, hi=self.region.hi, target_type=t, new_type=int(p.type), interval=1, reset_velocity=rv, reset_force=rf)
            if p.mass is not None:
                kw.update(new_mass=float(p.mass), new_q=float(p.q or 0.0))
            kw.update(self._selection())
            out.append(kw)
        return out

    def save_stats(self, filename=None):
        """`step rule candidates changed`, one row per firing of a rule that changed something: the rows of every ChangeInRegion
        of the system that names the same file (the six regions of a FreezeRegion share one)."""
        filename = filename or self.stats_filename
        mine = set(h for x in self.system._region_extensions if (filename is None and x is self) or (filename and x.stats_filename == filename)
                   for h in (x._handles or []))
        rows = [r for r in self.system.engine.region_stats() if int(r["rule"]) in mine] if mine else []
        if filename:
            with _rank.wopen(filename, "w") as f:
                f.write("# step rule candidates changed\n")
                for r in rows:
                    f.write("%d %d %d %d\n" % (r["step"], r["rule"], r["candidates"], r["changed"]))
        return rows


class _ChangeParticleType(_RegionExtension):
    """integrator.ChangeParticleType(system, interval, num_particles, old_type, new_type) (reaction_post_process.py:364-378):
    every `interval` steps `num_particles` random particles of old_type become new_type; mass, charge, velocity and force are
    kept.  A region rule over the whole box, selection by count."""

    def __init__(self, system, interval, num_particles, old_type, new_type):
        self.system = system
        self.interval, self.num_particles, self.old_type, self.new_type = int(interval), int(num_particles), int(old_type), int(new_type)
        self._handles = None

    def _rules(self):
        return [dict(lo=[0.0, 0.0, 0.0], hi=[float(b) for b in self.system.bc.boxL], target_type=self.old_type, new_type=self.new_type,
                     interval=self.interval, mode="num", num=self.num_particles)]


integrator = _ns(
    ChangeInRegion=_ChangeInRegion, ChangeParticleType=_ChangeParticleType,
    FixDistances=_FixDistances, PostProcessReleaseParticles=_PostProcessReleaseParticles,
    VelocityVerlet=_VelocityVerlet, FixedListDynamicResolution=_FixedListDynamicResolution, LangevinThermostat=_LangevinThermostat, ChemicalReaction=_ChemicalReaction,
    Reaction=_Reaction, PostProcessChangeProperty=_PostProcessChangeProperty,
    PostProcessChangePropertyByTopologyManager=_PostProcessChangeProperty, ReactionConstraintNeighbourState=_ReactionConstraintNeighbourState,
    TopologyParticleProperties=_TopologyParticleProperties, TopologyManager=_TopologyManager, ExtAnalyze=_ExtAnalyze,
    StochasticVelocityRescaling=_StochasticVelocityRescaling,
    BerendsenThermostat=_BerendsenThermostat, BerendsenBarostat=_BerendsenBarostat,
    Isokinetic=_Isokinetic, LangevinBarostat=_LangevinBarostat,
    CapForce=_CapForce, RestrictReaction=_RestrictReaction,
    DissociationReaction=_DissociationReaction, ATRPActivator=_ATRPActivator,
    ReactionCutoffRandom=_unsupported("integrator.ReactionCutoffRandom"),
    BasicDynamicResolution=_BasicDynamicResolution,
    PostProcessChangeNeighboursProperty=_PostProcessChangeNeighboursProperty,
    PostProcessRemoveNeighbourBond=_PostProcessRemoveNeighbourBond, PostProcessJoinParticles=_PostProcessJoinParticles,
)


# ---- analysis ------------------------------------------------------------------------------------
class _Observable(object):
    def __init__(self, system, *a):
        self.system, self.args = system, a

    def compute(self):
        raise NotImplementedError


class _Temperature(_Observable):
    """analysis.Temperature(system) + add_type(type_id) (start_simulation.py:453-456): with types, the temperature of the
    particles of those types alone, 3 degrees of freedom each; without, the engine's own."""

    def __init__(self, system, *a):
        _Observable.__init__(self, system, *a)
        self._types = []

    def add_type(self, type_id):
        if type_id is not None and int(type_id) not in self._types:
            self._types.append(int(type_id))

    def compute(self):
        e = self.system.engine
        if not self._types:
            return e.observe()["temperature"]
        sel = np.isin(e.get_state("TYPE"), self._types)
        if not sel.any():
            return 0.0
        v, m = e.get_state("VEL")[sel], e.get_state("MASS")[sel]
        return float((m[:, None] * v * v).sum() / (3.0 * sel.sum()))


class _NumFixDistances(_Observable):
    """analysis.NumFixDistances(system, fd) (start_simulation.py:561-563): the number of live entries."""

    def __init__(self, system, fd):
        _Observable.__init__(self, system)
        self.fd = fd

    def compute(self):
        return self.fd.totalSize()


class _KineticEnergy(_Observable):
    def __init__(self, system, temperature=None):
        _Observable.__init__(self, system)

    def compute(self):
        return self.system.engine.observe()["ekin"]


class _Pressure(_Observable):
    """analysis.Pressure(system).compute(): (sum m v^2 + W) / (3 V) in the engine's units (start_simulation.py:466-469;
    include/chem_mi355.h chem_get_pressure)."""

    def __init__(self, system):
        _Observable.__init__(self, system)

    def compute(self):
        return self.system.engine.pressure()["pressure"]


class _PressureTensor(_Observable):
    """analysis.PressureTensor(system).compute(): the six components (K_ab + W_ab) / V in the order xx, yy, zz, xy, xz, yz, in
    the engine's units (include/chem_mi355.h chem_get_pressure_tensor)."""

    def __init__(self, system):
        _Observable.__init__(self, system)

    def compute(self):
        return [float(c) for c in self.system.engine.pressure_tensor()["tensor"]]


class _RadialDistrF(_Observable):
    """analysis.RadialDistrF(system): g(r) accumulated on the device (include/chem_mi355.h chem_rdf_*).

    compute(nbins, r_max=None, types=None) takes one frame of the current configuration and returns g of the first selector as
    a list of nbins values; `types` is a list of (t1, t2) pairs, -1 = any type (default: all pairs).  Upstream's class bins one
    configuration on the host out to half the box; this one stops at the list cutoff max_cutoff (r_max=None means max_cutoff),
    because the device's tile tables hold nothing beyond it.  For a time average inside integrator.run use
    start(nbins, r_max, types, every, split_molecules) once and result() (the dict of Engine.rdf()) when the run is over."""

    def __init__(self, system):
        _Observable.__init__(self, system)

    def _init(self, nbins, r_max, types, split_molecules=False):
        e = self.system.engine
        if not e.supports("rdf"):
            raise NotImplementedError("rdf: the CPU checker has no pair histogram")
        if r_max is None:
            r_max = self.system.max_cutoff
        if r_max is None:
            raise ValueError("RadialDistrF: no r_max and no list cutoff yet (VerletList sets it)")
        e.rdf_init(float(r_max), int(nbins), [(-1, -1)] if types is None else [tuple(t) for t in types], bool(split_molecules))
        return e

    def compute(self, nbins, r_max=None, types=None):
        e = self._init(nbins, r_max, types)
        e.rdf_sample()
        return [float(v) for v in e.rdf()["g"][0, 0]]

    def start(self, nbins, r_max=None, types=None, every=1, split_molecules=False):
        self._init(nbins, r_max, types, split_molecules).rdf_sample_every(int(every))

    def result(self):
        return self.system.engine.rdf()


class _StaticStructF(_Observable):
    """analysis.StaticStructF(system): partial structure factors on the reciprocal lattice of the box, accumulated on the device
    (include/chem_mi355.h chem_sq_*).

    start(nmax, types=None, every=1) once, behind the set-up: a frame inside integrator.run at every step s with s % every == 0,
    the wave vectors 2 pi n / L with |n_a| <= nmax, one S per (t1, t2) of `types` (-1 = any type; default the total); result()
    is the dict of Engine.sq() when the run is over.  compute(nmax, types=None) takes one frame of the current configuration and
    returns the shell-averaged S of the first selector as a list.  (Upstream's class takes (nqx, nqy, nqz, bin_factor) and works
    on the host; this rule set is this build's own.)"""

    def __init__(self, system):
        _Observable.__init__(self, system)

    def _init(self, nmax, types):
        e = self.system.engine
        if not e.supports("sq"):
            raise NotImplementedError("sq: the CPU checker has no structure factor")
        e.sq_init(int(nmax), [(-1, -1)] if types is None else [tuple(t) for t in types])
        return e

    def compute(self, nmax, types=None):
        e = self._init(nmax, types)
        e.sq_sample()
        return [float(v) for v in e.sq()["shell_S"][0]]

    def start(self, nmax, types=None, every=1):
        self._init(nmax, types).sq_sample_every(int(every))

    def result(self):
        return self.system.engine.sq()


class _BoxSize(_Observable):
    """The `L` column that goes with `P` (start_simulation.py:466-469): the x edge of the current box.  The reference's
    class is in the external fork; what it reports for a box that is not cubic is unpinned."""

    def __init__(self, system):
        _Observable.__init__(self, system)

    def compute(self):
        return float(self.system.bc.boxL[0])


class _PotentialEnergy(_Observable):
    def __init__(self, system, interaction_, compute_method=None):
        _Observable.__init__(self, system)
        self.interaction = interaction_

    def compute(self):
        i = self.interaction
        if isinstance(i, _VerletListCoulombTruncated):
            return self.system.engine.get_coulomb()[0]
        o = self.system.engine.observe()
        if isinstance(i, (_VerletListLennardJones, _VerletListDynamicResolutionLennardJones, _VerletListLennardJonesCapped)):      # (one LJ accumulator: plain and resolution-scaled pairs together)
            return o["epot_lj"]
        if isinstance(i, (_VerletListTabulated, _VerletListMixedTabulated, _VerletListDynamicResolutionTabulated, _VerletListTabulatedCapped)):    # (one tabulated-energy accumulator: plain and mixed tables together)
            return o["epot_tab"]
        h = getattr(i, "handle", None)      # the interaction's own library list (a list object carries one per kind)
        if h is None:
            h = i.flist.handle
        return o["epot_list"][h] if h is not None else 0.0


class _NPart(_Observable):
    def compute(self):
        return self.system.engine.n


class _MaxPID(_Observable):
    def compute(self):
        return int(self.system.engine.get_state("ID").max())


class _NFixedPairListEntries(_Observable):
    def __init__(self, system, fpl):
        _Observable.__init__(self, system)
        self.fpl = fpl

    def compute(self):
        return self.fpl.totalSize()


class _ResolutionFixedPairList(_Observable):
    """analysis.ResolutionFixedPairList(system, fpl) (start_simulation.py:495-498): mean lambda of the list's bonds, 0.0 for
    an empty list."""

    def __init__(self, system, fpl):
        _Observable.__init__(self, system)
        self.fpl = fpl

    def compute(self):
        lam = self.fpl.getAllLambda()
        return float(sum(lam)) / len(lam) if len(lam) else 0.0


class _ResolutionFixedTripleList(_ResolutionFixedPairList):
    """analysis.ResolutionFixedTripleList(system, ftl): mean lambda of the list's angles, 0.0 for an empty list."""


class _ResolutionFixedQuadrupleList(_ResolutionFixedPairList):
    """analysis.ResolutionFixedQuadrupleList(system, fql): mean lambda of the list's dihedrals, 0.0 for an empty list."""


class _CMVelocity(_Observable):
    def reset(self):
        pass   # the synthetic/initial velocities are generated with zero COM momentum

    def compute(self):
        o = self.system.engine.observe()
        return Real3D(*o["momentum"])


class _ChemicalConversion(_Observable):
    def __init__(self, system, type_id, total=None):
        _Observable.__init__(self, system)
        self.type_id, self.total = type_id, total

    def compute(self):
        t = self.system.engine.get_state("TYPE")
        c = float((t == self.type_id).sum())
        val = c / self.total if self.total else c
        for fn in getattr(self, "_listeners", ()):       # the reference's onValue signal: MixedTabulated follows the conversion
            fn(val)
        return val

    def connect(self, fn):
        self.__dict__.setdefault("_listeners", []).append(fn)


class _ChemicalConversionTypeState(_Observable):
    def __init__(self, system, type_id, state, total=None):
        _Observable.__init__(self, system)
        self.type_id, self.state, self.total = type_id, state, total

    def compute(self):
        e = self.system.engine
        c = float(((e.get_state("TYPE") == self.type_id) & (e.get_state("STATE") == self.state)).sum())
        return c / self.total if self.total else c


class _SystemMonitorOutputCSV(object):
    def __init__(self, filename, delimiter=","):
        self.filename, self.delimiter = filename, delimiter
        self._header_written = False

    def write(self, names, row):
        with _rank.wopen(self.filename, "a") as f:
            if not self._header_written:
                f.write(self.delimiter.join(names) + "\n")
                self._header_written = True
            f.write(self.delimiter.join("%g" % v for v in row) + "\n")


class _SystemMonitor(object):
    """analysis.SystemMonitor(system, integrator, output) + add_observable/info
    (start_simulation.py:447-569)."""

    def __init__(self, system, integrator_, output):
        self.system, self.integrator, self.output = system, integrator_, output
        self.obs = []
        self.last = None
        self.copy_state = None

    def add_observable(self, name, observable, visible=True):
        self.obs.append((name, observable, visible))

    def perform_action(self):
        names = ["step", "time"] + [n for n, _, _ in self.obs]
        row = [self.integrator.step, self.integrator.step * (self.integrator.dt or 0.0)] + [float(o.compute()) for _, o, _ in self.obs]
        self.last = (names, row)
        if self.output is not None:
            self.output.write(names, row)

    def info(self):
        if self.last is None:
            return
        names, row = self.last
        vis = ["step", "time"] + [n for n, _, v in self.obs if v]
        print(" ".join("%s=%g" % (n, v) for n, v in zip(names, row) if n in vis))

    def dump(self):
        pass


analysis = _ns(
    Temperature=_Temperature, KineticEnergy=_KineticEnergy, PotentialEnergy=_PotentialEnergy, NPart=_NPart, MaxPID=_MaxPID,
    NFixedPairListEntries=_NFixedPairListEntries, NumFixDistances=_NumFixDistances, CMVelocity=_CMVelocity, ChemicalConversion=_ChemicalConversion,
    ChemicalConversionTypeState=_ChemicalConversionTypeState, SystemMonitor=_SystemMonitor,
    SystemMonitorOutputCSV=_SystemMonitorOutputCSV, ResolutionFixedPairList=_ResolutionFixedPairList,
    ResolutionFixedTripleList=_ResolutionFixedTripleList, ResolutionFixedQuadrupleList=_ResolutionFixedQuadrupleList,
    Pressure=_Pressure, BoxSize=_BoxSize, PressureTensor=_PressureTensor, RadialDistrF=_RadialDistrF, StaticStructF=_StaticStructF,
)

esutil = _ns(RNG=_RNG)
bc = _ns(OrthorhombicBC=_OrthorhombicBC)
storage = _ns(DomainDecomposition=_DomainDecomposition)


def _gaussian_velocities(T, n, masses, kb=1.0, seed=0):
    """tools.velocities.gaussian: Maxwell velocities with zero COM momentum (start_simulation.py:136-146)."""
    rng = np.random.default_rng(seed)
    m = np.asarray(masses, dtype=np.float64)
    v = rng.standard_normal((n, 3)) * np.sqrt(kb * T / m)[:, None]
    v -= (m[:, None] * v).sum(0) / m.sum()
    return v[:, 0], v[:, 1], v[:, 2]


tools = _ns(decomp=_ns(nodeGrid=_node_grid, cellGrid=_cell_grid, tuneSkin=_unsupported("tools.decomp.tuneSkin")),
            velocities=_ns(gaussian=_gaussian_velocities),
            analyse=_ns(final_info=lambda *a, **k: None))
class _DumpGRO(object):
    """io.DumpGRO(system, integrator, filename, unfolded=False, append=False): every particle, generic names
    (start_simulation.py:1014-1016)."""

    def __init__(self, system, integrator, filename="out.gro", unfolded=False, append=False, **kw):
        self.system, self.filename, self.unfolded, self.append = system, filename, unfolded, append

    def dump(self):
        e = self.system.engine
        ids, pos = e.get_state("ID"), e.get_state("POS_UNFOLDED" if self.unfolded else "POS")
        vel, types, res = e.get_state("VEL"), e.get_state("TYPE"), e.get_state("RESID")
        box = list(self.system.bc.boxL)
        with _rank.wopen(self.filename, "a" if self.append else "w") as f:
            f.write("system size %d\n%d\n" % (len(ids), len(ids)))
            for k in range(len(ids)):
                f.write("%5d%-5s%5s%5d%8.3f%8.3f%8.3f%8.4f%8.4f%8.4f\n" % (int(res[k]) % 100000, "T%d" % types[k], "T%d" % types[k], int(ids[k]) % 100000,
                                                                            pos[k, 0], pos[k, 1], pos[k, 2], vel[k, 0], vel[k, 1], vel[k, 2]))
            f.write("%f %f %f\n" % tuple(box))

    perform_action = dump


class _DumpH5MD(object):
    """io.DumpH5MD(system, filename, group_name='atoms', store_species=..., store_state=..., ...) -- the trajectory writer
    of start_simulation.py:571-589: dump(step, time) appends one frame, flush() writes the file, close().
    Layout = the H5MD tree analysis scripts read (examples/chain_growth_catalytic/Checkup.ipynb,
    examples/mf/espp_cg_1_water/analyze.py:20-24):
        /particles/<group>/{position,image,species,state,res_id,mass,id,velocity,force}/{value,step,time}   value: [frames, N(, 3)]
        /particles/<group>/box/edges/{value,step,time}                                                   value: [frames, 3]
        /connectivity/<name>/{value,step,time}     value: [frames, max entries, arity], unused rows filled with -1
    With h5py importable the file is real HDF5; otherwise (this image) the same tree is written as a NumPy .npz archive
    whose keys are the dataset paths (`<filename minus .h5>.npz`); tools/npz2h5md.py turns it into the .h5 file."""

    def __init__(self, system, filename, group_name="atoms", static_box=True, author="", email="", store_species=True, store_res_id=True,
                 store_charge=False, store_position=True, store_state=True, store_lambda=False, store_force=False, store_velocity=False,
                 store_mass=True, is_single_prec=True, chunk_size=256, **kw):
        self.system, self.filename, self.group = system, filename, group_name
        self.store = dict(species=store_species, res_id=store_res_id, position=store_position, state=store_state, force=store_force,
                          velocity=store_velocity, mass=store_mass, lambda_adr=store_lambda)
        self.real = np.float32 if is_single_prec else np.float64
        self.frames = {}            # dataset path -> list of per-frame arrays
        self.steps, self.times = [], []
        self.connectivity = {}      # name -> dict(value=[...], step=[...], time=[...], arity)
        self.static_connectivity = {}

    def _add(self, name, arr):
        self.frames.setdefault("particles/%s/%s/value" % (self.group, name), []).append(arr)

    def dump(self, step, time_):
        e = self.system.engine
        self.steps.append(int(step)); self.times.append(float(time_))
        self._add("id", e.get_state("ID").astype(np.int64))
        if self.store["position"]:
            self._add("position", e.get_state("POS").astype(self.real))
            self._add("image", e.get_state("IMAGE").astype(np.int32))
        if self.store["velocity"]:
            self._add("velocity", e.get_state("VEL").astype(self.real))
        if self.store["force"]:
            self._add("force", e.get_state("FORCE").astype(self.real))
        if self.store["species"]:
            self._add("species", e.get_state("TYPE").astype(np.int32))
        if self.store["state"]:
            self._add("state", e.get_state("STATE").astype(np.int32))
        if self.store["res_id"]:
            self._add("res_id", e.get_state("RESID").astype(np.int32))
        if self.store["mass"]:
            self._add("mass", e.get_state("MASS").astype(self.real))
        if self.store["lambda_adr"]:
            self._add("lambda_adr", e.get_state("LAMBDA").astype(self.real))
        self.frames.setdefault("particles/%s/box/edges/value" % self.group, []).append(np.asarray(list(self.system.bc.boxL), dtype=self.real))

    def tree(self):
        """dataset path -> array, as written by flush()."""
        out = {}
        st, tm = np.asarray(self.steps, dtype=np.int64), np.asarray(self.times, dtype=np.float64)
        for path, fr in self.frames.items():
            out[path] = np.stack(fr) if fr else np.zeros((0,))
            base = path[:-len("/value")]
            out[base + "/step"], out[base + "/time"] = st[:len(fr)], tm[:len(fr)]
        for name, c in self.connectivity.items():
            rows = max([len(v) for v in c["value"]] + [1])
            val = -np.ones((len(c["value"]), rows, c["arity"]), dtype=np.int64)
            for k, v in enumerate(c["value"]):
                if len(v):
                    val[k, :len(v)] = v
            out["connectivity/%s/value" % name] = val
            out["connectivity/%s/step" % name] = np.asarray(c["step"], dtype=np.int64)
            out["connectivity/%s/time" % name] = np.asarray(c["time"], dtype=np.float64)
        for name, v in self.static_connectivity.items():
            out["connectivity/%s" % name] = v
        return out

    def flush(self):
        tree = self.tree()
        if not _rank.is_root():
            return self.filename
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(self.filename, "w") as h5:
                for path, arr in tree.items():
                    h5.create_dataset(path, data=arr)
            return self.filename
        out = self.filename[:-3] + ".npz" if self.filename.endswith(".h5") else self.filename + ".npz"
        np.savez_compressed(out, **tree)
        return out

    def close(self):
        return self.flush()


class _DumpTopology(object):
    """io.DumpTopology(system, integrator, h5md_file): observe_tuple/triple/quadruple(list, name) record the CURRENT entries of
    a (growing) list at every dump() into /connectivity/<name> (-1 padded rows); add_static_* store a list once
    (start_simulation.py:591-642).  Used through ExtAnalyze(dump_topol, topol_collect); update() is the reference's
    flush-to-file hook (a no-op here: the trajectory object writes everything in flush())."""

    def __init__(self, system, integrator, h5md_file):
        self.system, self.integrator, self.h5 = system, integrator, h5md_file
        self._observed = []

    def _observe(self, lst, name, arity):
        self._observed.append((lst, name))
        self.h5.connectivity[name] = dict(value=[], step=[], time=[], arity=arity)

    def observe_tuple(self, fpl, name):
        self._observe(fpl, name, 2)

    def observe_triple(self, ftl, name):
        self._observe(ftl, name, 3)

    def observe_quadruple(self, fql, name):
        self._observe(fql, name, 4)

    @staticmethod
    def _entries(lst):
        for getter in ("getAllBonds", "getAllTriples", "getAllQuadruples"):
            if hasattr(lst, getter):
                try:
                    return np.asarray(getattr(lst, getter)(), dtype=np.int64)
                except Exception:
                    continue
        return np.zeros((0, 2), dtype=np.int64)

    def add_static_tuple(self, fpl, name):
        self.h5.static_connectivity[name] = self._entries(fpl).reshape(-1, 2)

    def add_static_triple(self, ftl, name):
        self.h5.static_connectivity[name] = self._entries(ftl).reshape(-1, 3)

    def add_static_quadruple(self, fql, name):
        self.h5.static_connectivity[name] = self._entries(fql).reshape(-1, 4)

    def dump(self):
        step = self.integrator.step
        for lst, name in self._observed:
            c = self.h5.connectivity[name]
            c["value"].append(self._entries(lst).reshape(-1, c["arity"]))
            c["step"].append(int(step)); c["time"].append(float(step) * float(self.integrator.dt or 0.0))

    perform_action = dump
    perform = dump

    def update(self):
        pass


io = _ns(DumpH5MD=_DumpH5MD, DumpTopology=_DumpTopology, DumpGRO=_DumpGRO)
