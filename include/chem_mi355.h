/*
 * chem_mi355.h -- C ABI of libchem_mi355.so, the MI355X-native reactive-MD inner loop
 * that replaces the modified-ESPResSo++ back end ChemLab drives.
 *
 * The reference (cgchemlab/chemlab) has no C ABI: its hot path is reached through
 * Boost.Python `espressopp.*` objects.  Every entry point below therefore cites the
 * ChemLab call site (file:line under /root/reference) whose espressopp call it replaces.
 * INTEGRATION.md shows the py3 `espressopp`-shaped shim (ctypes) a maintainer binds
 * on top of these symbols.
 *
 * Conventions
 *  - every function returns 0 (or a count >= 0) on success and a negative CHEM_E* code on
 *    failure; the message is available from chem_last_error(ctx);
 *  - the caller owns every input buffer; it is copied during the call;
 *  - the context owns all device memory; outputs go to caller-allocated buffers with a
 *    capacity, the return value is the element count (CHEM_ENOSPC if cap is too small);
 *  - a context is bound to one GPU and is not thread-safe; multi-GPU = one context per
 *    rank (one process per GPU), joined with chem_comm_init();
 *  - there is NO CPU fall-back behind these symbols: without a gfx950 device
 *    chem_create() fails.
 */
#ifndef CHEM_MI355_H
#define CHEM_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHEM_ABI_VERSION 1

/* error codes */
#define CHEM_OK        0
#define CHEM_EINVAL   -1   /* bad argument */
#define CHEM_ENOSPC   -2   /* output capacity too small / internal capacity exceeded */
#define CHEM_EDEVICE  -3   /* HIP error or no usable device */
#define CHEM_ESTATE   -4   /* call sequence error (e.g. run before particles) */
#define CHEM_ENOTIMPL -5   /* feature outside the hot-path scope */
#define CHEM_ECOMM    -6   /* RCCL error */

/* arithmetic precision of the device path (chem_create) */
#define CHEM_PREC_F32 32   /* fp32 positions/velocities/forces, fp64 bonded + reaction distance */
#define CHEM_PREC_F64 64   /* everything fp64 (parity mode)                                    */

/* bonded potential kinds (chem_list_create).  Parameter vectors `p` for chem_list_set_params:
 *   HARMONIC        K, r0                 U = K (r-r0)^2            gromacs_topology.py:918,949-961
 *   FENE            K, r0, rMax           U = -K/2 rMax^2 ln(1-((r-r0)/rMax)^2)      :926-931
 *   ANG_HARMONIC    K, theta0[rad]        U = K (theta-theta0)^2                    :1073,1086
 *   ANG_COSINE      K, theta0[rad]        U = K (1+cos(theta-theta0))               :1082
 *   DIH_NCOS        K, phi0[rad], n       U = K (1+cos(n phi - phi0))               :1185-1190
 *   DIH_RB          C0..C5                U = sum_n C_n cos^n(phi-pi)               :1192-1198
 */
#define CHEM_POT_HARMONIC      1
#define CHEM_POT_FENE          2
#define CHEM_POT_TABULATED     3   /* bonds: params = { table handle } from chem_table_create */
#define CHEM_POT_FENE_LJ       4   /* bonds func 9, FENELennardJones(K, r0, rMax, sigma, epsilon): FENE + 4 eps ((s/r)^12 - (s/r)^6),
                                      doc/topology.rst:68-75, gromacs_topology.py:935-942 */
#define CHEM_POT_LJ_BOND       5   /* 1-4 pairs, FixedPairListLennardJones(epsilon, sigma, cutoff): plain LJ inside the cutoff,
                                      gromacs_topology.py:1314-1411 */
/* 1-4 Coulomb pairs, FixedPairListCoulombTruncated / FixedPairListTypesCoulombTruncated with CoulombTruncated(prefactor, cutoff),
 * gromacs_topology.py:1391-1409.  The arithmetic is in the external fork, so this rule set is this build's own ([EXT-RECALL],
 * parity unpinned like chem_nb_coulomb).  Arity 2, plain or by types, params = { prefactor k, cutoff rc }.
 * For a list entry (i, j) with minimum-image distance r <= rc (inclusive, compared as CHEM_POT_LJ_BOND compares):
 *     U = k q_i q_j / r,     F_i = k q_i q_j r_ij / r^3,     the energy is not shifted.
 *   - nothing else is asked of the entry: it need not be on the Verlet list nor be non-excluded, and rc is not bound by
 *     max_cutoff; the pair is found through its tags like every bonded term (same reach as an LJ 1-4 entry between slabs);
 *   - charges are the per-particle charges of chem_set_particles at the time of the force evaluation: a reaction (new_q),
 *     neighbour rule, ATRP flip, dissociation or chem_modify_particle(CHEM_STATE_CHARGE) acts from the next evaluation on
 *     (the rule of chem_nb_coulomb);
 *   - by types: parameters of the CURRENT type pair; an entry whose type pair has none contributes nothing;
 *   - the energy goes to the list's slot of chem_obs.epot_list; chem_get_coulomb keeps meaning the non-bonded term only;
 *   - chem_list_set_hybrid applies: force and energy times lambda;
 *   - bond graph, cluster labels and exclusions: exactly what chem_list_add does for an LJ 1-4 list;
 *   - chem_list_create with arity 3 or 4 is CHEM_ENOTIMPL; chem_list_set_params with np != 2, rc <= 0 or a non-finite value is
 *     CHEM_EINVAL; prefactor = 0 is allowed (a list that does nothing);
 *   - harmonic bonds are not evaluated inline while a list of this kind exists. */
#define CHEM_POT_COULOMB_BOND  6
#define CHEM_POT_ANG_HARMONIC 10
#define CHEM_POT_ANG_COSINE   11
#define CHEM_POT_ANG_TABULATED 12  /* angles func 8: params = { table handle }, grid in radians, f = -dU/dtheta */
#define CHEM_POT_DIH_NCOS     20
#define CHEM_POT_DIH_RB       21
#define CHEM_POT_DIH_HARMONIC  23  /* dihedrals func 12, DihedralHarmonic(K, phi0): U = K/2 (phi - phi0)^2, difference wrapped to
                                      (-pi, pi], doc/topology.rst:120-128, gromacs_topology.py:1199-1202 */
#define CHEM_POT_DIH_TABULATED 22  /* dihedrals func 8: params = { table handle }, grid in radians over [-pi, pi], f = -dU/dphi */
#define CHEM_MAX_POT_PARAMS    6
#define CHEM_MAX_LISTS        32
#define CHEM_MAX_TYPES        16
#define CHEM_MAX_REACTIONS    16

/* selectors for chem_get_state; all outputs are in ascending particle-id order */
#define CHEM_STATE_POS     1   /* double[n*3], folded into the box                 */
#define CHEM_STATE_VEL     2   /* double[n*3]                                      */
#define CHEM_STATE_FORCE   3   /* double[n*3], forces of the last evaluation       */
#define CHEM_STATE_TYPE    4   /* int32[n]                                         */
#define CHEM_STATE_STATE   5   /* int32[n]  chemical state                         */
#define CHEM_STATE_RESID   6   /* int32[n]                                         */
#define CHEM_STATE_MASS    7   /* double[n]  the mass the device integrates with: (float)m in the CHEM_PREC_F32 build */
#define CHEM_STATE_ID      8   /* int64[n]                                         */
#define CHEM_STATE_IMAGE   9   /* int32[n*3] periodic image counters               */
#define CHEM_STATE_MOLID  10   /* int32[n]  lowest particle id of the bonded cluster (CHEM_EINVAL with ids beyond 32 bits: chem_set_particles) */
#define CHEM_STATE_POS_UNFOLDED 11 /* double[n*3] = pos + image*L                  */
#define CHEM_STATE_CHARGE  12  /* double[n]; also a `what` of chem_modify_particle  */
#define CHEM_STATE_LAMBDA  13  /* double[n]  resolution lambda at the current step (chem_set_resolution); also a `what` of chem_modify_particle */

typedef struct chem_ctx chem_ctx;

/* One chemical reaction  T1(min1,max1) + T2(min2,max2) -> N1(d1):N2(d2).
 * Replaces espressopp.integrator.Reaction(type_1,type_2,delta_1,delta_2,min_state_1,
 * max_state_1,min_state_2,max_state_2,rate,fpl,cutoff) + .intramolecular/.intraresidual/
 * .is_virtual/.active, get_reaction_cutoff().min_cutoff and the PostProcessChangeProperty
 * type change (reaction_setup.py:81-163). */
typedef struct chem_reaction_desc {
  int32_t type_1, type_2;
  int32_t delta_1, delta_2;
  int32_t min_state_1, max_state_1;   /* half-open [min,max) */
  int32_t min_state_2, max_state_2;
  double  rate;
  double  cutoff;
  double  min_cutoff;
  int32_t intramolecular;             /* 1: partners may belong to one bonded cluster */
  int32_t intraresidual;              /* 1: partners may share res_id                 */
  int32_t is_virtual;                 /* 1: no bond is created                        */
  int32_t active;
  int32_t bond_list;                  /* handle of the arity-2 list receiving new bonds */
  int32_t new_type_1, new_type_2;     /* -1: unchanged                                */
  double  new_mass_1, new_mass_2;     /* used when the type changes: an event that names the type a particle already has
                                         leaves its mass alone (the charge is set wherever a new type is named)          */
  double  new_q_1, new_q_2;
} chem_reaction_desc;

/* One accepted reaction event; chem_get_events returns them sorted by
 * (step, min(id_a,id_b), max(id_a,id_b)). */
typedef struct chem_event {
  int64_t step;
  int64_t id_a, id_b;     /* particle taking role type_1 / type_2 */
  int32_t reaction;
  int32_t pad;            /* with option "count_intra_inter": 1 = both particles had one mol_id before this step's bonds (the
                             cluster labels as the step's scan read them: no bond of the same step counts); 0 without the option.
                             Served on every path, slabs included: the labels are replicated on every rank. */
  double  r2;             /* fp64 squared distance at decision time */
} chem_event;

typedef struct chem_obs {
  int64_t step;
  int64_t npart;
  double  ekin;
  double  temperature;             /* 2 Ekin / (3 N), in energy units (k_B T)  */
  double  epot_lj;                 /* VerletListLennardJones                   */
  double  epot_tab;                /* VerletListTabulated                      */
  double  epot_list[CHEM_MAX_LISTS];
  int64_t list_size[CHEM_MAX_LISTS];
  double  momentum[3];
  double  virial_nb;               /* sum_pairs r.F of non-bonded              */
} chem_obs;

typedef struct chem_timers {
  double run_wall_s;               /* wall seconds inside chem_run (== integratorLoop, start_simulation.py:779-781) */
  int64_t steps;
  int64_t rebuilds;
  int64_t reaction_steps;
  int64_t nlist_entries;           /* entries of the current full neighbour list */
  int64_t nlist_capacity;
  double  reaction_wall_s;
  double  rebuild_wall_s;          /* host-observed; only reaction-step/forced rebuilds are synchronous */
  double  pair_kernel_ms;          /* HIP-event time of all pair-force launches of the last chem_run */
  int64_t pair_kernel_launches;
  /* HIP-event samples of the per-step neighbour kernel (k_rebuild_fused) of the last chem_run, split
   * into launches that rebuilt the lists and launches that only took the decision */
  double  rebuild_kernel_ms;
  int64_t rebuild_kernel_launches;
  double  decide_kernel_ms;
  int64_t decide_kernel_launches;
  int64_t nlist_entries_all;       /* pairs within rc+skin before the type-pair filter (0 if unknown) */
  /* HIP-event samples of the remaining per-step kernels of the last chem_run */
  double  integrate_kernel_ms;
  int64_t integrate_kernel_launches;
  double  bonded_kernel_ms;
  int64_t bonded_kernel_launches;
  /* list builds actually performed (`rebuilds` above counts the reference rule on the workload's skin; with a wider internal
   * list skin -- option list_skin -- the lists are rebuilt less often) */
  int64_t list_rebuilds;
} chem_timers;

/* ---- life cycle ---------------------------------------------------------------------- */
/* espressopp.System() + esutil.RNG + storage (start_simulation.py:148-163) */
chem_ctx*   chem_create(int device_id, int precision);
void        chem_destroy(chem_ctx* ctx);
const char* chem_last_error(chem_ctx* ctx);      /* ctx may be NULL: last create error */
int         chem_abi_version(void);

/* ---- system set-up ------------------------------------------------------------------- */
/* bc.OrthorhombicBC(rng, box)  start_simulation.py:162 */
int chem_set_box(chem_ctx* ctx, const double L[3]);
/* VerletList(system, cutoff=max_cutoff, ...) + system.skin  start_simulation.py:151,193-197 */
int chem_set_cutoff(chem_ctx* ctx, double max_cutoff, double skin);
/* integrator.dt = dt  start_simulation.py:166 */
int chem_set_dt(chem_ctx* ctx, double dt);
/* storage.addParticles(particle_list,'id','type','pos','mass','q','res_id','state',..)
 * + decompose()  start_simulation.py:169-171, gromacs_topology.py:1418-1441.
 * vel may be NULL (zeros); q, state, res_id may be NULL (0 / 0 / id).
 *
 * Particle ids: any distinct int64 values, in any row order.  Inside, a particle is its TAG, the rank of its id among all ids
 * (chem_add_particles appends: its ids lie above the present ones); ids exist at this boundary only, and every call that takes
 * an id refuses one that no particle carries with CHEM_EINVAL and leaves the context as it was (a list of ids is resolved
 * completely before anything is changed).  Random streams are keyed by tag (chem_philox.h), so two contexts whose ids differ
 * but stand in the same order compute the same bits, whatever the row order.  Read-backs carry ids as int64.  Two int32 labels
 * are MADE of ids and exist only for ids that fit 32 bits: the default res_id (res_id == NULL with such an id is CHEM_EINVAL
 * here and in chem_add_particles: pass res_id) and CHEM_STATE_MOLID (chem_get_state answers CHEM_EINVAL for a context that
 * holds such an id; the mol_id the reaction rules read is a tag and is not affected). */
int chem_set_particles(chem_ctx* ctx, int64_t n, const int64_t* id, const int32_t* type,
                       const double* pos, const double* vel, const double* mass,
                       const double* q, const int32_t* state, const int32_t* res_id);
/* storage.modifyParticle(pid, 'type'|'state'|'mass', v)  examples/atrp_lj/hooks.py:63-65 */
int chem_modify_particle(chem_ctx* ctx, int64_t id, int what /*CHEM_STATE_TYPE|STATE|MASS|RESID|CHARGE|LAMBDA*/, double value);
/* DynamicExcludeList(integrator, gt.exclusions)  start_simulation.py:189 */
int chem_set_exclusions(chem_ctx* ctx, int64_t n, const int64_t* id_pairs);

/* ---- non-bonded ---------------------------------------------------------------------- */
/* interaction.LennardJones(epsilon, sigma, cutoff) via VerletListLennardJones.setPotential
 * gromacs_topology.py:715-721.  shift_auto!=0: U(rc)=0. */
int chem_nb_lj(chem_ctx* ctx, int t1, int t2, double eps, double sig, double rc, int shift_auto);
/* interaction.Tabulated(itype=1, filename, cutoff) via VerletListTabulated.setPotential
 * gromacs_topology.py:696-707; rows are the `r e f` lines of the .pot file
 * (tools/convert_gromacs2espp.py:84-107), uniform spacing dr starting at r0. */
int chem_nb_table(chem_ctx* ctx, int t1, int t2, int64_t nrow, double r0, double dr,
                  const double* e, const double* f, double rc);
/* Interpolation kinds of every tabulated potential (pairs, bonds, angles, dihedrals): the `itype` of
 * interaction.Tabulated / TabulatedAngular / TabulatedDihedral.  1 = linear (the calls without `_interp`), 2 = Akima,
 * 3 = natural cubic spline; anything else, and nrow < 4 for itype 2 and 3, is CHEM_EINVAL.  The arithmetic of the
 * reference's InterpolationAkima / InterpolationCubic is in the external fork, so this rule set is this build's own:
 *   - the e and the f column are interpolated independently (the force is the spline of f, not the derivative of the e spline);
 *   - per interval k = 0 .. nrow-2 and column: y(w) = c0 + w (c1 + w (c2 + w c3)), w = (x - x_k) / dr in [0, 1];
 *   - itype 2, Akima (1970): d_k = y_{k+1} - y_k, continued by d_-1 = 2 d_0 - d_1, d_-2 = 2 d_-1 - d_0,
 *     d_{n-1} = 2 d_{n-2} - d_{n-3}, d_n = 2 d_{n-1} - d_{n-2}; node slope per grid step
 *       t_k = (|d_{k+1} - d_k| d_{k-1} + |d_{k-1} - d_{k-2}| d_k) / s_k,  s_k = the sum of the two weights,
 *     and t_k = (d_{k-1} + d_k) / 2 where s_k <= 1e-9 max_j s_j (the tie rule of scipy's Akima1DInterpolator);
 *       c0 = y_k, c1 = t_k, c2 = 3 d_k - 2 t_k - t_{k+1}, c3 = t_k + t_{k+1} - 2 d_k;
 *   - itype 3: second derivatives (times dr^2) M_0 = M_{n-1} = 0, M_{k-1} + 4 M_k + M_{k+1} = 6 (y_{k+1} - 2 y_k + y_{k-1});
 *       c0 = y_k, c1 = d_k - (2 M_k + M_{k+1}) / 6, c2 = M_k / 2, c3 = (M_{k+1} - M_k) / 6;
 *   - evaluation as for the linear kind: t = (x - r0) / dr clamped to [0, nrow-1], k = min(int(t), nrow-2), w = t - k,
 *     Horner; beyond the grid the end rows' values hold.  Pairs: F_ij = f(r)/r * r_ij for r^2 <= rc^2, energy e(r) without
 *     a shift.  Bonds: f(r)/r.  Angles: U(theta), -dU/dtheta in radians.  Dihedrals: over [-pi, pi], not periodic.
 * A type pair may be re-sent with another kind (or as LJ) between two chem_run calls. */
int chem_nb_table_interp(chem_ctx* ctx, int t1, int t2, int64_t nrow, double r0, double dr,
                         const double* e, const double* f, double rc, int itype);

/* interaction.CoulombTruncated(prefactor, cutoff) via VerletListCoulombTruncated.setPotential(type1, type2, potential)
 * gromacs_topology.py:866-878 (prefactor = 138.935485 * fudgeQQ, one potQQ for every type pair).  Registers the term for
 * the type pair (symmetric); prefactor == 0 or rc <= 0 removes it.  All registered pairs must share one (prefactor, rc):
 * anything else is CHEM_ENOTIMPL.  The arithmetic of CoulombTruncated is in the external fork, so this rule set is this
 * build's own ([EXT-RECALL]).  With k = prefactor and rc_qq = rc, for every pair on the Verlet list that
 * is not excluded and has r^2 <= rc_qq^2 (inclusive, as LJ's r^2 <= rc^2):
 *     U = k q_i q_j / r,     F_i = k q_i q_j r_ij / r^3,     the energy is not shifted.
 *   - the term comes ON TOP of whatever LJ or table the type pair carries; a pair without either (sigma = 0) still gets it;
 *   - excluded pairs get nothing; type pairs that were not registered get nothing;
 *   - rc_qq may be smaller or larger than the pair's LJ / table cutoff, but not larger than max_cutoff: chem_run refuses
 *     that with CHEM_EINVAL naming the type pair;
 *   - charges are per particle (chem_set_particles `q`); a reaction (new_q_1/2, set wherever the reaction names a new type),
 *     neighbour rule, ATRP flip, dissociation or chem_modify_particle(CHEM_STATE_CHARGE) that changes a charge acts from the
 *     next force evaluation on;
 *   - while a pair is registered the force kernels are built for option tpp = 1 (or 0) and pair_block = 512 only: other
 *     values are CHEM_EINVAL at the next evaluation; harmonic bonds are not evaluated inline (option bonds_inline has no
 *     effect). */
int chem_nb_coulomb(chem_ctx* ctx, int t1, int t2, double prefactor, double rc);
/* Energy and sum over pairs of r.F of the Coulomb term, evaluated as chem_observe does (at the current positions; zeros while
 * no pair is registered).  Either pointer may be NULL.  chem_obs.epot_lj / epot_tab keep their meaning; chem_obs.virial_nb,
 * the sum over ALL non-bonded pairs, includes the Coulomb part. */
int chem_get_coulomb(chem_ctx* ctx, double* epot, double* virial);

/* ---- dynamic resolution: per-particle lambda ------------------------------------------ */
/* interaction.VerletListDynamicResolutionLennardJones / ...Tabulated(vl, cg_potential=False) (gromacs_topology.py:584-600,
 * 819-862: nonbond_params func 15 / 11), integrator.BasicDynamicResolution(system, {type: alpha}) with
 * add_postprocess(PostProcessChangeProperty) (reaction_setup.py:257-356) and the particle property lambda_adr.  The arithmetic
 * is in the external fork, so this rule set is this build's own ([EXT-RECALL], parity unpinned; DESIGN.md "Dynamic resolution").
 *
 * Every particle has a resolution lambda in [0, 1], 1 unless set.  Per particle (by tag) the host keeps a stamp (lambda0, s0);
 * with alpha(t) the rate registered for type t (0 if none) the resolution at step s is
 *     lambda(s) = min(1.0, lambda0 + alpha(type) * (double)(s - s0))        fp64, in this order, no fused multiply-add.
 * The forces that are current at step s use lambda(s) (the convention of chem_list_set_hybrid): lambda is a pure function of
 * the stamp, the type and the step -- no array that is updated per step --, the same on every rank and for run(a); run(b)
 * as for run(a+b).  A particle is re-stamped with (its current lambda, the current step) when its lambda is set explicitly,
 * when its type changes by any route (reaction, neighbour rule, ATRP, dissociation, chem_modify_particle, completion below)
 * and when the rate of its type is changed.  chem_set_particles puts every lambda back to 1.
 *
 * chem_nb_resolution marks (on != 0) or unmarks the LJ or table already registered for the symmetric type pair as
 * resolution-scaled.  For each listed pair of a marked type pair that is not excluded and lies inside that potential's cutoff:
 *   - w = lambda_i lambda_j; a pair with w == 0 contributes nothing and its potential is not evaluated;
 *   - F = w F_pot; if max_force > 0 and |F| > max_force, F is rescaled to |F| = max_force (the cap comes after the scaling);
 *   - the energy share is w U, uncapped, in chem_obs.epot_lj / epot_tab; the virial share is r.F of the force that was applied;
 *   - unmarked type pairs behave exactly as without this call, whatever lambda their particles have; a context without a
 *     marked pair launches the kernels it launched before and allocates nothing;
 *   - marking a type pair that carries no LJ or table is CHEM_EINVAL (the mark would have nothing to scale; a potential that
 *     is re-sent later keeps its mark; unmarking is always allowed);
 *   - the Coulomb term is never scaled, and a context does not serve a Coulomb pair and a marked pair together: the next
 *     force evaluation refuses that with CHEM_ENOTIMPL naming the marked pair;
 *   - the reference's cg_potential = True variant (weight 1 - w) is not built;
 *   - while a pair is marked the force kernels are built for option tpp = 1 (or 0) and pair_block = 512 only (CHEM_EINVAL at
 *     the next evaluation otherwise), and harmonic bonds are not evaluated inline, as for chem_nb_coulomb. */
int chem_nb_resolution(chem_ctx* ctx, int t1, int t2, int on, double max_force);
/* BasicDynamicResolution's {type: alpha} entry plus the PostProcessChangeProperty attached to it.  alpha <= 0 removes the
 * entry.  The rate applies to every particle of that type with lambda < 1.  new_type < 0: no property change; new_state < 0:
 * the chemical state is kept.  Completion: let s_full be the first step at which the expression above evaluates to >= 1.0.
 * When the step counter reaches s_full a particle of a type with a registered change gets new_type, new_mass, new_q and
 * new_state by the route of chem_modify_particle; its lambda stays 1 (stamp (1, s_full) under the new type, so a rate of the
 * new type does nothing more).  chem_run splits at these steps as it splits at reaction steps -- the host knows every stamp,
 * so it knows every s_full: no device-side polling, no host round trip per step -- and evaluates the forces again after the
 * change, so the forces current at s_full (chem_get_state(CHEM_STATE_FORCE), the first half kick of the next step) are those
 * of the new properties; the half kick that ended the step into s_full was the last with the old ones.  A reaction of the
 * same step acts first.  On slabs the change goes as far as chem_modify_particle does there.  Call it after
 * chem_set_particles (CHEM_ESTATE otherwise). */
int chem_resolution_rate(chem_ctx* ctx, int type, double alpha, int new_type, double new_mass, double new_q, int new_state);
/* lambda_adr of addParticles / modifyParticle: lambda of the n particles `ids`, stamped at the current step.  A value outside
 * [0, 1] or non-finite, and an unknown id, are CHEM_EINVAL (nothing is set then).  The same on every rank of a decomposition.
 * CHEM_STATE_LAMBDA reads lambda at the current step back (chem_get_state: the fp64 host expression) and sets one particle's
 * (chem_modify_particle). */
int chem_set_resolution(chem_ctx* ctx, int64_t n, const int64_t* ids, const double* lambda);
/* TopologyParticleProperties(lambda_adr=...) of the PostProcessChangeProperty of a Reaction / DissociationReaction
 * (reaction_setup.py:300-330): on every event of `reaction` (an index of chem_reaction_add or chem_dissociation_add) the
 * particle in `role` (1 | 2) is stamped (lambda, event step), after the reaction's own state and type changes and after the
 * re-stamping those cause.  A negative lambda removes the rule.  CHEM_EINVAL: unknown index, role other than 1 or 2,
 * lambda > 1.  Not on the decomposed path (CHEM_ENOTIMPL here after chem_comm_init*, and in chem_comm_init* after this call).
 * While a rule or a rate exists, a reaction step waits for its own host bookkeeping before the next MD step is enqueued, and
 * chem_run also ends its pieces at every reaction and ATRP step (a stamp set there may create a completion step).  Rules
 * are keyed by the reaction index and live as long as the reaction does: reactions are never removed from a context, and
 * chem_set_particles keeps reactions and rules alike. */
int chem_reaction_set_resolution(chem_ctx* ctx, int reaction, int role, double lambda);

/* ---- capped pair potentials ------------------------------------------------------------ */
/* interaction.TabulatedCapped(itype, filename, cutoff, caprad) via VerletListTabulatedCapped, and LennardJonesCapped(epsilon,
 * sigma, cutoff, caprad, shift) via VerletListLennardJonesCapped (gromacs_topology.py:619-621, 684-695, 895-897: nonbond_params
 * func 13, label lj-tab_cap; put on the type pairs that react, so that two reactive beads can approach to the reaction cutoff
 * without the steep core throwing them apart).  The arithmetic is in the external fork, so this rule set is this build's own
 * ([EXT-RECALL], parity unpinned; DESIGN.md "Capped pairs").
 *
 * chem_nb_cap marks the LJ or table already registered for the symmetric type pair as capped at c = caprad; caprad <= 0
 * removes the mark.  A potential that is re-sent later keeps its mark.  For every listed, non-excluded pair of a capped type
 * pair with r^2 <= rc^2 (rc: that potential's cutoff):
 *   - r_e = c if r^2 < c^2, else r: the decision is taken on the squares;
 *   - F_i = (f(r_e) / r) r_ij, with f the potential's force magnitude: the interpolated force column for a table of any
 *     itype, f(r) = 24 eps (2 (sigma/r)^12 - (sigma/r)^6) / r for LJ.  Inside the cap the force keeps the magnitude f(c) and
 *     the direction of r_ij;
 *   - the energy share is U(r_e), plus the LJ shift where the pair has one: constant inside the cap, in chem_obs.epot_tab /
 *     epot_lj; the virial share is r.F of the force that was applied, f(c) r inside the cap;
 *   - at r = 0 the force is exactly zero and finite (no NaN, no Inf), the energy is U(c);
 *   - force and energy are continuous at r = c, so two precisions (or two ranks) that disagree on which side of c a pair lies
 *     agree on what it contributes to within their rounding: no pair has to be set aside at the cap radius when results are
 *     compared, unlike at the cutoff, where the force jumps;
 *   - inside the cap the energy does not integrate the force (U is constant, F is not zero): a trajectory with overlapping
 *     capped pairs does not conserve the total energy in NVE;
 *   - uncapped type pairs behave exactly as without this call; a context without a capped pair launches the kernels it
 *     launched before and allocates nothing;
 *   - a type change by any route (reaction, neighbour rule, chem_modify_particle, resolution completion) moves a pair between
 *     capped and uncapped type pairs from the next force evaluation on.
 * CHEM_EINVAL: the type pair carries no LJ or table; caprad is non-finite; caprad >= rc of that potential (if a re-sent
 * potential's rc no longer exceeds the radius, the next chem_run refuses with CHEM_EINVAL naming the pair); the type pair is
 * also resolution-marked -- chem_nb_resolution on a capped pair is refused likewise.  Capped pairs and resolution-marked
 * pairs on DIFFERENT type pairs are served together.  A context does not serve a Coulomb pair and a capped pair together:
 * the next force evaluation refuses that with CHEM_ENOTIMPL naming the capped pair.  While a pair is capped the force
 * kernels are built for option tpp = 1 (or 0) and pair_block = 512 only (CHEM_EINVAL at the next evaluation otherwise), and
 * harmonic bonds are not evaluated inline, as for chem_nb_coulomb.  Caps are type-pair data: the same call on every rank of a
 * decomposition. */
int chem_nb_cap(chem_ctx* ctx, int t1, int t2, double caprad);

/* ---- fixed distances: by-product release (FixDistances, ReleaseMolecule) --------------- */
/* integrator.FixDistances(system, fix_list[, anchor_type, target_type]) + add_postprocess(PostProcessChangeProperty),
 * integrator.PostProcessReleaseParticles(fd, count) on a Reaction, analysis.NumFixDistances, and storage.addParticles after
 * the first upload -- reaction_post_process.py:203-320 (ext_type=ReleaseMolecule): dummy particles ride at a fixed distance
 * from a host particle until a reaction of the host, or a type change, sets them free as a small molecule that fades in
 * through the resolution lambda.  The arithmetic of FixDistances is in the external fork, so this rule set is this build's own
 * ([EXT-RECALL], parity unpinned; DESIGN.md "Fixed distances").
 *
 * A set holds entries (anchor a, target t, distance d) in insertion order.
 * Per step: behind every drift (the first half kick + drift of velocity Verlet), exactly once per drift and before anything
 * reads the new positions (rebuild decision, forces), for every live entry:
 *     u = minimum image of x_t - x_a, both after the drift (the target drifts like any particle, with the velocity it carries);
 *     u = (1, 0, 0) if |u| = 0, else u / |u|;
 *     x_t <- x_a + d u, applied as the displacement (d u - (x_t - x_a)) through the drift's own position update (fixed-point
 *            add in the CHEM_PREC_F32 build), so folding, image counters and CHEM_STATE_POS_UNFOLDED go on as for any particle;
 *     v_t <- v_a, the anchor's half-step velocity at that moment.
 * Nothing else is special about a target: it takes the second half kick with its own force and mass, counts in ekin,
 * temperature and momentum, and is thermalised or not according to chem_thermostat_langevin_types.  The constraint's move
 * does not enter the displacement maximum of the rebuild criterion.  After a run that the device stopped and the host resumed
 * the positions of that step are drifted and constrained already: the rule is not applied again there.
 * Release: the entry is removed; the post-process of its set whose old_type is the target's current type (if any) is applied
 * by the route of chem_modify_particle (type, mass, charge, state, and the stamp (lambda, release step) as
 * chem_reaction_set_resolution sets one); the lists are rebuilt before the next force evaluation.  From the next drift on the
 * target is an ordinary particle; it keeps the velocity it had.
 *   by a reaction  (chem_reaction_release) in the reaction step, after the step's bonds and type changes: for every
 *       bond-forming event of a reaction with a release rule, events in the order chem_get_events reports them, role 1 before
 *       role 2, rules in the order they were added: up to `count` live entries of the rule's set whose anchor is that reactant,
 *       lowest insertion index first; fewer if fewer remain.  Cause 1.
 *   by type  (sets created with types; -1 asks nothing of that side): an entry leaves when type(anchor) != anchor_type or
 *       type(target) != target_type.  Types change only at host-visible points, so the check runs behind the release by
 *       reaction, behind the ATRP step, behind the resolution completions and at the start of chem_run (chem_modify_particle):
 *       indistinguishable from a check on every step.  The record carries the current step.  Cause 2.
 * While a release rule or a typed set with entries exists, chem_run ends its pieces at every reaction and ATRP step, and a
 * reaction step waits for its own host bookkeeping (as for chem_reaction_set_resolution).
 * Not on the decomposed path (anchor and target may sit on different ranks): chem_fix_add after chem_comm_init*, and
 * chem_comm_init* with entries present, are CHEM_ENOTIMPL. */
#define CHEM_MAX_FIX_SETS 8
typedef struct chem_fix_record {
  int64_t step;
  int64_t anchor_id, target_id;
  int32_t set;
  int32_t cause;            /* chem_fix_log: 1 = reaction, 2 = type condition; chem_fix_joins: 3 = joined, 4 = refused */
} chem_fix_record;
/* storage.addParticles after the particle set exists: appends n particles.  Every new id must be greater than the largest
 * present id (CHEM_EINVAL otherwise; ids within the call in any order, no duplicates): id order stays tag order and existing
 * tags do not move.  Allowed only while chem_get_step() == 0 and before the first chem_run (CHEM_ESTATE later, and before
 * chem_set_particles).  Exclusions, bonded lists, the bond graph, lambda stamps (new particles: lambda 1), reactions and rates
 * are kept -- chem_set_particles would clear them.  A type at or above CHEM_MAX_TYPES is CHEM_EINVAL naming the limit.  Pointer
 * conventions of chem_set_particles.  Not after chem_comm_init* (CHEM_ENOTIMPL). */
int chem_add_particles(chem_ctx* ctx, int64_t n, const int64_t* id, const int32_t* type, const double* pos, const double* vel,
                       const double* mass, const double* q, const int32_t* state, const int32_t* res_id);
/* FixDistances(system, fix_list, anchor_type, target_type): a new, empty set; (-1, -1): no type condition.  Returns the handle;
 * more than CHEM_MAX_FIX_SETS sets: CHEM_ENOSPC. */
int chem_fix_create(chem_ctx* ctx, int anchor_type, int target_type);
/* fd.add_triplet(anchor, target, dist): ids = n (anchor, target) pairs.  CHEM_EINVAL (nothing is added then): dist not positive
 * and finite, an unknown id, anchor == target, a target that already is the target of a live entry of any set, a target that
 * is an anchor, an anchor that is a target.  An anchor may carry any number of entries.  Allowed between chem_run calls. */
int chem_fix_add(chem_ctx* ctx, int set, int64_t n, const int64_t* ids, double dist);
/* fd.add_postprocess(PostProcessChangeProperty): what becomes of a released target whose type is old_type at the release.
 * new_type < 0: no property change; new_state < 0: the chemical state is kept (conventions of chem_resolution_rate);
 * lambda in [0, 1]: stamp (lambda, release step); lambda < 0: the resolution is left alone; lambda > 1: CHEM_EINVAL.  A second
 * call for one old_type replaces the first. */
int chem_fix_postprocess(chem_ctx* ctx, int set, int old_type, int new_type, double new_mass, double new_q, int new_state, double lambda);
/* reaction.add_postprocess(PostProcessReleaseParticles(fd, count), 'type_1' | 'type_2'): role 1 | 2 ('both': two calls) of the
 * association reaction `reaction` (index of chem_reaction_add) releases `count` >= 1 entries of `set` per event. */
int chem_reaction_release(chem_ctx* ctx, int reaction, int role, int set, int count);
/* analysis.NumFixDistances: the number of live entries */
int64_t chem_fix_count(chem_ctx* ctx, int set);
/* fd.get_all_triplets(): the live entries in insertion order, ids[2k] = anchor, ids[2k+1] = target, dist[k]; either pointer
 * may be NULL.  Returns the count (ids == dist == NULL: the count alone). */
int64_t chem_fix_get(chem_ctx* ctx, int set, int64_t* ids, double* dist, int64_t cap);
/* the release records since the context was created, ordered by (step, set, insertion index); out == NULL: the count.
 * (chem_set_particles empties every set and the log -- tags are new --; sets, post-processes and release rules stay.) */
int64_t chem_fix_log(chem_ctx* ctx, chem_fix_record* out, int64_t cap);

/* ---- reverse reactions: bond removal and join by a reaction (RemoveNeighboursBonds, JoinMolecule) ---------------- */
/* integrator.PostProcessRemoveNeighbourBond(tm).add_bond_to_remove(anchor_type, nb_level, t1, t2) and
 * integrator.PostProcessJoinParticles(fd, eq_length), each with reaction.add_postprocess(pp, invoke_on) --
 * reaction_post_process.py:117-137, 322-362 (ext_type=RemoveNeighboursBonds / JoinMolecule; examples/dacron/rev_with_water:
 * the hydrolysis  C(0,1):E(0,1) + W(0,2) -> A(1):Z(1) + E(1)  takes the ester bond out again and attaches the consumed water
 * to the regenerated acid group as a dummy, ready to be released by the next condensation).  The arithmetic of both is in the
 * external fork, so these rule sets are this build's own ([EXT-RECALL], parity unpinned; DESIGN.md "Reverse reactions").
 * Both act on the events of association reactions (chem_reaction_add, virtual ones included) in the reaction step, in this
 * order: association events, neighbour changes (chem_reaction_neighbour_change), REMOVALS, JOINS, ATRP step, lambda rules
 * (chem_reaction_set_resolution), release by reaction, release by type.
 *
 * chem_reaction_remove_bond
 *   order       events of `reaction` in canonical order (min id, max id); role 1 before role 2; rules in the order they were
 *               added; within one visit the bonds by (id p, id q).
 *   roles       a role is visited only if invoke_on (1 | 2 | 3 = both) includes it and the reaction's own type for that role
 *               (chem_reaction_desc.type_1 / type_2: the reactant's type before the event) equals anchor_type.
 *   bonds       from the anchor, every bond (p, q) of the bond graph as it stands after this step's new bonds (and before any
 *               removal of this step) with graph distance d(anchor, p) = nb_level - 1 and d(anchor, q) = nb_level; it is
 *               removed when the unordered pair {type p, type q} equals {type_1, type_2}, with the types at the START of this
 *               step's association phase: after the dissociation block, before any association event, role change or
 *               neighbour change of the step (an E that the same step turns into something else still matches C:E).
 *   effect      what the `apply` of a dissociation (chem_dissociation_desc) does to a broken pair, except that the pair leaves
 *               EVERY arity-2 list that holds it (order of the survivors kept): it leaves the bond graph, mol_id of the
 *               fragments is recomputed, res_id stays, unexclude != 0 lifts the 1-2 exclusion, triples and quadruples that
 *               hold p, q as consecutive members go; the 1-3 / 1-4 exclusions those once caused stay (the same known limit).
 *               No state or type changes: those are the reaction's own.
 *   duplicates  a bond found by two visits is removed once and recorded for the first.
 *   log         chem_reaction_removed: one record per (bond, list), ordered by step, then by visit order, then by list handle;
 *               id_near = p, id_far = q; `reaction` is the public index.  out == NULL: the count.  chem_set_particles empties it.
 *   afterwards  the lists are rebuilt before the next force evaluation (the table rebuild of a dissociation step).
 * CHEM_EINVAL: rule == NULL, not an index of chem_reaction_add, invoke_on outside 1..3, nb_level < 1, a type outside
 * [0, CHEM_MAX_TYPES).  A context without a rule launches exactly what it launched before. */
typedef struct chem_nb_remove {
  int32_t reaction, invoke_on, anchor_type, nb_level;
  int32_t type_1, type_2, unexclude, pad;
} chem_nb_remove;
typedef struct chem_bond_record {
  int64_t step;
  int64_t id_near, id_far;
  int32_t list, reaction;
} chem_bond_record;
int chem_reaction_remove_bond(chem_ctx* ctx, const chem_nb_remove* rule);
int64_t chem_reaction_removed(chem_ctx* ctx, chem_bond_record* out, int64_t cap);
/* chem_reaction_join: on every event of `reaction` the reactant in `role` (1 | 2) becomes the anchor and the other reactant
 * the target of a new entry (anchor, target, dist) of `set`; insertion order continues.
 *   order       events in canonical order, rules in the order they were added.
 *   refusals    a pair chem_fix_add would refuse (a target that already is a target or an anchor, an anchor that is a target)
 *               adds nothing and is recorded with cause 4.
 *   placement   at once, on the device, over this step's new entries only, by the arithmetic of the per-step rule above:
 *               u = minimum image of x_t - x_a, (1, 0, 0) for |u| = 0; x_t <- x_a + d u / |u| through the drift's position
 *               update; v_t <- v_a.  The lists are then rebuilt before the next force evaluation: the rebuild bins the target
 *               where it is, and the jump never meets the displacement criterion.
 *   afterwards  the release by reaction and the type check of the same step see the entry: a set created with types judges it
 *               with the types the step has just given.
 *   log         chem_fix_joins: cause 3 = joined, 4 = refused, in visit order.  chem_fix_log keeps its meaning (releases only).
 * While a join rule exists chem_run ends its pieces at every reaction step, as for release rules.
 * CHEM_EINVAL: not an index of chem_reaction_add, role other than 1 or 2, unknown set, dist not positive and finite.
 * Neither call is available on the decomposed path: CHEM_ENOTIMPL after chem_comm_init*, and in chem_comm_init* after either. */
int chem_reaction_join(chem_ctx* ctx, int reaction, int role, int set, double dist);
int64_t chem_fix_joins(chem_ctx* ctx, chem_fix_record* out, int64_t cap);

/* ---- bonded lists -------------------------------------------------------------------- */
/* FixedPairList/TripleList/QuadrupleList(storage) + FixedXListYyy(system, list, potential)
 * gromacs_topology.py:949-961,1086-1096,1206-1224; reaction_setup.py:444-467.
 * by_types!=0 -> the "Types" variant: parameters selected per entry from the CURRENT
 * particle types (gromacs_topology.py:969-981).  Returns the list handle. */
int chem_list_create(chem_ctx* ctx, int arity, int potential_kind, int by_types);
/* interaction.Tabulated(itype=1, filename=table_b<N>.pot) for bonds, `[ bonds ]`/`[ bondtypes ]` func 8
 * gromacs_topology.py:919-925,953,961: rows `r e f` on a uniform grid (tools/convert_gromacs2espp.py), linear
 * interpolation of e(r) and f(r), F_ij = f(r)/r * r_ij, first/last row beyond the grid.  Returns a table
 * handle >= 0 that is passed as the single parameter of a CHEM_POT_TABULATED list (plain or per type pair).
 * The same registry serves interaction.TabulatedAngular (angles func 8, table_a<N>.pot, gromacs_topology.py:1074-1080):
 * grid in radians, columns U(theta) and -dU/dtheta, list kind CHEM_POT_ANG_TABULATED; and interaction.TabulatedDihedral
 * (dihedrals func 8, table_d<N>.pot, gromacs_topology.py:1192-1198): grid over [-pi, pi], kind CHEM_POT_DIH_TABULATED. */
int chem_table_create(chem_ctx* ctx, int64_t nrow, double r0, double dr, const double* e, const double* f);
/* The same with an interpolation kind (see chem_nb_table_interp); itype = 1 is chem_table_create. */
int chem_table_create_interp(chem_ctx* ctx, int64_t nrow, double r0, double dr, const double* e, const double* f, int itype);
/* addBonds/addTriples/addQuadruples: ids is n*arity particle ids */
int chem_list_add(chem_ctx* ctx, int list, int64_t n, const int64_t* ids);
/* plain list: t1..t4 ignored (pass -1); Types list: setPotential(type1,type2[,type3[,type4]],pot) */
int chem_list_set_params(chem_ctx* ctx, int list, int t1, int t2, int t3, int t4,
                         const double* p, int np);
/* getAllBonds/getAllTriples/getAllQuadruples: out receives count*arity ids */
int64_t chem_get_list(chem_ctx* ctx, int list, int64_t* out, int64_t cap_entries);
/* FixedPairListLambda(storage, init_lambda) + integrator.FixedListDynamicResolution.register_pair_list(fpl, rate)
 * reaction_setup.py:444-467, start_simulation.py:289-293: a HYBRID pair list.  Every entry remembers its birth step -- the
 * value of chem_get_step() when it was added, by a reaction, by chem_list_add or otherwise -- and the forces that are
 * current at step s (those chem_get_state(CHEM_STATE_FORCE) shows, those the step from s to s+1 starts with) use, per entry,
 *     lambda = min(1, lambda0 + rate * (s - birth)):
 * the entry's force is lambda F, its share of chem_obs.epot_list is lambda U.  lambda is a pure function of the two step
 * numbers (no array that is updated per step), so it is the same on every rank and for run(a); run(b) as for run(a+b).
 * The pair is excluded from the non-bonded terms as soon as the bond exists, whatever its lambda; angles and dihedrals
 * spawned around it act at full strength unless their list is hybrid too (chem_list_set_hybrid_tuples); a dissociation reaction removes the birth step with the entry, a pair that
 * bonds again starts at lambda0.  Any pair kind, plain or by types.  Harmonic bonds of a context that has a hybrid list
 * are not evaluated inline (option bonds_inline has no effect).  (Parity unpinned: DESIGN.md "Hybrid bonds".)
 * CHEM_EINVAL: list of arity != 2, lambda0 outside [0, 1], rate < 0, a non-finite value; CHEM_ESTATE: the list already
 * has entries (calling it again on an empty list, e.g. to set the rate later, is allowed). */
int chem_list_set_hybrid(chem_ctx* ctx, int list, double lambda0, double rate);
/* FixedTripleListLambda / FixedQuadrupleListLambda(storage, init_lambda) + FixedListDynamicResolution.register_triple_list /
 * register_quadruple_list(list, rate), app_args.py:206-209 (--t_hybrid_angle, --t_hybrid_dihedral): a HYBRID triple or
 * quadruple list, for the angles and dihedrals the topology manager spawns around a new bond (chem_topology_register).
 * (Parity unpinned, as for hybrid bonds: the rule set below is this build's own; DESIGN.md "Hybrid bonds".)
 *   - Arity 3 or 4 only; a pair list is CHEM_EINVAL (it is chem_list_set_hybrid's, which in turn refuses these lists).
 *   - lambda0 outside [0, 1], rate < 0, a non-finite value, an unknown handle: CHEM_EINVAL.  A list that already has entries:
 *     CHEM_ESTATE (their birth steps are unknown); calling it again on an empty list is allowed.
 *   - Any angle or dihedral kind, plain or by types.
 *   - Every entry remembers its birth step, the value of chem_get_step() when it was added: spawned in a reaction step, by
 *     chem_list_add or by any other path that appends.
 *   - The forces that are current at step s use, per entry, lambda = min(1, lambda0 + rate * (s - birth)), the expression of
 *     chem_list_set_hybrid: the entry's force on every member is lambda F, its share of chem_obs.epot_list lambda U, its
 *     contribution to the list virial of chem_get_pressure and to the list part of chem_get_pressure_tensor lambda times the
 *     plain one.
 *   - lambda is a pure function of the two step numbers: no kernel updates it and no array holds it, run(a); run(b) equals
 *     run(a+b) bit for bit, every rank of a slab run computes the same value (the host topology is replicated, births are
 *     global step numbers).
 *   - An entry whose lambda is exactly 0 is skipped, not multiplied: a tuple spawned in a geometry where the full term is not
 *     finite contributes exactly nothing.
 *   - The 1-3 / 1-4 exclusion of a spawned tuple acts from the moment it is inserted, whatever lambda.
 *   - Whatever removes a bond (a dissociation, chem_reaction_remove_bond) takes the birth step away with every tuple it
 *     removes; the survivors keep theirs; a tuple spawned again after the pair bonds again starts at lambda0.
 *   - chem_list_get_lambda serves these lists; a checkpoint carries their birth steps (same format version). */
int chem_list_set_hybrid_tuples(chem_ctx* ctx, int list, double lambda0, double rate);
/* analysis.ResolutionFixedPairList / ResolutionFixedTripleList / ResolutionFixedQuadrupleList (start_simulation.py:495-498):
 * lambda of every entry at the current step, in the order
 * of chem_get_list (same count convention); 1.0 for every entry of a list that is not hybrid. */
int64_t chem_list_get_lambda(chem_ctx* ctx, int list, double* out, int64_t cap_entries);

/* ---- thermostat ---------------------------------------------------------------------- */
/* integrator.LangevinThermostat: .temperature (=T*kb), .gamma  start_simulation.py:330-336.
 * gamma<=0 or kT<0 switches it off (thermostat=no, Q6 in SURVEY). */
int chem_thermostat_langevin(chem_ctx* ctx, double kT, double gamma, uint64_t seed);
/* LangevinThermostat.add_valid_types(thermal_groups)  start_simulation.py:312-336: friction and noise act only on
 * particles whose CURRENT type is listed (types change through reactions); n = 0 restores "every type" (the
 * reference passes an empty list when neither --thermal_groups nor --table_groups is given). */
int chem_thermostat_langevin_types(chem_ctx* ctx, int n, const int32_t* types);
/* integrator.BerendsenThermostat(system) (.temperature, .tau) and integrator.Isokinetic(system) (.temperature,
 * .coupling) -- start_simulation.py:341-348 (`thermostat = br | iso`): velocity rescaling after the second half
 * kick of a step (aftIntV).  With kT_now = 2 Ekin / (3 N):
 *   kind 1 Berendsen : v *= sqrt(1 + dt/tau * (kT/kT_now - 1)) every step            (param = tau)
 *   kind 2 Isokinetic: v *= sqrt(kT/kT_now) every `param` steps                       (param = coupling, >= 1)
 *   kind 0 switches it off.  Independent of chem_thermostat_langevin (the driver uses one of them). */
int chem_thermostat_rescale(chem_ctx* ctx, int kind, double kT, double param);
/* integrator.StochasticVelocityRescaling(system) (.temperature, .coupling) -- start_simulation.py:337-340
 * (`thermostat = vr`): every step after the second half kick, v *= sqrt(K_new / K) with K_new drawn from the
 * canonical kinetic-energy distribution relaxing with time constant `coupling` (Bussi-Donadio-Parrinello 2007;
 * 3 N degrees of freedom; stream keyed (seed, step), include/chem_philox.h svr_lambda).  coupling <= 0 switches it
 * off.  Shares the slot of chem_thermostat_rescale (the last call of either wins). */
int chem_thermostat_svr(chem_ctx* ctx, double kT, double coupling, uint64_t seed);
/* integrator.CapForce(system, max_force), added before the thermostat -- start_simulation.py:320-324
 * (`max_force`, app_args default -1 = off): after every force evaluation the conservative force of a
 * particle is rescaled to |f| = max_force where it exceeds it; the thermostat's friction and noise come
 * on top, uncapped (extension order).  max_force <= 0 switches it off. */
int chem_cap_force(chem_ctx* ctx, double max_force);

/* ---- pressure and barostat (NPT) ------------------------------------------------------- */
/* analysis.Pressure(system).compute() and integrator.BerendsenBarostat(system, pressure) with .tau / .pressure --
 * start_simulation.py:356-376, 466-469.  The arithmetic is in the external fork, so this rule set is this build's own
 * ([EXT-RECALL], parity unpinned; DESIGN.md "Pressure and barostat").
 *
 * Pressure:  P = (sum_i m_i v_i^2 + W) / (3 V),  V = Lx Ly Lz, in the engine's units, over all particles (dummies included).
 * W = sum r.F over every registered interaction:
 *   - non-bonded: exactly chem_obs.virial_nb (LJ, tables, Coulomb, capped and lambda-weighted terms, each with the force that
 *     was applied);
 *   - pair lists: r_ij . F_ij of every entry, one list at a time (harmonic, FENE, FENE+LJ, tabulated, 1-4 LJ, 1-4 Coulomb),
 *     a hybrid list's entries times their lambda; member 0 of an entry contributes it once, so it is right on slabs;
 *   - triple and quadruple lists depend on angles only: their virial vanishes identically under uniform scaling and is
 *     reported as exactly 0 (it is not evaluated).
 * Not in W: thermostat friction and noise, the clipping of chem_cap_force, the chem_fix_* constraint.
 * Same preconditions as chem_observe; works on slabs (the sums join the all-reduce). */
typedef struct chem_pressure {
  double pressure;
  double volume;
  double mv2;                          /* sum_i m_i v_i^2 */
  double virial_nb;                    /* == chem_obs.virial_nb */
  double virial_list[CHEM_MAX_LISTS];
  double virial;                       /* W = virial_nb + sum of virial_list */
} chem_pressure;
int chem_get_pressure(chem_ctx* ctx, chem_pressure* out);
/* Pressure tensor: analysis.PressureTensor(system).compute().  This build's own rule set, as the pressure above.
 *     Pi_ab = (K_ab + W_ab) / V,   six components in the order xx, yy, zz, xy, xz, yz  (every array [6] below).
 * K_ab = sum_i m_i v_i,a v_i,b over all particles, dummies included, with the mass the device integrates with.
 * W_ab = sum d_a F_b (a <= b) over the interactions of the scalar W, with the same forces and the same weights: the Coulomb
 * term, capped pairs with the force that was applied, lambda-weighted and force-capped resolution pairs, hybrid lists times
 * lambda, 1-4 Coulomb lists; a pair between two slabs is counted once.
 *   - a non-bonded pair or an entry of a pair list: d = the minimum-image vector the force law itself uses, F = the force on
 *     the first member;
 *   - triples and quadruples ARE evaluated (their trace vanishes, their components do not):
 *       triple (i, j, k), centre j:   d_ij (x) F_i + d_kj (x) F_k;
 *       quadruple (i, j, k, l):       d_ij (x) F_i + d_kj (x) F_k + (d_kj + d_lk) (x) F_l;
 *     the d are the minimum-image differences the bonded term forms; the entry is counted once, at member 0, as its energy is.
 *     The bending term of this pass is the force kernels' law in a form that keeps its digits next to a straight or folded
 *     angle (r1 x r2 by compensated products, the angle from atan2, the forces as double cross products); the force kernels'
 *     own form is off by about 1e-10 of a list's d (x) F at 1e-5 off folded, see DESIGN.md.
 * Not in W, as in the scalar: thermostat friction and noise, the clipping of chem_cap_force, the chem_fix_* constraint.
 * (K_xx + K_yy + K_zz = chem_pressure.mv2 and W_xx + W_yy + W_zz = chem_pressure.virial to rounding, part by part.)
 * Preconditions and side effects are those of chem_get_pressure and no others (the chem_observe route; a list build where the
 * skin is used up); works on slabs, every rank returns the global value.  The non-bonded part is a pass of its own over the
 * lists the step's forces used; which kernel runs is chem_tensor_host.hpp's rule, which refuses what the force launch refuses.
 * A context that never calls this allocates and launches nothing for it. */
typedef struct chem_pressure_tensor {
  double volume;
  double kinetic[6];
  double virial_nb[6];
  double virial_list[CHEM_MAX_LISTS][6];
  double virial[6];                    /* virial_nb + sum of virial_list */
  double tensor[6];                    /* (kinetic + virial) / volume */
} chem_pressure_tensor;
int chem_get_pressure_tensor(chem_ctx* ctx, chem_pressure_tensor* out);
/* Berendsen barostat, isotropic, on every step at the reference's aftIntV point: after the second half kick of step s and
 * after a velocity-rescale thermostat (if any), before the reaction, dissociation or ATRP work of that step.
 *     mu = [1 - (dt / tau) (P0 - P)]^(1/3),   P from x(t+dt), v(t+dt) and the virial of the step's own force evaluation;
 *     L <- mu L,  x <- mu x about the origin for every particle (dummies and the unfolded image bookkeeping scale too:
 *     CHEM_STATE_POS_UNFOLDED = pos + image * L).
 * Velocities and forces are not touched: the next half kick uses the forces evaluated before the scaling, also when it is the
 * first of the next chem_run (run(a); run(b) is run(a + b)), unless the system was changed or observed in between in a way
 * that re-sorts the particles (then the forces are evaluated again at the scaled positions).
 * mu^3 <= 0 stops chem_run with CHEM_ESTATE "Berendsen barostat: ..."; there is no clamp.  tau <= 0 switches it off: the
 * context then enqueues exactly the launches it enqueued before.  While it is on: the host waits for the device on every step (to read mu from
 * pinned memory, the box travels to the kernels by value; on the fused path also to look for a stop by the device; and in a
 * list build that the scalings ask for), the fused integrate and the skip_idle shortcut are off, the virial comes from a second
 * pair pass (the energy instantiation, over the lists the step's forces used).  The lists outlive a scaling: every scaling is
 * charged |mu - 1| (rc + skin_eff) / 2 (+ |mu - 1| skin_eff / 2 for the distance already accumulated) as displacement wherever
 * the rebuild criterion accumulates, under both rebuild_criterion values, and what the device keeps in absolute length
 * (reference positions, tile descriptors) follows mu.  After a scaling
 * cell_grid(L, rc + skin_eff) is compared with the grid in force; if they differ, in either direction, the geometry is planned
 * again in front of a list build behind the next drift, so the cell counts are always those a fresh context would plan at that box (this can switch
 * between the tile path and the per-cell lists in the middle of a run).  Reaction cutoffs and fixed distances are absolute
 * lengths and do not scale.  The three box edges are multiplied by the same mu: their ratios hold to one rounding per step.
 * Not on the decomposed path, a gap of that path: the call is CHEM_ENOTIMPL after chem_comm_init*, and chem_run refuses a
 * context that was decomposed after the call. */
int chem_barostat_berendsen(chem_ctx* ctx, double pressure, double tau);
/* Langevin piston barostat, isotropic: integrator.LangevinBarostat(system, rng, kT) with .gammaP / .mass / .pressure --
 * start_simulation.py:361-367.  The arithmetic is in the external fork, so this rule set is this build's own ([EXT-RECALL],
 * parity unpinned): the Quigley-Probert / Hoover Langevin piston, discretised symmetrically so that it has a conserved quantity.
 * State: the piston momentum pe, a half-step quantity, 0 when the barostat is switched on.  Parameters: target P0, piston mass
 * W > 0, friction gammaP >= 0, kT >= 0, seed.  N_f = 3 n over all particles (dummies included, as in chem_get_pressure),
 * c = 1 + 3 / N_f.  One step, with eps_dot = pe / W, sv = exp(-c eps_dot dt / 2) and mu = exp(eps_dot dt), all three computed in
 * double at the end of the previous step:
 *   1. v <- sv v, then v <- v + dt f / 2m  (f: what the step starts with, thermostat force included);
 *   2. drift and box: x <- mu (x + dt v / sqrt(mu)), L <- mu L.  The displacement dt v / sqrt(mu) is what the rebuild criterion
 *      sees; the scaling by mu is charged to the lists exactly as a Berendsen scaling is, and reference positions, tile
 *      descriptors, the unfolded-image bookkeeping and the re-plan of the geometry follow as they do there.  In the fp32 build
 *      the positions are box fractions: the drift is in the old box, the box then becomes mu L.  Fixed distances are absolute
 *      lengths: they are restored behind the scaling;
 *   3. rebuild decision / list build, forces at the new x, L; thermalize;
 *   4. v <- v + dt f / 2m, then v <- sv v; then a velocity-rescale thermostat, if any;
 *   5. the piston's kick, at the reference's aftIntV point, in front of the reaction / dissociation / ATRP work:
 *        P = (sum m v^2 + W_vir) / 3V from the step's own x, v, L and virial,
 *        G = 3V (P - P0) + (3 / N_f) sum m v^2 - gammaP pe + sqrt(24 gammaP W kT / dt) (u - 1/2),   pe <- pe + dt G,
 *      u = u01(out[0]) of chem_philox::barostat_draw(seed, step), step = the number of the step just counted; then sv and mu of
 *      the next step.
 * With pe = 0, sv = mu = 1: the first step after switching on is the plain velocity-Verlet step.  The state between steps is
 * consistent (the forces read back are those at the positions and the box read back), and run(a); run(b) is run(a + b) bit for
 * bit when nothing touches the system in between.  With gammaP = 0 and no thermostat,
 *   H = sum m v^2 / 2 + U + P0 V + (pe + dt G / 2)^2 / 2W,  evaluated behind 4. with that step's G, is conserved to O(dt^2).
 * A pe, mu or sv that is not finite (or a mu of 0) stops chem_run with CHEM_ESTATE "Langevin barostat: ..." naming the step, P,
 * P0 and pe; there is no clamp.  mass <= 0 switches it off and resets pe: the context then enqueues exactly the launches it
 * enqueued before.  A call that only changes parameters while it is on keeps pe.  While it is on, what holds for the Berendsen
 * barostat holds: a host wait on every step, no fused integrate, no skip_idle shortcut, the virial from a second pair pass.
 * One barostat at a time: switching one on while the other is on is CHEM_EINVAL.  CHEM_ENOTIMPL on a decomposed context. */
int chem_barostat_langevin(chem_ctx* ctx, double pressure, double mass, double gammaP, double kT, uint64_t seed);
/* The barostat in force.  kind: 0 off, 1 Berendsen, 2 Langevin piston.  pressure_last: P of the last step's barostat action.
 * Langevin piston: momentum = pe, eps_dot = pe / W, mu_next and sv_next the factors of the next step (Berendsen: 0, 0, 1, 1). */
typedef struct chem_barostat_state {
  int kind;
  double pressure_last, momentum, eps_dot, mu_next, sv_next;
} chem_barostat_state;
int chem_barostat_state_get(chem_ctx* ctx, chem_barostat_state* out);
/* system.bc.boxL: the current box edges */
int chem_get_box(chem_ctx* ctx, double L[3]);

/* ---- reactions ----------------------------------------------------------------------- */
/* integrator.ChemicalReaction(system, vl, storage, tm, interval) + .nearest_mode
 * + .max_per_interval  reaction_setup.py:416-427
 * Capacity: a reaction step holds at most max(8 * N, 1024) candidates (N particles of the whole system; a candidate is a pair
 * and a reaction that passed every filter and its acceptance draw, before the one-event-per-particle resolve).  A step that
 * finds more fails chem_run with CHEM_ENOSPC "reaction candidate buffer overflow" and applies nothing; fewer events are never
 * reported instead.  The limit is on the total alone: where in the box the candidates sit does not matter (one rank of a
 * decomposition: the candidates it finds, and the gathered total).
 * Labels: a bond-forming event joins two bonded clusters.  All bonds of the step are put into the bond graph first; then,
 * for the step's bonds (a, b) in (min id, max id) order, every particle of the cluster that now holds a and b gets
 * res_id = min(res_id[a], res_id[b]) as these two are at that moment (the residue id is transferred from the bond's own ends:
 * where several bonds of one step join one cluster, the first of them decides, and that need not be the lowest res_id in the
 * cluster) and mol_id = the lowest particle of the cluster (CHEM_STATE_MOLID).  The next reaction step's intramolecular /
 * intraresidual filters read these. */
int chem_reaction_init(chem_ctx* ctx, int interval, int nearest, int max_per_interval, uint64_t seed);
/* ar.add_reaction(Reaction(...))  reaction_setup.py:81-92,506; returns the reaction index */
int chem_reaction_add(chem_ctx* ctx, const chem_reaction_desc* d);
/* topology_manager.register_tuple/triplet/quadruplet(list, t1, t2[, t3[, t4]])
 * start_simulation.py:395-440: new bonds spawn entries of `list` when the type tuple matches.
 *   when         in the reaction step, after ALL bonds of the step are in the bond graph; the step's bonds (a, b) = (role 1,
 *                role 2) are taken in canonical order (min id, max id).
 *   types        those right after the step's events (a type the same event changed decides the match) and before any
 *                neighbour change of the step (chem_reaction_neighbour_change does not).
 *   candidates   per bond, neighbours walked in ascending tag: triples (n, a, b) for n bonded to a, then (a, b, m) for m bonded
 *                to b; then quadruples, per n bonded to a: (n', n, a, b) for n' bonded to n, then (n, a, b, m) for m bonded to
 *                b; then (a, b, m, m') for m bonded to b, m' bonded to m.  A particle appears once in a tuple.
 *   which list   the first list of the tuple's arity, in handle order, that has a registered type tuple (in registration
 *                order) equal to the tuple's types read forward or reversed; the forward match is preferred and the tuple is
 *                stored in the matching orientation.  No later list is tried, also where that list holds the tuple already.
 *   duplicates   a list holds a tuple once, whatever its orientation: two adjacent bonds of one step give one angle.
 *   exclusion    the (first, last) pair of a tuple is excluded only when the tuple was inserted. */
int chem_topology_register(chem_ctx* ctx, int arity, int list, const int32_t* types);
/* integrator.PostProcessChangeNeighboursProperty(tm).add_change_property(old_type, TopologyParticleProperties, nb_level),
 * attached to the reactions of a group by `extensions=` (reaction_post_process.py:76-115, reaction_setup.py:128-165;
 * examples/atrp_lj/atrp.cfg `type_transfers=MA:2->PA,ML:1->PL(state=1)`).  After the events of a reaction step have
 * been applied and the new bonds are in the graph, every particle exactly `nb_level` bonds away from a reactant of an
 * event of `reaction` (invoke_on 1: the type_1 role, 2: the type_2 role, 3: both) whose type is `old_type` gets
 * new_type / new_mass / new_q and, if set_state != 0, chemical state new_state.  Events are visited in canonical order
 * (min id, max id), role 1 before role 2, rules in the order they were added.  The graph distance is exact (a particle
 * reachable at two distances counts at the shorter one); the particles of one visit are taken in ascending tag; a later
 * visit sees the types and states an earlier one left.  new_mass and new_q are set also where new_type == old_type. */
typedef struct chem_nb_change {
  int32_t reaction, invoke_on, old_type, nb_level;
  int32_t new_type, set_state, new_state, pad;   /* set_state 0: keep the state, 1: state = new_state, 2: state += new_state (incr_state) */
  double  new_mass, new_q;
  int32_t min_state, max_state;                  /* only neighbours whose state is in [min, max) change (set_min_max_state); min >= max: no window */
} chem_nb_change;
int chem_reaction_neighbour_change(chem_ctx* ctx, const chem_nb_change* rule);
/* reaction.add_constraint(ReactionConstraintNeighbourState(type, min_state, max_state), 'type_1' | 'type_2')
 * reaction_setup.py:203-204 (exchange reactions `A:B + C -> A:C + B`, which the reference sets up as a virtual A + C reaction
 * that requires A to carry a B): a candidate pair is accepted only if the particle in role `role` (1 | 2) has a bonded
 * neighbour of type nb_type whose chemical state is in [min_state, max_state).
 *   one per reaction   a reaction carries ONE constraint: a second call for the same reaction replaces the first, whatever
 *                      its role.
 *   what is read       bond graph, types and states as they are at the start of that step's association scan (after the
 *                      step's dissociation block; the events, neighbour changes and ATRP firings of earlier steps included).
 *   who is judged      the particle that holds `role` after the role assignment of the scan: the forward assignment (lower
 *                      tag = type_1) first, the reversed one only where the forward one does not fit.  A pair that fits
 *                      both assignments (equal types, both in both windows) is judged by the forward one alone: it is NOT
 *                      tried reversed when the constraint fails. */
int chem_reaction_constraint(chem_ctx* ctx, int reaction, int role, int nb_type, int min_state, int max_state);
/* integrator.RestrictReaction(...).define_connection(b1, b2)  reaction_setup.py:75-78,115-128 (group option
 * `connectivity_map`: a file of id pairs): reaction `reaction` only accepts candidate pairs whose unordered id pair was
 * defined; everything else about the reaction is unchanged.  Calls accumulate. */
int chem_reaction_restrict(chem_ctx* ctx, int reaction, int64_t n, const int64_t* id_pairs);
/* integrator.ATRPActivator(system, interval, num_particles, ratio_activator, ratio_deactivator, delta_catalyst,
 *     k_activate, k_deactivate) + .select_from_all + add_reactive_center(type_id, state, is_activator, new_property,
 *     delta_state)  -- src/chemlab/reaction_post_process.py:380-426, examples/atrp_lj/atrp.cfg:15-25.  An integrator
 * extension that fires every `interval` steps (after the reaction step when both fall on the same step -- the driver
 * adds it behind `ar`, start_simulation.py:737-740) and flips reactive centres between dormant and active:
 *   pool      = every particle (select_from_all != 0) or every particle matching a centre's (type, state);
 *   selection = the num_particles members of the pool with the smallest key (Philox stream keyed (seed, step, tag):
 *               out[0] = key, ties by tag; out[1] = acceptance uniform); visited in that order;
 *   a selected particle matching centre c (first match in insertion order) is flipped with probability
 *               k_activate * ratio_activator   when c.is_activator == 0  ("A" centres: consume activator),
 *               k_deactivate * ratio_deactivator when c.is_activator != 0 ("DA" centres: consume deactivator);
 *   a flip sets type/mass/q to the centre's new property where new_type differs from the particle's type (a centre that
 *               names the type the particle already has changes neither its mass nor its charge), state += delta_state, and moves
 *               delta_catalyst / num_particles of catalyst from the consumed pool to the other one (clamped at 0).
 * The arithmetic lives in the external ESPResSo++ fork; this rule set is this build's restatement of the call
 * site's contract ([EXT-RECALL]).  desc == NULL disconnects the extension. */
typedef struct chem_atrp_desc {
  int32_t interval, num_particles, select_from_all, pad;
  double  ratio_activator, ratio_deactivator, delta_catalyst, k_activate, k_deactivate;
  uint64_t seed;
} chem_atrp_desc;
typedef struct chem_atrp_stats {     /* one row per firing (the reference writes them to `stats_file`) */
  int64_t step, candidates, selected, activated, deactivated;
  double  ratio_activator, ratio_deactivator;
} chem_atrp_stats;
int chem_atrp_init(chem_ctx* ctx, const chem_atrp_desc* desc);
int chem_atrp_add_center(chem_ctx* ctx, int type, int state, int is_activator, int new_type, double new_mass, double new_q, int delta_state);
int64_t chem_atrp_get_stats(chem_ctx* ctx, chem_atrp_stats* out, int64_t cap);
/* One dissociation reaction  T1(min1,max1):T2(min2,max2) -> N1(d1) + N2(d2): breaks bonds of the pair list `bond_list`.
 * Replaces espressopp.integrator.DissociationReaction(type_1, type_2, delta_1, delta_2, min_state_1, max_state_1,
 * min_state_2, max_state_2, rate, fpl, cutoff) + .diss_rate + .active and the PostProcessChangeProperty type change
 * (reaction_setup.py:257-356; examples/atrp_activator/atrp.cfg:77-84 `I(0,5):I(0,5) -> I(1) + I(1)`).  The arithmetic
 * lives in the external ESPResSo++ fork; this rule set is this build's restatement of the call site's contract
 * ([EXT-RECALL]).
 *
 * Runs every `interval` steps (chem_reaction_init) at the reaction step, BEFORE the association scan of that step.
 *   candidates  every entry (a, b) of `bond_list`, in list order.  a takes role 1 if type[a] == type_1 and
 *               type[b] == type_2, otherwise the swap is tried; if both fit (equal types) the particle with the lower
 *               id takes role 1.  Current types; both chemical states must lie in their half-open windows, read
 *               before any of this step's dissociation events.
 *   distance    exact fp64 minimum-image r^2 of the decoded positions, no FMA contraction (as the association scan).
 *   decision    the bond breaks if  cutoff > 0 && r^2 >= cutoff^2,  or if  u01(out[0]) < p  with
 *               p = diss_rate * dt * interval  (fp64, in that order) and
 *               out = dissociation_draw(seed, step, tag_lo, tag_hi, r)  (include/chem_philox.h; seed of
 *               chem_reaction_init, step as the event reports it, r the index this call returned).  Several
 *               dissociation reactions on one list are tried in index order, the first that breaks the bond wins.
 *   independence every qualifying bond breaks on its own: no one-event-per-particle resolve, no max_per_interval; a
 *               particle that loses k bonds in one step receives k * delta.
 *   apply       state += delta_{1,2}; where new_type_{1,2} >= 0 type, mass and q change AT ONCE (the delayed change of
 *               the reference's BasicDynamicResolution(alpha): new_type = -1 here, chem_reaction_set_resolution(r, role, 0)
 *               and chem_resolution_rate on the old type with the change; where one particle gets several new
 *               types in one step the last event in list order wins).  The entry leaves `bond_list` (order of the
 *               survivors kept) and the pair leaves the bond graph (unless another pair list still holds it).  mol_id of
 *               the two fragments becomes the lowest particle of each bonded cluster (nothing changes if a still
 *               reaches b); res_id stays: a merge cannot be undone.  unexclude != 0 lifts the 1-2 exclusion (a, b).
 *               Every triple / quadruple that holds a, b as consecutive members is removed.  Known limit: the 1-3 / 1-4
 *               exclusions those tuples once caused stay.
 *   afterwards  the association scan of the same step sees the new states, types, labels and exclusions (a pair that
 *               just broke may bond again at once if it qualifies); forces change with the next evaluation, in front
 *               of which the lists are rebuilt.
 *   event log   one chem_event per broken bond: `reaction` = the returned index (one index space with
 *               chem_reaction_add), id_a / id_b the role-1 / role-2 particle, r2 as above, pad = 0.  The events of a
 *               step form a block of their own in front of that step's association events; chem_get_events sorts
 *               inside each block as described at chem_event.
 * Not on the decomposed path: chem_comm_init* after this call, or this call after chem_comm_init*, is CHEM_ENOTIMPL. */
typedef struct chem_dissociation_desc {
  int32_t type_1, type_2;
  int32_t delta_1, delta_2;
  int32_t min_state_1, max_state_1;   /* half-open [min,max) */
  int32_t min_state_2, max_state_2;
  double  diss_rate;
  double  cutoff;                     /* <= 0: no distance rule */
  int32_t bond_list;                  /* handle of the arity-2 list that is scanned */
  int32_t unexclude;                  /* 1: a broken pair interacts through the pair potential again */
  int32_t active;
  int32_t new_type_1, new_type_2;     /* -1: unchanged */
  int32_t pad;
  double  new_mass_1, new_mass_2;     /* used when the type changes */
  double  new_q_1, new_q_2;
} chem_dissociation_desc;
/* ar.add_reaction(DissociationReaction(...))  reaction_setup.py:330-356; returns the reaction index */
int chem_dissociation_add(chem_ctx* ctx, const chem_dissociation_desc* d);
/* integrator.addExtension(ar) / ar.disconnect()  start_simulation.py:735-741,776-777: both kinds of reaction */
int chem_reactions_enable(chem_ctx* ctx, int on);
/* per-reaction rate update (Arrhenius hook, start_simulation.py:785-796); on an index of chem_dissociation_add: diss_rate */
int chem_reaction_set_rate(chem_ctx* ctx, int reaction, double rate);

/* ---- region rules: FreezeRegion, ChangeParticleType ------------------------------------- */
/* integrator.ChangeInRegion(system, ParticleRegion, prob | p_num | p_num_percentage) with set_particle_properties / set_flags
 * (ext_type=FreezeRegion: box edges act as sinks, a particle of the target type that reaches one becomes an inert type), and
 * integrator.ChangeParticleType(system, interval, num_particles, old_type, new_type) -- reaction_post_process.py:139-201,
 * 364-378.  The arithmetic is in the external fork, so this rule set is this build's own ([EXT-RECALL], parity unpinned;
 * DESIGN.md "Region rules").
 *
 * A rule holds a box [lo, hi) in folded coordinates, a target type and what becomes of a selected particle.
 *   firing      an enabled rule fires at every step counter value s > 0 with s % interval == 0, behind the second half kick
 *               that completes step s and behind the reaction, dissociation and ATRP work of the same s.  It works on the
 *               positions x(s) exactly as chem_get_state(CHEM_STATE_POS) returns them at that step (decoded, folded), compared
 *               in fp64 with lo / hi.  run(a); run(b) gives the same bits as run(a + b).
 *   candidates  of rule k at step s: the particles of target_type with lo[d] <= x[d] < hi[d] on every axis.  Rules act in
 *               insertion order; a particle changed by an earlier rule of the step is seen by later rules with its new type.
 *   selection   out = chem_philox::region_draw(seed, s, tag, k): out[0] is the selection key (ties broken by tag), out[1]
 *               gives the acceptance uniform u01(out[1]).
 *                 mode 0  every candidate
 *                 mode 1  the candidates with u01(out[1]) < value
 *                 mode 2  the min(num, |C|) candidates with the smallest key
 *                 mode 3  the floor(value |C|) candidates with the smallest key (fp64 product)
 *               A pure function of (seed, step, tag, rule): never of thread or particle order.
 *   the change  type := new_type; mass and charge := new_mass, new_q unless new_mass < 0 (then both are kept); v := 0 exactly
 *               when reset_velocity; the stored force := 0 exactly when reset_force, so the next half kick adds nothing to the
 *               particle.  Everything else is treated as after a type change by any route: the particle is re-stamped
 *               (chem_set_resolution section), by-types list slots are resolved against the new type before the next force
 *               evaluation, a typed fixed-distance set (chem_fix_create) judges its entries with the new type at once, the
 *               chemical state is kept.  Forces are NOT evaluated again at s: every other particle keeps the stored force of
 *               step s for one more half kick, as under the reference's integrator; the force list is rebuilt in front of the
 *               next evaluation, which uses the new type -- also where a chem_run call ends at s and the next begins there.
 *               Afterwards the particle is an ordinary particle of new_type (chem_thermostat_langevin_types decides whether the
 *               thermostat moves it).
 *   lifetime    regions are absolute lengths fixed at chem_region_add: a barostat does not move or scale them.  Rules survive
 *               chem_set_particles, like reactions; the change log and the stats are cleared there.  A rule is off until
 *               chem_region_enable(rule, 1).
 *   cost        while an enabled rule is due, one scan launch on the run's stream per firing step, and that step's two
 *               half kicks are launched apart (as on a reaction step).  A firing that changes nothing never synchronises the
 *               host on the fused tile path; one that does stops the asynchronous run at that step (the DevCtl halt / resume
 *               route), the host applies the change and resumes: one synchronisation per firing that changes something.  On
 *               the per-cell and brute-force list paths (boxes of few cells) and under a barostat every firing synchronises.
 *               A context without a rule launches and allocates nothing for this.
 *   logs        chem_region_get_changes: every change as (step, id, rule), ordered by step, then rule, then id.
 *               chem_region_get_stats: one row per firing of a rule that changed something, same order.  chem_region_counters:
 *               firings = firing steps (steps on which at least one enabled rule was due) and syncs = host synchronisations
 *               the rules caused, since the context was created.  out == NULL: the count alone.
 *   checkpoint  the blob format and its fingerprint do not know the rules: the change log, the stats and the counters are not
 *               part of a blob -- after a load they hold what happened since.  The draws are counter based, so a context set up
 *               alike, with the same rules enabled, that loads a blob goes on bit for bit.
 * CHEM_EINVAL: a type outside [0, CHEM_MAX_TYPES), lo > hi, a non-finite bound, interval < 1, value outside [0, 1] (modes 1
 * and 3), num < 0 (mode 2), an unknown mode, new_mass == 0 or non-finite, an unknown rule index.  CHEM_ENOSPC: more than
 * CHEM_MAX_REGIONS rules.  Not on the decomposed path (a selection by count would need a gather across ranks):
 * chem_region_add after chem_comm_init*, and chem_comm_init* after a rule, are CHEM_ENOTIMPL. */
#define CHEM_MAX_REGIONS 16
typedef struct chem_region_desc {
  double   lo[3], hi[3];        /* folded coordinates; a particle is inside when lo[d] <= x[d] < hi[d] on every axis */
  int32_t  target_type, new_type;
  double   new_mass, new_q;     /* new_mass < 0: mass and charge are kept (what both call sites do) */
  int32_t  interval;            /* >= 1 */
  int32_t  mode;                /* 0 all candidates, 1 prob, 2 num, 3 fraction */
  double   value;               /* mode 1: probability in [0,1]; mode 3: fraction in [0,1] */
  int32_t  num;                 /* mode 2 */
  int32_t  reset_velocity, reset_force;
  uint64_t seed;
} chem_region_desc;
typedef struct chem_region_change { int64_t step; int64_t id; int32_t rule, pad; } chem_region_change;
typedef struct chem_region_stats { int64_t step; int64_t rule; int64_t candidates, changed; } chem_region_stats;
int     chem_region_add(chem_ctx* ctx, const chem_region_desc* desc);      /* -> rule index >= 0 */
int     chem_region_enable(chem_ctx* ctx, int rule, int on);
int64_t chem_region_get_changes(chem_ctx* ctx, chem_region_change* out, int64_t cap);
int64_t chem_region_get_stats(chem_ctx* ctx, chem_region_stats* out, int64_t cap);
int     chem_region_counters(chem_ctx* ctx, int64_t* firings, int64_t* syncs);   /* either pointer may be NULL */

/* ---- checkpoint and exact restart ------------------------------------------------------ */
/* Stop a run and go on with it in another process (the reference's jobs are 5 M-step runs under wall limits of 24 to 72 h,
 * examples/mf/espp_cg_1/params and the *.pbs files).  The reference has no such call: this rule set is
 * this build's own (DESIGN.md "Checkpoint").
 *
 * A blob holds the STATE of a context, not its CONFIGURATION.
 *   configuration  what the set-up calls define and no chem_run changes: box-independent lengths (cutoffs, skin), dt, pair
 *                  potentials and tables, the list table (arity, kind, by types, hybrid) and every list's parameters and
 *                  registered type tuples, thermostat and barostat parameters, reaction, dissociation, neighbour, removal, join,
 *                  release and ATRP descriptors, restrictions and constraints, fix sets with their post-processes, resolution
 *                  marks, caps and rates, options.  The caller repeats those calls on a fresh context -- chem_set_particles (and
 *                  chem_add_particles) with the ids of the saved context included, whatever else it passes there -- and then loads.
 *   state          everything chem_run changes: the step; the box; the barostat's state (what chem_barostat_state_get shows, and
 *                  what the scalings since the last list build were charged to the lists); the particle table in id order (id,
 *                  type, chemical state, res_id, mol_id, mass, charge, position, image counters, velocity), particles of
 *                  chem_add_particles included; the resolution stamps; every list's entries in order, with the birth steps of a
 *                  hybrid list; the exclusions; the bond graph of the topology manager; the entries of every fix set with
 *                  chem_fix_log and chem_fix_joins; chem_reaction_removed; the event log (chem_get_events on the restored context
 *                  returns the whole log); the ATRP statistics and catalyst ratios; chem_reactions_enable.
 *   not state      rebuild and idle-launch diagnostics (the counters of chem_get_timers, chem_debug_*): they go on counting in the
 *                  saving context and start at zero in the loading one.
 * The contract.  Context A has run; blob = chem_checkpoint_save(A).  Context B is set up like A and calls chem_checkpoint_load(B,
 * blob).  From then on A and B are indistinguishable: every chem_get_* / chem_*_get / chem_observe value is equal, floating-point
 * values bit for bit, at once and after any further chem_run(b), in both precisions and on every list path (tiles, per-cell
 * lists, brute force).  This is how it is kept: save pulls the device's particle data into the host's staging arrays (coordinates
 * as the device holds them, image counters beside them), writes the blob from the host data, and then leaves A exactly as load
 * leaves B -- the same routine puts the blob's data in place and raises every dirty flag, so that particles, tables and lists are
 * uploaded and built again and the forces are evaluated anew at the next call that needs them.  So
 *   - chem_checkpoint_save is a list-build point: a run that saved differs in the last bits (the summation order of the forces
 *     follows the particle order of the list build) from one that never did; the time of a step is not touched;
 *   - chem_get_state(CHEM_STATE_FORCE) between a save (or load) and the next chem_run shows zeros, as after chem_set_particles;
 *   - two saves with nothing run between them, and a save right after a load, give the loaded bytes again.
 * chem_checkpoint_save(ctx, NULL, 0) returns the bytes needed and touches nothing; with a buffer it returns the bytes written,
 * CHEM_ENOSPC (nothing touched) if cap is smaller.  The blob: magic, format version, precision, then sections that each carry
 * their length -- the first is a fingerprint of the configuration: the CHEM_MAX_* values, the list table (arity, kind, by_types,
 * hybrid per handle), the lengths of the reaction and dissociation tables, the fix-set count, whether ATRP is on, the particle
 * count -- and a checksum at the end (chem_ckpt_host.hpp).  chem_checkpoint_load validates the whole blob before it changes
 * anything; a refused load leaves the context as it was.
 *   CHEM_ENOTIMPL  save or load on a decomposed context (after chem_comm_init*): a gap of the decomposed path, like the barostats;
 *                  decomposing a context that holds a loaded state is refused at its next upload likewise.
 *   CHEM_EINVAL    precision or fingerprint mismatch, naming the first field that differs; other particle ids; another barostat
 *                  kind; a short, truncated or corrupt blob or an unknown format version (never a read past nbytes).
 *   CHEM_ESTATE    chem_checkpoint_save or _load before chem_set_particles; chem_add_particles on a context that holds a staged
 *                  state (add before loading).
 * Out of scope: blobs across precisions or format versions, saving the configuration, the driver's loop counter. */
int64_t chem_checkpoint_save(chem_ctx* ctx, void* buf, int64_t cap);
int     chem_checkpoint_load(chem_ctx* ctx, const void* buf, int64_t nbytes);

/* ---- radial distribution functions ------------------------------------------------------ */
/* Time-averaged g(r) per type pair, accumulated on the device as exact integer counts; a frame can be taken inside chem_run
 * without a host round trip.  (Upstream's analysis.RadialDistrF bins one configuration on the host, out to half the box; this
 * rule set is this build's own.)
 *   Pairs.     Every unordered pair of distinct particles {i, j} of the whole system, dummies of fixed-distance sets and excluded
 *              (bonded, 1-3, 1-4) pairs included, once per frame.
 *   Distance.  d2 = the fp64 minimum-image r^2 of the decoded positions, without FMA contraction: the expression of the
 *              reaction scan (the fp32 build decodes its fixed-point positions to double first).
 *   Bins.      dr = r_max / nbins in fp64, e[k] = (double)k * dr, e2[k] = e[k] * e[k], k = 0..nbins.  A pair is in the bin k with
 *              e2[k] <= d2 < e2[k+1] and is not counted when d2 >= e2[nbins].  The edges decide, never the rounding of a sqrt.
 *              r_max <= max_cutoff (chem_set_cutoff): the tile tables of the last build hold every pair inside max_cutoff while
 *              the skin lasts, and nothing beyond.  A wider range is out of scope.
 *   Selectors. Up to CHEM_RDF_MAX_PAIRS unordered type pairs (t1, t2), -1 = any type.  A pair is counted in EVERY selector it
 *              matches, so (-1, -1) is the total.  Types are those at the sampled step.
 *   Split.     split_molecules != 0: two histograms per selector, intra (mol_id[i] == mol_id[j], the labels the reaction scan of
 *              that step would read) and inter, in that order; otherwise one.
 *   Normalisers, per selector and frame: M = the number of unordered pairs of distinct particles whose types match, from the
 *              type counts c[]: the sum over matching type pairs u <= v of c_u (c_u - 1) / 2 (u == v) or c_u c_v.  Accumulated:
 *              frames; pairs[sel] = sum of M_f; density[sel] = sum of M_f / V_f in frame order, V_f = Lx Ly Lz of that frame.
 *   Result.    g_sel(k) = counts[sel][k] / (density[sel] (4 pi / 3) (e[k+1]^3 - e[k]^3)); the division is the caller's.
 *   Frames.    chem_rdf_sample takes one now, with chem_observe's preconditions and side effects and no others.
 *              chem_rdf_sample_every(every) takes one inside chem_run at every step s with s % every == 0: of the positions the
 *              forces of step s were evaluated at (what CHEM_STATE_POS shows if the run ends at s), enqueued behind that step's
 *              force launch and in front of the next integrate launch, without a host wait (with the split, a label merge of the
 *              last reaction step that is still running on the host is joined first, as the reaction scan does); every <= 0
 *              switches it off.  A run is not sampled at its starting step, so run(a); run(b) accumulates bit for bit what
 *              run(a + b) does.
 *   Read-only. With sampling on, positions, velocities, forces, events and rebuild counters are bit for bit those of the same
 *              run without it.  A context that never calls chem_rdf_* allocates nothing and launches what it launched before.
 *   Not state. Accumulators and configuration are no part of a checkpoint; save and load leave them alone.
 * chem_rdf_init: npairs = 0 switches everything off and frees the buffers; a second call reconfigures and resets.
 * chem_rdf_get returns the configuration and normalisers in *out and the counts as [npairs][1 + split][nbins] (counts may be
 * NULL with cap 0 to read the normalisers alone).
 *   CHEM_EINVAL    r_max not finite or not positive, nbins outside 1..CHEM_RDF_MAX_BINS, npairs outside 0..CHEM_RDF_MAX_PAIRS, a
 *                  type outside -1..CHEM_MAX_TYPES-1; at the next sample or run: r_max > max_cutoff (both values named, since the
 *                  cutoff can be set later), a histogram that does not fit the LDS beside the staged particles, or more than
 *                  65536 particles on a path without tiles.
 *   CHEM_ENOSPC    chem_rdf_get with a cap below npairs * (1 + split) * nbins.
 *   CHEM_ESTATE    chem_rdf_sample, chem_rdf_sample_every, chem_rdf_get or chem_rdf_reset before chem_rdf_init (or after
 *                  npairs = 0).
 * Slabs.  Every rank accumulates the pairs of its own home particles; a pair with a ghost member is counted by the rank that owns
 * its lower tag, and a frame adds no communication.  frames, pairs and density are kept on the host from the type table, which is
 * replicated by tag.  chem_rdf_get is collective, like chem_get_pressure, and returns the global integers on every rank.
 * The per-cell and brute-force paths of a single domain run an all-pairs pass, O(N^2): refused (CHEM_EINVAL, at the next sample or
 * run) above 65536 particles.  Under a barostat V_f is the box the forces of the sampled step were evaluated in. */
#define CHEM_RDF_MAX_PAIRS 8
#define CHEM_RDF_MAX_BINS  1024
int chem_rdf_init(chem_ctx* ctx, double r_max, int nbins, int npairs, const int32_t* type_pairs /* 2*npairs, -1 = any */, int split_molecules);
int chem_rdf_sample(chem_ctx* ctx);
int chem_rdf_sample_every(chem_ctx* ctx, int every);
typedef struct chem_rdf_result { double r_max; int32_t nbins, npairs, split; int64_t frames; uint64_t pairs[CHEM_RDF_MAX_PAIRS]; double density[CHEM_RDF_MAX_PAIRS]; } chem_rdf_result;
int chem_rdf_get(chem_ctx* ctx, chem_rdf_result* out, uint64_t* counts /* [npairs][1+split][nbins] */, int64_t cap);
int chem_rdf_reset(chem_ctx* ctx);   /* zero the accumulators, keep the configuration */

/* ---- static structure factor --------------------------------------------------------------- */
/* Time-averaged partial structure factors on the reciprocal lattice of the box, accumulated on the device in fp64: the structure
 * beyond max_cutoff that g(r) cannot show.  A frame can be taken inside chem_run without a host round trip.  (Upstream has
 * analysis.StaticStructF; this rule set is this build's own.)
 *   Vectors.   q(n) = 2 pi (nx / Lx, ny / Ly, nz / Lz) of the frame's box, n integer, |n_a| <= nmax, 1 <= nmax <= CHEM_SQ_MAX_N.
 *              Only the canonical half is kept (S(-q) = S(q)): n != 0 with nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and
 *              nz > 0.  nvec = ((2 nmax + 1)^3 - 1) / 2: 13 for nmax = 1, 171 for 3, 2456 for 8, 17968 for 16.  The index k runs
 *              over the kept vectors in lexicographic order of (nx, ny, nz); the map k <-> n is sq_vec / sq_index of
 *              chemlab_amd/csrc/chem_sq_host.hpp (Python: chemlab_amd.engine.sq_vectors), used by the kernels too.
 *   Phases.    f_a = x_a * invL_a in fp64, x the decoded position the reaction scan and chem_rdf_* use (the fp32 build decodes
 *              its fixed-point positions to double first), invL of the box the sampled step's forces were evaluated in;
 *              theta_j(n) = 2 pi (nx f_x + ny f_y + nz f_z).  All arithmetic of this feature is fp64 in both precisions.
 *   Selectors. Up to CHEM_SQ_MAX_PAIRS unordered type pairs (t1, t2), -1 = any type; types are those at the sampled step.  With
 *              the type sets A (of t1) and B (of t2): rho_A(n) = sum over j with type_j in A of exp(-i theta_j(n)); dummies of
 *              fixed-distance sets are included, as for g(r).
 *   Accumulated, per selector s and vector k, over the frames: sums[s][k] += Re(rho_A(n_k) conj rho_B(n_k)); na[s] += N_A and
 *              nb[s] += N_B, the particle counts of the two sets in the frame, as doubles; frames += 1; box_sum[a] += L_a.
 *   Result.    S_s(n) = sums / sqrt(na nb), the Ashcroft-Langreth partial; (-1, -1) gives the total <|rho|^2> / N.  The
 *              division, |q| at the mean box box_sum / frames and any shell average are the caller's.
 *   Frames.    As for chem_rdf_*: chem_sq_sample takes one now, with chem_observe's preconditions and side effects and no
 *              others.  chem_sq_sample_every(every) takes one inside chem_run at every step s with s % every == 0: of the
 *              positions the forces of step s were evaluated at, enqueued behind that step's force launch and in front of the
 *              next integrate launch, without a host wait; every <= 0 switches it off.  A run is not sampled at its starting step.
 *   Read-only. With sampling on, positions, velocities, forces, events and rebuild counters are bit for bit those of the same
 *              run without it.  A context that never calls chem_sq_* allocates nothing and launches what it launched before.
 *   Determinism. No floating-point atomics.  A workgroup sums its particle slots in slot order, the partial sums of the
 *              super-chunks are added in index order: the order is a function of (slot order, n, nvec, the launch plan) alone.
 *              Two frames of the same context state give the same bits, and on a single domain run(a); run(b) accumulates bit
 *              for bit what run(a + b) does.
 *   Not state. Accumulators and configuration are no part of a checkpoint; save and load leave them alone.
 * chem_sq_init: npairs = 0 switches everything off and frees the buffers; a second call reconfigures and resets (in-run sampling
 * is off again).  chem_sq_get returns the configuration and the books in *out and the sums as [npairs][nvec] (sums may be NULL
 * with cap 0 to read the books alone).
 *   CHEM_EINVAL    nmax outside 1..CHEM_SQ_MAX_N, npairs outside 0..CHEM_SQ_MAX_PAIRS, a type outside -1..CHEM_MAX_TYPES-1, null
 *                  type_pairs with npairs > 0.
 *   CHEM_ENOSPC    chem_sq_get with a cap below npairs * nvec.
 *   CHEM_ESTATE    chem_sq_sample, chem_sq_sample_every, chem_sq_get or chem_sq_reset before chem_sq_init (or after npairs = 0).
 * Slabs.  Every rank sums rho over its home particles (never ghosts); the rho array (classes x nvec x 2 doubles) goes through the
 * transport's all-reduce on the run's stream, as the velocity-rescale thermostat's kinetic energy does, and every rank squares and
 * accumulates the global rho.  na, nb, frames and box_sum are kept on the host from the type table, which is replicated by tag.
 * Every transport of this build hands every rank the same bits from its all-reduce (the in-process and the shared-memory
 * transports add the ranks' words in rank order on every rank, RCCL delivers one reduced buffer), so every rank holds the same
 * accumulators and chem_sq_get is NOT collective.  Slab sums differ from single-domain sums in the last bits (another order).
 * The shared-memory transport (chem_comm_init_ipc) reduces at most 64 values per call and answers a frame with CHEM_ECOMM. */
#define CHEM_SQ_MAX_N     16
#define CHEM_SQ_MAX_PAIRS 4
typedef struct chem_sq_result { int32_t nmax, npairs; int64_t nvec, frames;
  double na[CHEM_SQ_MAX_PAIRS], nb[CHEM_SQ_MAX_PAIRS], box_sum[3]; } chem_sq_result;
int chem_sq_init(chem_ctx* ctx, int nmax, int npairs, const int32_t* type_pairs /* 2*npairs, -1 = any */);
int chem_sq_sample(chem_ctx* ctx);
int chem_sq_sample_every(chem_ctx* ctx, int every);
int chem_sq_get(chem_ctx* ctx, chem_sq_result* out, double* sums /* [npairs][nvec], may be NULL with cap 0 */, int64_t cap);
int chem_sq_reset(chem_ctx* ctx);   /* zero the accumulators, keep the configuration */

/* ---- the hot call -------------------------------------------------------------------- */
/* integrator.run(n)  start_simulation.py:780.  No host round trip per step. */
int chem_run(chem_ctx* ctx, int64_t nsteps);

/* ---- read-back ----------------------------------------------------------------------- */
int64_t chem_num_particles(chem_ctx* ctx);
int64_t chem_get_step(chem_ctx* ctx);
/* storage.getParticle(pid).pos/.v/.type/...; returns number of particles written */
int64_t chem_get_state(chem_ctx* ctx, int what, void* out, int64_t cap_elems);
int64_t chem_get_events(chem_ctx* ctx, chem_event* out, int64_t cap);
int64_t chem_get_exclusions(chem_ctx* ctx, int64_t* out_pairs, int64_t cap_pairs);
/* current Verlet list as unique id pairs (id_lo,id_hi), sorted; for tests/diagnostics */
int64_t chem_get_verlet_pairs(chem_ctx* ctx, int64_t* out_pairs, int64_t cap_pairs);
/* analysis.Temperature/KineticEnergy/PotentialEnergy/NFixedPairListEntries  start_simulation.py:453-493 */
int chem_observe(chem_ctx* ctx, chem_obs* out);
/* integrator.getTimers()/verletlist.get_timers()  start_simulation.py:1040-1076 */
int chem_get_timers(chem_ctx* ctx, chem_timers* out);
int chem_device_sync(chem_ctx* ctx);

/* ---- tuning -------------------------------------------------------------------------- */
/* neighbours per particle the list can hold (0 = automatic from density) */
int chem_set_nlist_capacity(chem_ctx* ctx, int max_neighbours);
/* generic integer knobs, see DESIGN.md ("tpp": lanes per particle in the pair kernel, ...) */
int chem_set_option(chem_ctx* ctx, const char* name, double value);
/* counters of "neighbour launch only on steps that can need a rebuild" (options skip_idle, idle_lag, idle_kappa; DESIGN.md
 * section 5), since the context was created: steps that ran without the neighbour launch; such steps on which a rebuild fell
 * due after all (the run stopped there and the step was redone); waits for the device's published state that ran out */
int64_t chem_debug_idle_skipped(chem_ctx* ctx);
int64_t chem_debug_idle_wrong_skips(chem_ctx* ctx);
int64_t chem_debug_idle_timeouts(chem_ctx* ctx);

/* ---- multi-GPU (spatial domain decomposition, RCCL halo) ------------------------------ */
/* storage.DomainDecomposition(system, nodeGrid, cellGrid) under mpirun
 * start_simulation.py:152-163.  uid comes from chem_comm_unique_id on rank 0. */
int chem_comm_unique_id(char uid[128]);
int chem_comm_init(chem_ctx* ctx, int nranks, int rank, const int node_grid[3], const char uid[128]);
/* Same decomposition with the ranks living in ONE process (one host thread per context) and
 * exchanging by device-to-device copies through a hub named `hub_id`: several domains on a single
 * GPU; used to validate the multi-rank path without a multi-GPU node. */
int chem_comm_init_local(chem_ctx* ctx, int nranks, int rank, int hub_id);
/* Same decomposition with one PROCESS per rank and the ghost/migration buffers mapped through hipIpc memory handles
 * (rendezvous in the POSIX shared-memory segment `shm_name`, the same fresh name on every rank): ranks may share a
 * device, which RCCL refuses -- the multi-process flow of `bench.py --gpus N` on a box with fewer than N GPUs. */
int chem_comm_init_ipc(chem_ctx* ctx, int nranks, int rank, const char* shm_name);

#ifdef __cplusplus
}
#endif
#endif /* CHEM_MI355_H */
