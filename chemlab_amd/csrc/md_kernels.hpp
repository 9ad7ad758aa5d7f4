// md_kernels.hpp -- hand-written CDNA4 (gfx950, wave64) kernels of the reactive-MD inner loop.
//
// Everything is templated on the storage/compute real type R (float: production,
// double: parity mode).  Layout in HBM (SoA of 16/32-byte vectors, cell-sorted order):
//   x4[i] = (x, y, z, (R)type)       v4[i] = (vx, vy, vz, mass)      f4[i] = (fx, fy, fz, 0)
//   tag[i]   : dense particle tag (rank of the external id)          img4[i]: image counters
//   by-tag   : rtag[tag] -> i, state[tag], res_id[tag], mol_id[tag]
//   nlist    : full neighbour list, row-major, row stride S ints, nn[i] entries used
// No MFMA anywhere: there is no dense contraction on this path (pair sums are gathers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/chem_mi355.h"
#include "../../include/chem_philox.h"
#include "chem_geom_host.hpp"
#include "chem_idle_host.hpp"
#include "chem_launch_host.hpp"
#include "chem_roworder_host.hpp"
#include "chem_baro_host.hpp"
#include "chem_region_host.hpp"
#include "chem_rdf_host.hpp"
#include "chem_sq_host.hpp"

namespace chem {

template <typename R> struct Vec4T;
template <> struct Vec4T<float> { using type = float4; };
template <> struct Vec4T<double> { using type = double4; };
template <typename R> using Vec4 = typename Vec4T<R>::type;

template <typename R> __device__ __forceinline__ Vec4<R> mk4(R a, R b, R c, R d);
template <> __device__ __forceinline__ float4 mk4<float>(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
template <> __device__ __forceinline__ double4 mk4<double>(double a, double b, double c, double d) { return make_double4(a, b, c, d); }

__device__ __forceinline__ float rint_r(float x) { return rintf(x); }
__device__ __forceinline__ double rint_r(double x) { return rint(x); }
__device__ __forceinline__ float sqrt_r(float x) { return sqrtf(x); }
__device__ __forceinline__ double sqrt_r(double x) { return sqrt(x); }
__device__ __forceinline__ float floor_r(float x) { return floorf(x); }
__device__ __forceinline__ float rcp_r(float x) { return __builtin_amdgcn_rcpf(x); }   // 1 ulp, fp32 production mode
__device__ __forceinline__ double rcp_r(double x) { return 1.0 / x; }
__device__ __forceinline__ double floor_r(double x) { return floor(x); }

constexpr int kMaxTypes = CHEM_MAX_TYPES;
#ifndef CHEM_INT_PER_BLOCK
#define CHEM_INT_PER_BLOCK 512
#endif
constexpr int kIntPerBlock = CHEM_INT_PER_BLOCK;   // particles per workgroup of k_integrate (= entries of the blockmax array per 512 particles)
constexpr int kWave = 64;

// ---- device-resident control block (one per context) ---------------------------------
struct DevCtl {
  unsigned long long step_max2_bits;  // max |dx|^2 of the current step (bits of a non-negative real)
  double acc_maxdist;                 // accumulated sqrt(max|dx|^2) since the last rebuild
  int need_rebuild;                   // decision of the current step (read by the rebuild chain)
  int force_rebuild;                  // host request (topology/exclusions changed): 1.  Set when a stopped run is resumed (halt below): 2 = build at
                                      // this step, the reference rule counts it as the regular decision it was; 4 = build again, everything is counted already
  int nl_overflow;                    // max neighbours seen when a row overflowed (0 = fine)
  int stage_overflow;                 // stencil tile exceeded the LDS capacity
  int cand_count;                     // reaction candidates appended
  int cand_overflow;
  int rebuild_count;
  int skin_violation;                 // list used with acc_maxdist > skin/2 (must never happen)
  int alive;                          // reaction resolve: pairs still undecided
  int accepted;                       // reaction resolve: accepted events
  long long nlist_entries;
  double step_m2;                     // max |dx|^2 of the step (after the cross-rank max in DD mode)
  int mig_error;                      // a particle left its slab by more than one layer / migration buffer overflow
  int bonded_missing;                 // a bonded partner is neither owned nor a ghost on this rank
  int barrier_timeout;                // fused rebuild: a grid barrier gave up waiting (fatal)
  int pad0;
  double acc_pp[2];                   // fused rebuild: accumulated distance, double-buffered by launch parity
  unsigned long long bw64;            // bonded work list: owners (low word) and entries (high word), one atomic per chunk
  int excl_slot_error;                // list build: an excluded partner was not found in the cell computed from its position (internal)
  int bucket_overflow;                // fused rebuild: a cell holds more particles than a bucket row (value = needed capacity)
  // Rebuild count of the REFERENCE rule (accumulated per-step maxima against the workload's skin/2, reset by every forced
  // rebuild): what chem_get_timers reports.  With an internal list skin wider than the workload's (option list_skin) the
  // lists are rebuilt less often than that; forces do not depend on it (the force kernel applies the exact cutoff).
  int ref_rebuilds;
  double acc_ref;
  // Recoverable stop of an asynchronous run: the fused rebuild met a cell fuller than a bucket row at step `halt_step`.  Every
  // later launch of the run leaves at once (integrate, forces, bonded, rebuild), so the state stays "drifted, forces of
  // halt_step not evaluated"; the host finds the flag at its next synchronisation, rebuilds with wider rows (or the unfused
  // chain) and resumes at that step.
  // halt: 1 a full bucket row (nothing of the step counted yet), 2 a rebuild fell due on a step without a neighbour launch
  // (k_pair_tiles guard 3; nothing counted either), 3 lists the launch could not finish (the step is counted).  halt_par: the
  // parity of acc_pp the stopped step's decision read.
  int halt;
  int bond_slot_miss;                 // list build: a bonded partner was not among the located excluded partners (internal: the host only enables inline bonds when it cannot happen)
  long long halt_step;
  int halt_par, pad1;
};

// ---- one step's decision about the Verlet list, shared by everything that takes it from fold words: the prologue of the force
// kernel (guard 2: slabs, guard 3: single domain without a neighbour launch) and P0 of k_rebuild_fused ----
// maximum of nwords bit patterns of non-negative reals, by every wave for itself: lane l takes words l, l + 64, ...
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long mb) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(mb, o); mb = v > mb ? v : mb; }
  return mb;
}
__device__ __forceinline__ unsigned long long fold_words_max(const unsigned long long* w, int nwords) {
  unsigned long long mb = 0;
  for (int q = (int)(threadIdx.x & 63); q < nwords; q += 64) { const unsigned long long v = w[q]; mb = v > mb ? v : mb; }
  return wave_max_u64(mb);
}
// the bookkeeping of a decision, by ONE thread of the launch: accumulated distance (double-buffered by parity: every workgroup
// of the launch reads [par]), the reference rule on the workload's skin (reported rebuild count; acc_ref and ref_rebuilds are
// this thread's alone) and the counts.  forced = DevCtl::force_rebuild as every workgroup read it.
__device__ __forceinline__ void decide_book(DevCtl* ctl, int par, int criterion, double m2, double acc, int need, int forced, double half_skin_ref) {
  ctl->step_m2 = m2; ctl->acc_pp[par ^ 1] = need ? 0.0 : acc; ctl->acc_maxdist = need ? 0.0 : acc;
  ctl->need_rebuild = need;
  if (forced & 4) return;      // a resumed step whose first launch counted it
  const double accr = criterion ? sqrt(m2) : ctl->acc_ref + sqrt(m2);
  const bool rn = (accr > half_skin_ref) || (forced & 1);
  ctl->acc_ref = rn ? 0.0 : accr;
  if (rn) ctl->ref_rebuilds++;
  if (need) ctl->rebuild_count++;
}
// the same thread tells the host where the device stands (chem_idle_host.hpp; pinned memory, the step last)
__device__ __forceinline__ void publish_hint(IdleHint* hint, int gen, long long step, double acc, double d) {
  if (!hint) return;
  volatile IdleHint* h = hint;
  h->gen = gen; h->acc = acc; h->d = d;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  h->step = step;
}

// bonded tables (per-tag CSR, see K4-K6 below; declared here because the list build records the LDS slots of bonded partners)
constexpr int kBondSlots = 8;   // inline bonds: recorded partner slots per home particle (two 8-byte words)
// The record of a home particle: the LDS slots of its bonded partners, four 16-bit slots per 8-byte word (slot k of a word in bits
// 16 k .. 16 k + 15, kBondRecNone = no partner; bond_records_fit, chem_launch_host.hpp, keeps every slot below it).  Two arrays,
// one word per particle each, indexed by the particle's place in the sorted arrays: rec0 holds partners 1-4 and is read by every
// lane of the force kernel as one dense stream, rec1 holds partners 5-8 and is written and read only behind a FULL rec0 (fourth
// slot set) -- a stale rec1 behind a rec0 that is no longer full is never looked at.
typedef uint2 BondRec;
struct BondRecs {
  BondRec* __restrict__ rec0; BondRec* __restrict__ rec1;
  CHEM_HD explicit operator bool() const { return rec0 != nullptr; }
};
// ... from four slots (any value with the low 16 bits set, ~0u included: no partner) and back (kBondRecNone: no partner)
CHEM_HD BondRec bond_rec_pack(unsigned int s0, unsigned int s1, unsigned int s2, unsigned int s3) {
  BondRec r; r.x = (s0 & 0xffffu) | (s1 << 16); r.y = (s2 & 0xffffu) | (s3 << 16); return r;
}
CHEM_HD void bond_rec_unpack(const BondRec r, unsigned int (&s)[4]) { s[0] = r.x & 0xffffu; s[1] = r.x >> 16; s[2] = r.y & 0xffffu; s[3] = r.y >> 16; }
CHEM_HD BondRec bond_rec_none() { return bond_rec_pack(kBondRecNone, kBondRecNone, kBondRecNone, kBondRecNone); }
CHEM_HD bool bond_rec_full(const BondRec r) { return (r.y >> 16) != kBondRecNone; }
// ... and slot k (0 .. kBondSlots - 1) of particle p's record in memory, for the one writer that records hit by hit (the generic
// path of the list sweep): the same layout as bond_rec_pack's, written 16 bits at a time
__device__ __forceinline__ unsigned short* bond_rec_slot(const BondRecs& b, size_t p, int k) {
  return reinterpret_cast<unsigned short*>(k < 4 ? b.rec0 + p : b.rec1 + p) + (k & 3);
}
struct BondedEntry { int t0, t1, t2, meta; };   // tuple tags in order (self included); meta = bonded_meta(slot, mypos) (chem_host.hpp); quadruples use a 2nd entry for t3
                                                // pairs: t2 = 0, or ~birth step (< 0) for an entry of a hybrid list (chem_list_set_hybrid)
                                                // triples and quadruples of a hybrid list (chem_list_set_hybrid_tuples; pad of their slot): a 2nd entry
                                                // (t3 or 0, 0, ~birth step, 0) -- the birth where the pairs keep it, so the work-list build hands it on
struct BondedParam { int kind, list, arity, pad; double p[CHEM_MAX_POT_PARAMS]; };   // pad = 1: slot of a hybrid list, (lambda0, rate) in HybridArgs::par[slot]
// Hybrid lists: what the HYB instantiations of the bonded kernels get beside the regular arguments.  lambda of an entry is a
// pure function of (step, birth step); chem_host.hpp HostList::hybrid_lambda is the same expression on the host.
struct HybridArgs { const double2* par; long long step; };
__device__ __forceinline__ double hybrid_lambda(const HybridArgs& hy, const BondedParam& bp, const int slot, const int t2) {
  if (!bp.pad) return 1.0;
  const double2 h = hy.par[slot];
  const double l = h.x + h.y * (double)(hy.step - (long long)(~t2));
  return l < 1.0 ? l : 1.0;
}
// a triple of a hybrid list is two entries wide, as every quadruple is (HostList::entry_width is the same rule on the host)
__device__ __forceinline__ bool hybrid_wide_triple(const BondedParam& bp) { return bp.pad && bp.arity == 3; }

template <typename R> struct Box {
  R L[3], invL[3];
  int nc[3];       // cells per axis (0 => brute-force list build); in z-ghost mode nc[2] = own layers + 2
  int ncell;
  R cell_inv[3];   // cells per unit length (global grid)
  // slab domain decomposition along z (chem_comm_init): layer 0 and nc[2]-1 are ghost layers that
  // hold copies of the neighbour ranks' boundary layers; x and y stay periodic in-kernel
  int zghost;      // 0: z periodic in-kernel, 1: ghost layers
  int z0g, nzg;    // first own global layer, global layer count
  R shz_lo, shz_hi;  // shift to apply to the lower / upper ghost layer (+-Lz across the periodic boundary)
  // Fixed-point positions (R = float only, see "position codec" below): q = rint((x - L/2) / qs), qs = L / 2^31
  double qs[3], qh[3];     // scale and half box edge (fp64: exact decoding)
  R qsf[3], qinvf[3];      // scale and 1 / scale in R (staging, integrator)
  // Tile widths along x (see tile_x0): the first xs_nb tiles of a row are HX cells wide, the others xs_w (1 or 2) cells.
  // xs_nb * HX >= nc[0]: all tiles HX wide.  Narrow tiles are the small change that fills the last round of a force launch.
  int xs_nb, xs_w;
};

// ---- position codec ------------------------------------------------------------------------------------------------
// fp64 build: x4 = (x, y, z, type) in real coordinates.
// fp32 build: x4.xyz carry the BIT PATTERNS of int32 fixed-point coordinates  q = rint((x - L/2) / qs),  qs = L / 2^31
//   (resolution 5e-8 at L = 108, uniform over the box; the box is q in [-2^30, 2^30), int32 leaves half a box of headroom
//   on either side for the drift between two rebuilds; one box length is 2^31, i.e. the periodic shift is a wrap of the
//   32-bit arithmetic).  x4.w stays the type as a float.  Why: an absolute fp32 coordinate at x ~ 100 has an ulp of 7.6e-6,
//   and that -- not the fp32 pair arithmetic -- set the force error at the headline size (2e-4 of the largest force at
//   L = 107.7; SURVEY App. E asks 1e-5).  The kernels that matter stage TILE-LOCAL coordinates: (q + shift - q_ref) is
//   exact in integers and only the small result (|u| <= 7.1) is rounded to fp32.  The integrator adds rint(dt v / qs).
constexpr int kQHalf = 1 << 30;
__device__ __forceinline__ int qbits(float v) { return __float_as_int(v); }
__device__ __forceinline__ float qmake(int q) { return __int_as_float(q); }
struct D3 { double x, y, z; };
// exact real coordinates
__device__ __forceinline__ D3 pos_real(const float4& p, const double* qs, const double* qh) {
  return {(double)qbits(p.x) * qs[0] + qh[0], (double)qbits(p.y) * qs[1] + qh[1], (double)qbits(p.z) * qs[2] + qh[2]};
}
__device__ __forceinline__ D3 pos_real(const double4& p, const double*, const double*) { return {p.x, p.y, p.z}; }
// real coordinates in R (fp32 build: absolute fp32, for the paths where that is enough: fall-back kernels, sub-bin keys)
__device__ __forceinline__ float4 pos_abs(const float4& p, const Box<float>& b) {
  return make_float4((float)((double)qbits(p.x) * b.qs[0] + b.qh[0]), (float)((double)qbits(p.y) * b.qs[1] + b.qh[1]),
                     (float)((double)qbits(p.z) * b.qs[2] + b.qh[2]), p.w);
}
__device__ __forceinline__ double4 pos_abs(const double4& p, const Box<double>&) { return p; }
// cell index along axis d (nc cells), the box being [0, L): exact integer arithmetic in the fp32 build
__device__ __forceinline__ int pos_cell(float c, int d, int nc, const Box<float>&) {
  const long long o = (long long)qbits(c) + kQHalf;
  int cc = (int)((o * nc) >> 31);
  return cc >= nc ? nc - 1 : (cc < 0 ? 0 : cc);
}
__device__ __forceinline__ int pos_cell(double c, int d, int nc, const Box<double>& b) {
  int cc = (int)(c * ((double)nc * b.invL[d]));
  return cc >= nc ? nc - 1 : (cc < 0 ? 0 : cc);
}
// fold coordinate d into the box, counting the images; returns true when the value changed
__device__ __forceinline__ bool pos_fold(float& c, int& img, int d, const Box<float>&) {
  int q = qbits(c);
  if (q >= kQHalf) { q = (int)((unsigned)q + 0x80000000u); img += 1; c = qmake(q); return true; }
  if (q < -kQHalf) { q = (int)((unsigned)q + 0x80000000u); img -= 1; c = qmake(q); return true; }
  return false;
}
__device__ __forceinline__ bool pos_fold(double& c, int& img, int d, const Box<double>& box) {
  bool moved = false;
  double s_ = floor(c * box.invL[d]);
  if (s_ != 0.0) { c -= s_ * box.L[d]; img += (int)s_; moved = true; }
  if (c >= box.L[d]) { c -= box.L[d]; img += 1; moved = true; }
  if (c < 0.0) { c += box.L[d]; img -= 1; moved = true; }
  return moved;
}
// x + dx (integrator drift)
__device__ __forceinline__ float pos_add(float c, float dx, float qinv) { return qmake(qbits(c) + __float2int_rn(dx * qinv)); }
__device__ __forceinline__ double pos_add(double c, double dx, double) { return c + dx; }
// a - b in real units (displacement since a snapshot)
__device__ __forceinline__ float pos_diff(float a, float b, float qs) { return (float)(qbits(a) - qbits(b)) * qs; }
__device__ __forceinline__ double pos_diff(double a, double b, double) { return a - b; }
// encoding of a real coordinate (descriptor tables: reference point of a tile) and of a periodic shift of k box lengths
__device__ __forceinline__ float pos_enc(double x, int d, const Box<float>& b) { return qmake((int)(long long)rint((x - b.qh[d]) / b.qs[d])); }
__device__ __forceinline__ double pos_enc(double x, int d, const Box<double>&) { return x; }
__device__ __forceinline__ float pos_shift(int k, int d, const Box<float>&) { return qmake((int)((unsigned)k << 31)); }     // +-1 box = 2^31: the same wrap
__device__ __forceinline__ double pos_shift(int k, int d, const Box<double>& b) { return (double)k * b.L[d]; }
// tile-local coordinate (p + shift) - ref as a float / double: integers in the fp32 build, only the small result is rounded
__device__ __forceinline__ float pos_local(float p, float shift, float ref, float qs) {
  return (float)(int)((unsigned)qbits(p) + (unsigned)qbits(shift) - (unsigned)qbits(ref)) * qs;
}
__device__ __forceinline__ double pos_local(double p, double shift, double ref, double) { return (p + shift) - ref; }
// minimum-image difference a - b along axis d (fall-back kernels that gather positions through global memory)
__device__ __forceinline__ float pos_delta(float a, float b, int d, const Box<float>& box) {
  int dq = (int)((unsigned)qbits(a) - (unsigned)qbits(b));
  if (dq >= kQHalf) dq = (int)((unsigned)dq + 0x80000000u); else if (dq < -kQHalf) dq = (int)((unsigned)dq + 0x80000000u);
  return (float)dq * box.qsf[d];
}
__device__ __forceinline__ double pos_delta(double a, double b, int d, const Box<double>& box) {
  const double x = a - b;
  return x - box.L[d] * rint(x * box.invL[d]);
}

// Non-bonded parameters of one type pair, pre-multiplied (gromacs_topology.py:715-721,
// doc/topology.rst:12-14).  PairCore is the only thing the LJ fast path touches (one 16-byte
// LDS read per pair in fp32); PairExt holds energy and table terms.
//   kind 1: ff = r^-6 (lj1 r^-6 - lj2) r^-2,  e = r^-6 (e1 r^-6 - e2) + shift
//   kind 2: linear table interpolation, rows (f_k, f_k+1 - f_k, e_k, e_k+1 - e_k)
//   kind 3: piecewise cubic (Akima / natural spline, fitted on the host: chem_tab_host.hpp), two rows per interval,
//           (f c0..c3) and (e c0..c3), y = c0 + w (c1 + w (c2 + w c3)); only the CUBIC instantiations know it
template <typename R> struct PairCore { R rc2, lj1, lj2, kind; };   // kind as R: 0 none (rc2<0), 1 LJ, 2 table, 3 cubic table
template <typename R> struct PairExt { R e1, e2, shift, r0, inv_dr; int toff, nrow, pad; };

// ---- helpers -------------------------------------------------------------------------
template <typename R> __device__ __forceinline__ R minimg1(R d, R L, R invL) { return d - L * rint_r(d * invL); }

__device__ __forceinline__ unsigned long long real_bits(float x) { return (unsigned long long)__float_as_uint(x); }
__device__ __forceinline__ unsigned long long real_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double bits_real_f(unsigned long long b) { return (double)__uint_as_float((unsigned)b); }
__device__ __forceinline__ double bits_real_d(unsigned long long b) { return __longlong_as_double((long long)b); }

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long lanemask_lt() {
  int l = lane_id();
  return l ? (~0ull >> (64 - l)) : 0ull;
}

// =======================================================================================
// K7/K8  velocity-Verlet halves (start_simulation.py:165-167,780)
// =======================================================================================
constexpr int kFoldSlots = 64;   // words of the atomic displacement fold of the decomposed path (k_integrate, k_pair_tiles guard 2)
template <typename R> struct LangevinP { int on; double kT, gamma, dt; uint64_t seed; uint64_t step; uint32_t phase;
  uint32_t tmask; };   // thermal groups (LangevinThermostat.add_valid_types, start_simulation.py:312-336): bit t set = type t is thermalised; 0 = every type

template <typename R>
__device__ __forceinline__ void langevin_force(const LangevinP<R>& lp, int tag, R mass, R vx, R vy, R vz, R& fx, R& fy, R& fz) {
  uint32_t r[4];
  chem_philox::langevin_draw(lp.seed, lp.step, lp.phase, (uint32_t)tag, r);
  double m = (double)mass;
  double pref = sqrt(24.0 * lp.kT * lp.gamma * m / lp.dt);
  fx += (R)(-lp.gamma * m * (double)vx + pref * (chem_philox::u01(r[0]) - 0.5));
  fy += (R)(-lp.gamma * m * (double)vy + pref * (chem_philox::u01(r[1]) - 0.5));
  fz += (R)(-lp.gamma * m * (double)vz + pref * (chem_philox::u01(r[2]) - 0.5));
}

// mode bits: 1 = second half-kick (integrate2), 2 = first half-kick + drift (integrate1),
// 3 = fused integrate2(step s) + integrate1(step s+1); 4 = add Langevin force to f first
// (thermalize at aftCalcF) and, when mode has no drift..., store f_total back.
// x0 != nullptr: rebuild criterion "displacement" (max |x - x_at_last_build|^2); nullptr: the
// reference's accumulated per-step maxima (max |dt v|^2 of this step)
template <typename R> struct PosScale { R s[3], inv[3]; };   // fixed-point scale of the positions (fp32 build; unused in fp64)
// Langevin piston (chem_barostat_langevin; PISTON instantiations only): sv multiplies the velocities in front of the first half
// kick (mode 2) and behind the second (mode 1); the drift is dt v / sqrt(mu) in the box before its scaling (rsmu = 1 / sqrt(mu)),
// which is also what the rebuild criterion sees.  The factors cost nothing next to the kernel's HBM traffic.
template <typename R> struct PistonP { R sv, rsmu; };
template <typename R, int MODE, bool LANG, bool STOREF, bool PISTON = false>
__global__ __launch_bounds__(256) void k_integrate(int n, Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4,
                                                    Vec4<R>* __restrict__ f4, const int* __restrict__ tag,
                                                    R dt, LangevinP<R> lp, unsigned long long* __restrict__ blockmax,
                                                    const Vec4<R>* __restrict__ x0, R cap, PosScale<R> ps, const DevCtl* __restrict__ ctl,
                                                    unsigned long long* __restrict__ foldmax = nullptr, PistonP<R> pp = PistonP<R>{}) {
  // foldmax (decomposed path): kFoldSlots words that collect the block maxima with one atomicMax per block (block b -> word
  // b % kFoldSlots: a few dozen atomics per address, spread over the launch) -- the one-block fold launch between this kernel
  // and the halo exchange is gone; the words travel with the halo, the force kernel's prologue takes the maximum and clears them
  // (single domain, fused rebuild, option skip_idle: the same fold into one of two sets of words, chosen by the host by the parity
  //  of the step's decision; the launch that decides -- k_rebuild_fused P0 or k_pair_tiles guard 3 -- reads it and clears the other)
  if (ctl->halt) return;   // (uniform scalar load; see DevCtl::halt)
  // kIntPerBlock particles per 256-thread block: every thread owns kIntPerBlock/256 particles and issues
  // all their loads before the first dependent instruction (more bytes in flight per wave for this
  // purely HBM-bound kernel); the arithmetic per particle is unchanged
  constexpr int PPT = kIntPerBlock / 256;
  const int base = blockIdx.x * kIntPerBlock + threadIdx.x;
  Vec4<R> vv[PPT], ff[PPT], xx[PPT];
  int tg[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int i = base + u * 256;
    tg[u] = 0;
    if (i < n) {
      vv[u] = v4[i]; ff[u] = f4[i];
      if (LANG) tg[u] = tag[i];
      if (MODE & 2) xx[u] = x4[i];
    }
  }
  R d2 = 0;
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int i = base + u * 256;
    if (i >= n) continue;
    Vec4<R> v = vv[u], f = ff[u];
    if (cap > (R)0) {   // CapForce: f4 holds the conservative force of this step (the host passes cap only then)
      const R f2 = f.x * f.x + f.y * f.y + f.z * f.z;
      if (f2 > cap * cap) { const R s = cap / sqrt_r(f2); f.x *= s; f.y *= s; f.z *= s; }
    }
    if (LANG) {
      bool on = true;
      if (lp.tmask) {   // (uniform branch; the second half kick alone does not load the position: the type comes from x4 then)
        const int ty = (int)((MODE & 2) ? xx[u].w : x4[i].w);
        on = (lp.tmask >> (ty & 31)) & 1u;
      }
      if (on) langevin_force<R>(lp, tg[u], v.w, v.x, v.y, v.z, f.x, f.y, f.z);
      if (STOREF) f4[i] = f;
    }
    R hm = (R)0.5 * dt / v.w;
    if (MODE & 1) { v.x += hm * f.x; v.y += hm * f.y; v.z += hm * f.z; }
    if (PISTON && MODE == 1) { v.x *= pp.sv; v.y *= pp.sv; v.z *= pp.sv; }
    if (PISTON && MODE == 2) { v.x *= pp.sv; v.y *= pp.sv; v.z *= pp.sv; }
    if (MODE & 2) {
      v.x += hm * f.x; v.y += hm * f.y; v.z += hm * f.z;
      Vec4<R> x = xx[u];
      R dx = dt * v.x, dy = dt * v.y, dz = dt * v.z;
      if (PISTON && MODE == 2) { dx *= pp.rsmu; dy *= pp.rsmu; dz *= pp.rsmu; }
      x.x = pos_add(x.x, dx, ps.inv[0]); x.y = pos_add(x.y, dy, ps.inv[1]); x.z = pos_add(x.z, dz, ps.inv[2]);
      x4[i] = x;
      if (x0) { const Vec4<R> o = x0[i]; dx = pos_diff(x.x, o.x, ps.s[0]); dy = pos_diff(x.y, o.y, ps.s[1]); dz = pos_diff(x.z, o.z, ps.s[2]); }
      const R dd = dx * dx + dy * dy + dz * dz;
      d2 = dd > d2 ? dd : d2;
    }
    v4[i] = v;
  }
  if (MODE & 2) {
    // max |dx|^2 of the block -> blockmax[blockIdx.x]; folded by k_rebuild_decide (no contended atomics)
    __shared__ unsigned long long wm[4];
    for (int o = 32; o > 0; o >>= 1) { R t = __shfl_xor(d2, o); d2 = t > d2 ? t : d2; }
    if (lane_id() == 0) wm[threadIdx.x >> 6] = real_bits(d2);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long m = wm[0];
      for (int k = 1; k < 4; ++k) m = wm[k] > m ? wm[k] : m;
      blockmax[blockIdx.x] = m;
      if (foldmax) atomicMax(&foldmax[blockIdx.x % kFoldSlots], m);
    }
  }
}

// ---- fixed distances (chem_fix_add; rule set in include/chem_mi355.h) -----------------------------------------------
// Behind every launch of k_integrate that drifts, while a live entry exists.  One lane per entry; anchor and target are found
// through rtag, so the array survives every resort.  Two 16-byte loads per particle (x4, v4), one 16-byte store each of the
// target's x4 and v4 (w = type / mass kept).  Entries of one anchor are consecutive (FixState::device_order): the anchor
// loads of neighbouring lanes hit one line.  The move is a displacement through pos_add, like the drift.
template <typename R> struct FixEnt;
template <> struct FixEnt<float> { int a, t; float d; int pad; };
template <> struct FixEnt<double> { int a, t; double d; };
template <typename R> struct FixGeom { R L[3], invL[3]; };      // (fp64 build only; the fp32 build wraps in fixed point)
__device__ __forceinline__ float fix_delta(float a, float b, float qs, float, float) {
  int dq = (int)((unsigned)qbits(a) - (unsigned)qbits(b));
  if (dq >= kQHalf || dq < -kQHalf) dq = (int)((unsigned)dq + 0x80000000u);
  return (float)dq * qs;
}
__device__ __forceinline__ double fix_delta(double a, double b, double, double L, double invL) { const double x = a - b; return x - L * rint(x * invL); }
// one entry: the target goes to x_a + d u / |u|, u the minimum image of x_t - x_a ((1, 0, 0) for |u| = 0), and takes the anchor's velocity
template <typename R>
__device__ __forceinline__ void fix_apply_entry(const FixEnt<R> e, const int* __restrict__ rtag, int ntag, Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4,
                                                const FixGeom<R>& g, const PosScale<R>& ps) {
  if ((unsigned)e.a >= (unsigned)ntag || (unsigned)e.t >= (unsigned)ntag) return;
  const int ia = rtag[e.a], it = rtag[e.t];
  if (ia < 0 || it < 0) return;
  const Vec4<R> xa = x4[ia], va = v4[ia];
  Vec4<R> xt = x4[it], vt = v4[it];
  const R rx = fix_delta(xt.x, xa.x, ps.s[0], g.L[0], g.invL[0]), ry = fix_delta(xt.y, xa.y, ps.s[1], g.L[1], g.invL[1]),
          rz = fix_delta(xt.z, xa.z, ps.s[2], g.L[2], g.invL[2]);
  const R r2 = rx * rx + ry * ry + rz * rz;
  R dx = e.d, dy = (R)0, dz = (R)0;      // |u| = 0: u = (1, 0, 0)
  if (r2 > (R)0) {
    const R s = e.d / sqrt_r(r2);
    dx = s * rx - rx; dy = s * ry - ry; dz = s * rz - rz;
  }
  xt.x = pos_add(xt.x, dx, ps.inv[0]); xt.y = pos_add(xt.y, dy, ps.inv[1]); xt.z = pos_add(xt.z, dz, ps.inv[2]);
  vt.x = va.x; vt.y = va.y; vt.z = va.z;
  x4[it] = xt; v4[it] = vt;
}
template <typename R>
__global__ __launch_bounds__(256) void k_fix_distances(int ne, const FixEnt<R>* __restrict__ ent, const int* __restrict__ rtag, int ntag,
                                                        Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4, FixGeom<R> g, PosScale<R> ps,
                                                        const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;   // (the drift in front of this launch left at once, too)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ne) return;
  fix_apply_entry<R>(ent[k], rtag, ntag, x4, v4, g, ps);
}
// Placement of the entries a reaction step has just joined (chem_reaction_join): the same move, once, at the reaction step and
// over the new entries only (targets are distinct, and no target is an anchor: the lanes write disjoint particles).  The host
// launches it behind a synchronised reaction step, in front of the forced rebuild, which then bins the target where it is.
template <typename R>
__global__ __launch_bounds__(256) void k_fix_place(int ne, const FixEnt<R>* __restrict__ ent, const int* __restrict__ rtag, int ntag,
                                                    Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4, FixGeom<R> g, PosScale<R> ps) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ne) return;
  fix_apply_entry<R>(ent[k], rtag, ntag, x4, v4, g, ps);
}

// one block: fold the step's per-block max displacement into the accumulated distance and
// decide whether the Verlet list must be rebuilt (VelocityVerlet::run).
// phase 3: both (single GPU); phase 1: fold only -> ctl->step_m2 (then max over ranks);
// phase 2: decide from ctl->step_m2.
template <typename R>
__global__ __launch_bounds__(1024) void k_rebuild_decide(DevCtl* ctl, unsigned long long* __restrict__ blockmax, int nblk, double half_skin, int criterion, int phase,
                                                         const double* __restrict__ gathered, int ngathered, volatile int* __restrict__ host_flag, int ticket,
                                                         double half_skin_ref) {      // (half_skin: the skin the lists were built for; _ref: the workload's, for the reported count)
  unsigned long long m = 0;
  if (phase & 1) {
    for (int k = threadIdx.x; k < nblk; k += 1024) { unsigned long long b = blockmax[k]; blockmax[k] = 0ull; m = b > m ? b : m; }
    for (int o = 32; o > 0; o >>= 1) { unsigned long long t = __shfl_xor(m, o); m = t > m ? t : m; }
  }
  __shared__ unsigned long long wm[16];
  if (lane_id() == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m2;
    if (phase & 1) {
      for (int k = 1; k < 16; ++k) m = wm[k] > m ? wm[k] : m;
      m2 = sizeof(R) == 4 ? bits_real_f(m) : bits_real_d(m);
      ctl->step_m2 = m2;
    } else if (gathered) { m2 = gathered[0]; for (int q = 1; q < ngathered; ++q) m2 = gathered[q] > m2 ? gathered[q] : m2; }
    else m2 = ctl->step_m2;
    if (phase & 2) {
      const int forced = ctl->force_rebuild;
      double acc = criterion ? sqrt(m2) : ctl->acc_maxdist + sqrt(m2);
      double accr = criterion ? sqrt(m2) : ctl->acc_ref + sqrt(m2);
      const int need = (acc > half_skin) || forced;
      if (need) { acc = 0.0; ctl->force_rebuild = 0; ctl->rebuild_count++; }
      if ((accr > half_skin_ref) || forced) { accr = 0.0; ctl->ref_rebuilds++; }      // the reference rule on the workload's skin
      ctl->acc_maxdist = acc; ctl->acc_ref = accr;
      ctl->need_rebuild = need;
      if (host_flag) {   // pinned, host-visible: [0] decision, [1] ticket (written last); the host spins on the ticket
        host_flag[0] = need;
        __threadfence_system();
        host_flag[1] = ticket;
      }
    }
  }
}

// device -> pinned host memory by a kernel (16-byte stores over PCIe): the copy engine's first
// transfer after a large allocation burst took 7 ms for 8 MB here
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
  for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < n16; k += (size_t)gridDim.x * blockDim.x) dst[k] = src[k];
}

// a handful of device integers to pinned host memory with ONE poll on the host (the slab rebuild
// used to read them with one blocking copy each): host[0] = ticket (written last), host[1..n] = values
struct CollectArgs { const int* src[8]; int n; };
__global__ void k_collect_ints(CollectArgs a, volatile int* host, int ticket) {
  if ((int)threadIdx.x < a.n) host[1 + threadIdx.x] = *a.src[threadIdx.x];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) host[0] = ticket;
}

// =======================================================================================
// K1  cell binning + canonical sort (storage.decompose(), start_simulation.py:158-171)
// =======================================================================================
// migration buffer of one direction (SoA, fixed capacity, count in front): particles that left the
// slab travel to the neighbour rank with their full state
template <typename R> struct MigBuf { int* count; Vec4<R>* x; Vec4<R>* v; int4* img; int* tag; int cap; };

// bucket != nullptr (fused rebuild): member `slot` of cell `cid` is recorded at bucket[cid * bcap + slot] right away
// (fixed-capacity rows), so that the sort phase needs no separate placement pass; cell_of / slot_of are not written.
template <typename R>
__device__ __forceinline__ void dev_bin(int i0, int n, Vec4<R>* x4, const Vec4<R>* v4, const int* tag, int4* img4, const Box<R>& box,
                                        int* cell_cnt, int* cell_of, int* slot_of, const MigBuf<R>& mdn, const MigBuf<R>& mup, DevCtl* ctl,
                                        int* bucket = nullptr, int bcap = 0, int* seg_tot = nullptr, int seg_shift = 0) {
  // Four particles per thread and trip, in three stages -- all position loads, then all slot atomics, then the stores --
  // so that a thread waits for ONE load and ONE returning atomic round trip per four particles instead of one each per
  // particle (the phase is a chain of dependent device-scope round trips, not bandwidth).
  // The trip bound is wave-uniform (rounded up) because the slot assignment uses cross-lane ops.
  constexpr int U = 4;
  const int iend = i0 + n;
  const int G = gridDim.x * blockDim.x;
  const int lane = lane_id();
  for (int ib0 = i0 + blockIdx.x * blockDim.x; ib0 < iend; ib0 += U * G) {
    Vec4<R> xs[U]; int4 ims[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = ib0 + u * G + (int)threadIdx.x;
      if (i < iend) { xs[u] = x4[i]; ims[u] = img4[i]; }
    }
    int cids[U], bases[U], starts[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = ib0 + u * G + (int)threadIdx.x;
      int cid = -1;                       // -1: lane idle or particle migrates away
      if (i < iend) {
        Vec4<R> x = xs[u];
        int4 im = ims[u];
        R* p = &x.x; int* ip = &im.x;
        int c[3];
        bool moved = false;   // folded back into the box: only then position and image counters are written back
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          moved |= pos_fold(p[d], ip[d], d, box);
          const int ncd = (d == 2 && box.zghost) ? box.nzg : (box.nc[d] > 0 ? box.nc[d] : 1);
          c[d] = pos_cell(p[d], d, ncd, box);
        }
        int dir = 0;   // 0 stays, -1 leaves downwards, +1 upwards
        if (box.zghost) {
          // c[2] is the global layer of the folded z; the slab owns layers [z0g, z0g + own)
          const int own = box.nc[2] - 2, gz = c[2];
          const int gu = (box.z0g + own) % box.nzg, gd = (box.z0g - 1 + box.nzg) % box.nzg;
          if (gz >= box.z0g && gz < box.z0g + own) c[2] = gz - box.z0g + 1;
          else if (gz == gu) dir = 1;
          else if (gz == gd) dir = -1;
          else { ctl->mig_error = 1; c[2] = 1; }   // moved by more than one layer: impossible within skin/2
        }
        if (moved) { x4[i] = x; img4[i] = im; }
        if (dir) {
          const MigBuf<R>& mb = dir < 0 ? mdn : mup;
          const int k = atomicAdd(mb.count, 1);
          if (k < mb.cap) { mb.x[k] = x; mb.v[k] = v4[i]; mb.img[k] = im; mb.tag[k] = tag[i]; } else ctl->mig_error = 2;
          cell_of[i] = -1;
        } else {
          cid = box.nc[0] > 0 ? (c[2] * box.nc[1] + c[1]) * box.nc[0] + c[0] : 0;
          if (!bucket) cell_of[i] = cid;
        }
      }
      cids[u] = cid;
    }
    // Slot inside the cell.  The arrays are still in the cell order of the previous rebuild, so
    // neighbouring lanes mostly share a cell: one atomic per run of equal cells in the wave
    // (run head adds the run length, the others take base + rank) instead of one per particle --
    // ~18 same-address atomics per cell were the whole cost of this kernel.
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cid = cids[u];
      const int prev = __shfl_up(cid, 1);
      const bool head = lane == 0 || prev != cid;
      const unsigned long long hm = __ballot(head);
      const unsigned long long upto = hm & (~0ull >> (63 - lane));          // heads at lanes <= lane
      const int start = 63 - __clzll((long long)upto);
      const unsigned long long above = lane == 63 ? 0ull : (hm >> (lane + 1));
      const int end = above ? lane + __ffsll((long long)above) : 64;        // first head after this lane
      int base = 0;
      if (head && cid >= 0) base = atomicAdd(&cell_cnt[cid], end - start);
      bases[u] = base; starts[u] = start;
      if (seg_tot) {
        // particles per segment of 2^seg_shift cells (fused rebuild): one atomic per run of equal SEGMENTS in the wave
        // (a wave usually sits inside one segment; per-cell-run atomics on the same word serialise in the L2)
        const int sg = cid >= 0 ? cid >> seg_shift : -1;
        const int sprev = __shfl_up(sg, 1);
        const bool shead = lane == 0 || sprev != sg;
        const unsigned long long shm = __ballot(shead);
        const unsigned long long sabove = lane == 63 ? 0ull : (shm >> (lane + 1));
        const int send = sabove ? lane + __ffsll((long long)sabove) : 64;
        if (shead && sg >= 0) atomicAdd(&seg_tot[sg], send - lane);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = ib0 + u * G + (int)threadIdx.x;
      const int cid = cids[u];
      const int base = __shfl(bases[u], starts[u]);
      if (cid >= 0) {
        const int slot = base + (lane - starts[u]);
        if (!bucket) slot_of[i] = slot;
        else if (slot < bcap) bucket[(size_t)cid * bcap + slot] = i;
        else atomicMax(&ctl->bucket_overflow, slot + 1);
      }
    }
  }
}

template <typename R>
__global__ __launch_bounds__(256) void k_bin(int i0, int n, Vec4<R>* __restrict__ x4, const Vec4<R>* __restrict__ v4, const int* __restrict__ tag,
                                             int4* __restrict__ img4, Box<R> box,
                                             int* __restrict__ cell_cnt, int* __restrict__ cell_of,
                                             int* __restrict__ slot_of, MigBuf<R> mdn, MigBuf<R> mup, DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  dev_bin<R>(i0, n, x4, v4, tag, img4, box, cell_cnt, cell_of, slot_of, mdn, mup, ctl);
}

// arrivals of a migration exchange are appended behind the current particles
template <typename R>
__global__ __launch_bounds__(256) void k_append_arrivals(MigBuf<R> in, int count, int dst0, Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4,
                                                        int* __restrict__ tag, int4* __restrict__ img4) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  x4[dst0 + k] = in.x[k]; v4[dst0 + k] = in.v[k]; tag[dst0 + k] = in.tag[k]; img4[dst0 + k] = in.img[k];
}

// single-block exclusive scan of cell counts -> cell_start[0..ncell]; zeroes cell_cnt for next time.
// Each of the 16 waves scans one contiguous 1/16 of the cells with wave shuffles only (running
// carry, four 256-cell groups in flight, no block barrier in the loop), then one barrier publishes
// the wave totals and a second sweep adds each wave's offset to what it wrote.
__global__ __launch_bounds__(1024) void k_scan_cells(int ncell, int base0, int* __restrict__ cell_cnt, int* __restrict__ cell_start,
                                                     const DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  __shared__ int wsum[16];
  const int w = threadIdx.x >> 6, lane = lane_id();
  const int per = (((ncell + 15) >> 4) + 255) & ~255;
  const int lo = w * per, hi = min(ncell, lo + per);
  constexpr int U = 4;
  int carry = 0;
  for (int b = lo; b < hi; b += 256 * U) {
    int v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i0 = b + u * 256 + lane * 4;
      if (i0 + 3 < hi) {
        const int4 t = *reinterpret_cast<const int4*>(cell_cnt + i0);
        v[u][0] = t.x; v[u][1] = t.y; v[u][2] = t.z; v[u][3] = t.w;
        *reinterpret_cast<int4*>(cell_cnt + i0) = make_int4(0, 0, 0, 0);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[u][k] = 0; if (i0 + k < hi) { v[u][k] = cell_cnt[i0 + k]; cell_cnt[i0 + k] = 0; } }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i0 = b + u * 256 + lane * 4;
      const int sum = v[u][0] + v[u][1] + v[u][2] + v[u][3];
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
      int run = carry + incl - sum;
      if (i0 + 3 < hi) {
        int4 o4; o4.x = run; o4.y = run + v[u][0]; o4.z = o4.y + v[u][1]; o4.w = o4.z + v[u][2];
        *reinterpret_cast<int4*>(cell_start + i0) = o4;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (i0 + k < hi) cell_start[i0 + k] = run; run += v[u][k]; }
      }
      carry += __shfl(incl, 63);
    }
  }
  if (lane == 0) wsum[w] = carry;
  __syncthreads();
  int off = base0, tot = base0;
  for (int k = 0; k < 16; ++k) { if (k < w) off += wsum[k]; tot += wsum[k]; }
  if (off != 0) {
    for (int i0 = lo + lane * 4; i0 < hi; i0 += 256) {
      if (i0 + 3 < hi) {
        int4 t = *reinterpret_cast<int4*>(cell_start + i0);
        t.x += off; t.y += off; t.z += off; t.w += off;
        *reinterpret_cast<int4*>(cell_start + i0) = t;
      } else {
        for (int k = 0; k < 4; ++k) if (i0 + k < hi) cell_start[i0 + k] += off;
      }
    }
  }
  if (threadIdx.x == 0) cell_start[ncell] = tot;
}

__global__ __launch_bounds__(256) void k_place(int i0, int n, const int* __restrict__ cell_of, const int* __restrict__ slot_of,
                                               const int* __restrict__ cell_start, int* __restrict__ perm, const DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  for (int i = i0 + blockIdx.x * blockDim.x + threadIdx.x; i < i0 + n; i += gridDim.x * blockDim.x) {
    const int c = cell_of[i];
    if (c >= 0) perm[cell_start[c] + slot_of[i]] = i;   // c < 0: migrated away
  }
}

// One wave per cell: rank the members by (x sub-bin, tag) -- a canonical order inside a cell, so the whole
// pipeline is run-to-run deterministic -- and gather the particle arrays into cell-sorted order.
// The cell is cut into NSUB slices along x; cell_sub[c] packs the number of members in front of slice
// 1, 2, 3 (8 bits each): the list build uses it to test only the x-window of a stencil row that can hold
// neighbours of a given home particle (dev_nlist_tile).  Crowded cells (> 64 members) keep plain tag
// order and store -1 ("no sub-bin information": the list build then takes the whole cell).
constexpr int NSUB = 4;
// key = x slice (2 bits) | y half | z half | tag: x-major so that cell_sub stays a prefix over the x slices; the
// y/z halves make neighbouring lanes of the force kernel (consecutive home particles) spatial neighbours, whose
// slot-sorted lists then read nearby LDS slots in the same instruction (fewer bank conflicts, more broadcasts)
template <typename R>
__device__ __forceinline__ int sort_key(const Vec4<R>& xq, int c, const Box<R>& box, int tg) {
  const Vec4<R> x = pos_abs(xq, box);   // (slices and halves only order the cell and prune windows: absolute fp32 is enough)
  const int nx = box.nc[0] > 0 ? box.nc[0] : 1, ny = box.nc[1] > 0 ? box.nc[1] : 1, nz = box.nc[2] > 0 ? box.nc[2] : 1;
  const int cx = c % nx, cy = (c / nx) % ny;
  const R clx = box.L[0] / (R)nx, cly = box.L[1] / (R)ny;
  int b = (int)((x.x - (R)cx * clx) * ((R)NSUB / clx));
  b = b < 0 ? 0 : (b > NSUB - 1 ? NSUB - 1 : b);
  const int hy = (x.y - (R)cy * cly) * (R)2 >= cly ? 1 : 0;
  // z: the half is taken from the fractional cell coordinate (slab mode shifts the layer index, not the split)
  const R zc = x.z * box.cell_inv[2];
  const int hz = (zc - floor_r(zc)) >= (R)0.5 ? 1 : 0;
  (void)nz;
  return (b << 29) | (hy << 28) | (hz << 27) | tg;     // tags < 2^27 (chem_set_particles)
}
template <typename R>
__device__ __forceinline__ void dev_sort_gather(int ncell, const int* cell_start, const int* perm, const Vec4<R>* x4, const Vec4<R>* v4,
                                                const int* tag, const int4* img4, Vec4<R>* x4o, Vec4<R>* v4o, int* tago, int4* img4o,
                                                const Box<R>& box, int* cell_sub) {
  // Two cells per wave (one per half-wave, width-32 shuffles) while both have <= 32 members -- the mean
  // occupancy is ~18 -- otherwise one cell per wave / the global-memory ranking for crowded cells.
  const int l = lane_id(), hl = l & 31, half = l >> 5;
  const int nw = gridDim.x * (blockDim.x >> 6);
  for (int c0 = 2 * (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); c0 < ncell; c0 += 2 * nw) {
    const int s0 = cell_start[c0], s1 = cell_start[c0 + 1], s2 = c0 + 1 < ncell ? cell_start[c0 + 2] : s1;
    const int cnt0 = s1 - s0, cnt1 = s2 - s1;
    if (cnt0 <= 32 && cnt1 <= 32) {
      const int s = half ? s1 : s0, cnt = half ? cnt1 : cnt0, cmax = cnt0 > cnt1 ? cnt0 : cnt1;
      const int cc = c0 + half;
      int pi = 0, tg = 0, key = 0x7fffffff;
      Vec4<R> xp = mk4<R>(0, 0, 0, 0);
      if (hl < cnt) { pi = perm[s + hl]; tg = tag[pi]; xp = x4[pi]; key = sort_key<R>(xp, cc, box, tg); }
      int rank = 0;
      for (int k = 0; k < cmax; ++k) { const int tk = __shfl(key, k, 32); rank += (k < cnt && tk < key) ? 1 : 0; }
      // members in front of slice 1, 2, 3 (per half-wave)
      const int bin = key >> 29;
      unsigned int packed = 0;
#pragma unroll
      for (int b = 1; b < NSUB; ++b) {
        const unsigned long long m = __ballot(hl < cnt && bin < b);
        packed |= (unsigned int)__popc((unsigned int)(half ? (m >> 32) : m)) << (8 * (b - 1));
      }
      if (hl == 0 && cc < ncell && cell_sub) cell_sub[cc] = (int)packed;
      if (hl < cnt) {
        const int dst = s + rank;
        x4o[dst] = xp; v4o[dst] = v4[pi]; tago[dst] = tg; img4o[dst] = img4[pi];
      }
      continue;
    }
    for (int cc = c0; cc < c0 + 2 && cc < ncell; ++cc) {
      const int s = cell_start[cc], cnt = cell_start[cc + 1] - s;
      if (cnt <= 64) {
        int pi = 0, tg = 0, key = 0x7fffffff;
        Vec4<R> xp = mk4<R>(0, 0, 0, 0);
        if (l < cnt) { pi = perm[s + l]; tg = tag[pi]; xp = x4[pi]; key = sort_key<R>(xp, cc, box, tg); }
        int rank = 0;
        for (int k = 0; k < cnt; ++k) { const int tk = __shfl(key, k); rank += (tk < key) ? 1 : 0; }
        const int bin = key >> 29;
        unsigned int packed = 0;
#pragma unroll
        for (int b = 1; b < NSUB; ++b) packed |= (unsigned int)__popcll(__ballot(l < cnt && bin < b)) << (8 * (b - 1));
        if (l == 0 && cell_sub) cell_sub[cc] = (int)packed;
        if (l < cnt) {
          const int dst = s + rank;
          x4o[dst] = xp; v4o[dst] = v4[pi]; tago[dst] = tg; img4o[dst] = img4[pi];
        }
      } else {
        // crowded cell: each lane ranks its members against all others through global memory (tag order)
        if (l == 0 && cell_sub) cell_sub[cc] = -1;
        for (int a = l; a < cnt; a += 64) {
          const int pi = perm[s + a], tg = tag[pi];
          int rank = 0;
          for (int k = 0; k < cnt; ++k) rank += (tag[perm[s + k]] < tg) ? 1 : 0;
          const int dst = s + rank;
          x4o[dst] = x4[pi]; v4o[dst] = v4[pi]; tago[dst] = tg; img4o[dst] = img4[pi];
        }
      }
    }
  }
}

// Fused-rebuild variant: members come from the fixed-capacity bucket rows filled while binning.  A cell's first index
// = offset of its segment (s_off, from the per-segment totals of the binning pass) + the counts of the cells in front
// of it inside the segment (<= 63 values: one load per lane and a wave reduction) -- no separate scan phase; it is
// published as cell_start, and the tag -> index map is written with the gather.  <= 64 members per cell (checked at
// binning time).
template <typename R>
__device__ __forceinline__ void dev_sort_gather_bucket(int ncell, const int* cell_cnt, const int* s_off, int seg_shift,
                                                       const int* bucket, int bcap, int* cell_start, const Vec4<R>* x4, const Vec4<R>* v4,
                                                       const int* tag, const int4* img4, Vec4<R>* x4o, Vec4<R>* v4o, int* tago, int4* img4o,
                                                       int* rtag, const Box<R>& box, int* cell_sub) {
  const int l = lane_id(), hl = l & 31, half = l >> 5;
  const int nw = gridDim.x * (blockDim.x >> 6);
  const int per = 1 << seg_shift;
  for (int c0 = 2 * (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); c0 < ncell; c0 += 2 * nw) {
    const bool two = c0 + 1 < ncell;
    // c0 is even and segments hold an even number (>= 2) of cells: c0 and c0 + 1 share a segment
    const int seg = c0 >> seg_shift, lo = seg << seg_shift;
    int before = 0;
    for (int k = lo + l; k < c0; k += 64) before += cell_cnt[k];     // per <= 64: one trip
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    (void)per;
    const int cnt0 = cell_cnt[c0], cnt1 = two ? cell_cnt[c0 + 1] : 0;
    const int s0 = s_off[seg] + before, s1 = s0 + cnt0;
    if (l == 0) { cell_start[c0] = s0; if (two) cell_start[c0 + 1] = s1; }
    if (cnt0 <= 32 && cnt1 <= 32) {
      const int s = half ? s1 : s0, cnt = half ? cnt1 : cnt0, cmax = cnt0 > cnt1 ? cnt0 : cnt1;
      const int cc = c0 + half;
      int pi = 0, tg = 0, key = 0x7fffffff;
      Vec4<R> xp = mk4<R>(0, 0, 0, 0);
      if (hl < cnt) { pi = bucket[(size_t)cc * bcap + hl]; tg = tag[pi]; xp = x4[pi]; key = sort_key<R>(xp, cc, box, tg); }
      int rank = 0;
      for (int k = 0; k < cmax; ++k) { const int tk = __shfl(key, k, 32); rank += (k < cnt && tk < key) ? 1 : 0; }
      const int bin = key >> 29;
      unsigned int packed = 0;
#pragma unroll
      for (int b = 1; b < NSUB; ++b) {
        const unsigned long long m = __ballot(hl < cnt && bin < b);
        packed |= (unsigned int)__popc((unsigned int)(half ? (m >> 32) : m)) << (8 * (b - 1));
      }
      if (hl == 0 && cc < ncell) cell_sub[cc] = (int)packed;
      if (hl < cnt) {
        const int dst = s + rank;
        x4o[dst] = xp; v4o[dst] = v4[pi]; tago[dst] = tg; img4o[dst] = img4[pi]; rtag[tg] = dst;
      }
      continue;
    }
    for (int cc = c0; cc < c0 + 2 && cc < ncell; ++cc) {
      const int s = cc == c0 ? s0 : s1, cnt = min(cc == c0 ? cnt0 : cnt1, 64);
      int pi = 0, tg = 0, key = 0x7fffffff;
      Vec4<R> xp = mk4<R>(0, 0, 0, 0);
      if (l < cnt) { pi = bucket[(size_t)cc * bcap + l]; tg = tag[pi]; xp = x4[pi]; key = sort_key<R>(xp, cc, box, tg); }
      int rank = 0;
      for (int k = 0; k < cnt; ++k) { const int tk = __shfl(key, k); rank += (tk < key) ? 1 : 0; }
      const int bin = key >> 29;
      unsigned int packed = 0;
#pragma unroll
      for (int b = 1; b < NSUB; ++b) packed |= (unsigned int)__popcll(__ballot(l < cnt && bin < b)) << (8 * (b - 1));
      if (l == 0) cell_sub[cc] = (int)packed;
      if (l < cnt) {
        const int dst = s + rank;
        x4o[dst] = xp; v4o[dst] = v4[pi]; tago[dst] = tg; img4o[dst] = img4[pi]; rtag[tg] = dst;
      }
    }
  }
}

template <typename R>
__global__ __launch_bounds__(256) void k_sort_gather(int ncell, const int* __restrict__ cell_start, const int* __restrict__ perm,
                                                     const Vec4<R>* __restrict__ x4, const Vec4<R>* __restrict__ v4,
                                                     const int* __restrict__ tag, const int4* __restrict__ img4,
                                                     Vec4<R>* __restrict__ x4o, Vec4<R>* __restrict__ v4o,
                                                     int* __restrict__ tago, int4* __restrict__ img4o, const DevCtl* ctl, Box<R> box, int* __restrict__ cell_sub) {
  if (!ctl->need_rebuild) return;
  dev_sort_gather<R>(ncell, cell_start, perm, x4, v4, tag, img4, x4o, v4o, tago, img4o, box, cell_sub);
}

template <typename R>
__global__ __launch_bounds__(256) void k_copyback(const int* __restrict__ cell_start, int c_first, int c_last, const Vec4<R>* __restrict__ x4o, const Vec4<R>* __restrict__ v4o,
                                                  const int* __restrict__ tago,
                                                  const int4* __restrict__ img4o, Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4,
                                                  int* __restrict__ tag, int4* __restrict__ img4,
                                                  int* __restrict__ rtag, Vec4<R>* __restrict__ x0, const DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  const int kbeg = cell_start[c_first], kend = cell_start[c_last];   // the own (non-ghost) cells
  for (int k = kbeg + blockIdx.x * blockDim.x + threadIdx.x; k < kend; k += gridDim.x * blockDim.x) {
    const Vec4<R> xk = x4o[k];
    x4[k] = xk; if (x0) x0[k] = xk;
    v4[k] = v4o[k]; img4[k] = img4o[k];
    int t = tago[k]; tag[k] = t; rtag[t] = k;
  }
}

// ---- slab decomposition: ghost layers --------------------------------------------------
// per-cell counts of the two boundary layers (what the neighbours need to lay out their ghosts)
__global__ __launch_bounds__(256) void k_layer_counts(int nxy, int own_layers, const int* __restrict__ cell_start,
                                                      int* __restrict__ cnt_dn, int* __restrict__ cnt_up) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > nxy) return;
  const int c1 = nxy, cn = own_layers * nxy;   // first cell of own layer 1 / of the last own layer
  if (k < nxy) { cnt_dn[k] = cell_start[c1 + k + 1] - cell_start[c1 + k]; cnt_up[k] = cell_start[cn + k + 1] - cell_start[cn + k]; }
  else { cnt_dn[nxy] = cell_start[c1 + nxy] - cell_start[c1]; cnt_up[nxy] = cell_start[cn + nxy] - cell_start[cn]; }
}

// cell_start of the two ghost layers from the neighbours' per-cell counts (single block):
// lower ghosts are right-aligned in front of the reals, upper ghosts follow them
__global__ __launch_bounds__(1024) void k_ghost_cells(int nxy, int own_layers, const int* __restrict__ gcnt_lo, const int* __restrict__ gcnt_up,
                                                      int* __restrict__ cell_start) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int c_up = (own_layers + 1) * nxy;
  for (int pass = 0; pass < 2; ++pass) {
    const int* cnt = pass ? gcnt_up : gcnt_lo;
    const int base_cell = pass ? c_up : 0;
    const int start = pass ? cell_start[c_up] : cell_start[nxy] - gcnt_lo[nxy];   // upper ghosts begin where the reals end
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int w = threadIdx.x >> 6;
    for (int b = 0; b < nxy; b += 1024) {
      const int i = b + threadIdx.x;
      const int v = i < nxy ? cnt[i] : 0;
      int incl = v;
      for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o); if (lane_id() >= o) incl += t; }
      if (lane_id() == 63) wsum[w] = incl;
      __syncthreads();
      int woff = 0, tot = 0;
      for (int k = 0; k < 16; ++k) { if (k < w) woff += wsum[k]; tot += wsum[k]; }
      if (i < nxy) cell_start[base_cell + i] = start + carry_s + woff + incl - v;
      __syncthreads();
      if (threadIdx.x == 0) carry_s += tot;
      __syncthreads();
    }
    if (pass && threadIdx.x == 0) cell_start[c_up + nxy] = start + carry_s;
    __syncthreads();
  }
}

// rtag for ghost copies (only where the particle is not owned here)
// gtag: the ghost copy of every tag that has one here, owned or not (a one-rank slab holds a real particle AND its ghost).
// One launch for both ghost ranges: [g0a, g0a + nga) in front of the reals, [g0b, g0b + ngb) behind them.
__global__ __launch_bounds__(256) void k_ghost_rtag(int g0a, int nga, int g0b, int ngb, const int* __restrict__ tag, int* __restrict__ rtag, int* __restrict__ gtag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nga + ngb) return;
  const int g = k < nga ? g0a + k : g0b + (k - nga);
  const int t = tag[g];
  atomicCAS(&rtag[t], -1, g);
  gtag[t] = g;
}
// first launch of a slab rebuild: the request is being served (need_rebuild on for the chain's kernels, force_rebuild off -- the
// force kernel's decision only reads it), headers of the two migration buffers cleared -- one launch instead of four memsets
__global__ void k_dd_begin(DevCtl* ctl, int* __restrict__ mig_dn, int* __restrict__ mig_up) {
  const int t = threadIdx.x;
  if (t == 0) { ctl->need_rebuild = 1; ctl->force_rebuild = 0; }
  if (t < 4) { mig_dn[t] = 0; mig_up[t] = 0; }
}
// what a slab rebuild clears before the sorted copies come back: the tag maps, and the x sub-bin words of the two ghost
// layers (filled by the neighbours' particles afterwards: no sub-bin information for their cells) -- one launch
__global__ __launch_bounds__(256) void k_dd_clear(int* __restrict__ rtag, int* __restrict__ gtag, int nglob, int* __restrict__ sub_lo, int* __restrict__ sub_hi, int nxy) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nglob) { rtag[k] = -1; gtag[k] = -1; }
  if (k < nxy) { sub_lo[k] = -1; sub_hi[k] = -1; }
}

// =======================================================================================
// K2  Verlet neighbour-list build (VerletList(system, cutoff, exclusionlist),
//     start_simulation.py:193-197).  One workgroup per home cell: the 27-cell stencil is
//     staged in LDS with the periodic shift applied, each wave then owns home particles and
//     tests 64 staged candidates per instruction; __ballot + popcount compacts the hits into
//     the particle's row with coalesced stores.
// =======================================================================================
__device__ __forceinline__ float idx_as_real(int i, float) { return __int_as_float(i); }
__device__ __forceinline__ double idx_as_real(int i, double) { return __longlong_as_double((long long)i); }
__device__ __forceinline__ int real_as_idx(float w) { return __float_as_int(w); }
__device__ __forceinline__ int real_as_idx(double w) { return (int)__double_as_longlong(w); }

// rows are padded with the particle's own index up to a multiple of 4 entries so that the
// force kernel can read them as int4 (the self entry has r = 0 and is masked there)
__device__ __forceinline__ void finish_row(int* row, int* nn, int p, int cnt, int S, int l, DevCtl* ctl) {
  const int c = cnt < S ? cnt : S;
  const int pad = (4 - (c & 3)) & 3;
  if (l < pad) row[c + l] = p;
  if (l == 0) { nn[p] = c; if (cnt > S) atomicMax(&ctl->nl_overflow, cnt); }
}

template <typename R, int CAP>
__global__ __launch_bounds__(256) void k_nlist_cells(int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                     const int* __restrict__ cell_start, Box<R> box, R rl2,
                                                     const int* __restrict__ excl_start, const int* __restrict__ excl_list,
                                                     int has_excl, int* __restrict__ nlist, int* __restrict__ nn, int S,
                                                     DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  __shared__ Vec4<R> sx[CAP];          // (x, y, z, bits of the global index), periodic shift applied
  __shared__ int seg_start[27], seg_cnt[27], seg_off[28];
  __shared__ R seg_shift[27][3];
  const int nx = box.nc[0], ny = box.nc[1], nz = box.nc[2];
  const int w = threadIdx.x >> 6, l = lane_id();
  for (int c = blockIdx.x; c < box.ncell; c += gridDim.x) {
    const int cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
    __syncthreads();   // previous cell's tile fully consumed
    if (threadIdx.x < 27) {
      int k = threadIdx.x;
      int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
      int ox = cx + dx, oy = cy + dy, oz = cz + dz;
      R sh[3] = {0, 0, 0};
      if (ox < 0) { ox += nx; sh[0] = -box.L[0]; } else if (ox >= nx) { ox -= nx; sh[0] = box.L[0]; }
      if (oy < 0) { oy += ny; sh[1] = -box.L[1]; } else if (oy >= ny) { oy -= ny; sh[1] = box.L[1]; }
      if (oz < 0) { oz += nz; sh[2] = -box.L[2]; } else if (oz >= nz) { oz -= nz; sh[2] = box.L[2]; }
      int oc = (oz * ny + oy) * nx + ox;
      seg_start[k] = cell_start[oc];
      seg_cnt[k] = cell_start[oc + 1] - cell_start[oc];
      seg_shift[k][0] = sh[0]; seg_shift[k][1] = sh[1]; seg_shift[k][2] = sh[2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int o = 0;
      for (int k = 0; k < 27; ++k) { seg_off[k] = o; o += seg_cnt[k]; }
      seg_off[27] = o;
    }
    __syncthreads();
    const int total_all = seg_off[27];
    const int hs = cell_start[c], he = cell_start[c + 1];
    // A stencil that holds more than CAP particles (dense systems that have left the LDS tiles) is walked in windows of
    // CAP slots; a home particle's running count waits in nn[] between two windows (written and read back by lane 0 of
    // the wave that owns the particle).
    for (int base = 0; base < total_all || base == 0; base += CAP) {
      if (base) __syncthreads();
      const int total = min(total_all - base, CAP);
      // stage: one wave per stencil cell round-robin, coalesced 16/32-byte loads
      for (int k = w; k < 27; k += 4) {
        const int s0 = seg_start[k], cnt = seg_cnt[k], o0 = seg_off[k] - base;
        const R sh0 = seg_shift[k][0], sh1 = seg_shift[k][1], sh2 = seg_shift[k][2];
        for (int t = l; t < cnt; t += 64) {
          const int dst = o0 + t;
          if (dst >= 0 && dst < CAP) {
            Vec4<R> p = pos_abs(x4[s0 + t], box);
            p.x += sh0; p.y += sh1; p.z += sh2; p.w = idx_as_real(s0 + t, (R)0);
            sx[dst] = p;
          }
        }
      }
      __syncthreads();
      const bool last = base + CAP >= total_all;
      for (int p = hs + w; p < he; p += 4) {
        const Vec4<R> xi = pos_abs(x4[p], box);
        int e0 = 0, e1 = 0;
        if (has_excl) { int tg = tag[p]; e0 = excl_start[tg]; e1 = excl_start[tg + 1]; }
        int cnt = 0;
        if (base) { if (l == 0) cnt = nn[p]; cnt = __shfl(cnt, 0); }
        int* row = nlist + (size_t)p * S;
        for (int s0 = 0; s0 < total; s0 += 64) {
          const int s = s0 + l;
          bool ok = s < total;
          int j = -1;
          if (ok) {
            const Vec4<R> xj = sx[s];
            j = real_as_idx(xj.w);
            const R dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            const R r2 = dx * dx + dy * dy + dz * dz;
            ok = (r2 <= rl2) && (j != p);
            if (ok && e1 > e0) {
              const int tj = tag[j];
              for (int e = e0; e < e1; ++e) if (excl_list[e] == tj) { ok = false; break; }
            }
          }
          const unsigned long long m = __ballot(ok);
          if (ok) {
            const int pos = cnt + __popcll(m & lanemask_lt());
            if (pos < S) row[pos] = j;
          }
          cnt += __popcll(m);
        }
        if (last) finish_row(row, nn, p, cnt, S, l, ctl);
        else if (l == 0) nn[p] = cnt;
      }
    }
  }
}

// brute-force variant for boxes with fewer than 3 cells per axis (tiny test systems):
// one wave per particle, all other particles are candidates, minimum image.
template <typename R>
__global__ __launch_bounds__(256) void k_nlist_brute(int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                     Box<R> box, R rl2, const int* __restrict__ excl_start,
                                                     const int* __restrict__ excl_list, int has_excl,
                                                     int* __restrict__ nlist, int* __restrict__ nn, int S, DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const int l = lane_id();
  const Vec4<R> xi = x4[p];
  int e0 = 0, e1 = 0;
  if (has_excl) { int tg = tag[p]; e0 = excl_start[tg]; e1 = excl_start[tg + 1]; }
  int cnt = 0;
  int* row = nlist + (size_t)p * S;
  for (int s0 = 0; s0 < n; s0 += 64) {
    const int j = s0 + l;
    bool ok = j < n && j != p;
    if (ok) {
      const Vec4<R> xj = x4[j];
      const R dx = pos_delta(xi.x, xj.x, 0, box), dy = pos_delta(xi.y, xj.y, 1, box), dz = pos_delta(xi.z, xj.z, 2, box);
      ok = dx * dx + dy * dy + dz * dz <= rl2;
      if (ok && e1 > e0) {
        const int tj = tag[j];
        for (int e = e0; e < e1; ++e) if (excl_list[e] == tj) { ok = false; break; }
      }
    }
    const unsigned long long m = __ballot(ok);
    if (ok) { const int pos = cnt + __popcll(m & lanemask_lt()); if (pos < S) row[pos] = j; }
    cnt += __popcll(m);
  }
  finish_row(row, nn, p, cnt, S, l, ctl);
}

// =======================================================================================
// K3  non-bonded pair forces over the Verlet list (VerletListLennardJones /
//     VerletListTabulated, gromacs_topology.py:511-512,696-721).  TPP lanes cooperate on one
//     particle: lane t handles neighbours t, t+TPP, ...; partial forces are combined with a
//     segmented xor-shuffle reduction.  Full list => no atomics, deterministic sums.
// =======================================================================================
// Truncated Coulomb term (VerletListCoulombTruncated, gromacs_topology.py:866-878; rule set in include/chem_mi355.h):
// U = k qi qj / r, F_i = k qi qj r_ij / r^3 for r^2 <= rc_qq^2, unshifted, on top of the pair's LJ / table term.  One
// (k, rc_qq) for all type pairs; mask[ti] bit tj = the pair carries the term; charges by tag.
template <typename R> struct CoulArgs { const R* qtag; const int* tag; const unsigned int* mask; double* eout; R k, rc2; };
__device__ __forceinline__ float rsqrt_r(float x) { return __builtin_amdgcn_rsqf(x); }   // 1 ulp
__device__ __forceinline__ double rsqrt_r(double x) { return 1.0 / sqrt(x); }
// kqi = k * qi of the home particle; on = the type pair's mask bit
template <typename R, bool ENERGY>
__device__ __forceinline__ void coul_term(R kqi, R qj, bool on, R rc2, R r2, R dx, R dy, R dz, R& fx, R& fy, R& fz, double& e_q, double& v_q) {
  if (on && r2 <= rc2) {
    const R ri = rsqrt_r(r2);
    const R e = kqi * qj * ri, ff = e * ri * ri;
    fx += ff * dx; fy += ff * dy; fz += ff * dz;
    if (ENERGY) { e_q += (double)e; v_q += (double)(ff * r2); }
  }
}

// Per-particle resolution lambda (VerletListDynamicResolutionLennardJones / ...Tabulated + BasicDynamicResolution; rule set in
// include/chem_mi355.h, chem_nb_resolution): the LJ / table force of a MARKED type pair is scaled by w = lambda_i lambda_j and
// then capped at fmax (> 0), its energy by w.  lambda is a pure function of the by-tag stamp (lambda0, s0), the rate of the
// particle's current type and the step of the forces (chem_res_host.hpp res_lambda: the same expression, unfused):
// nothing is updated per step.  mask[ti] bit tj = the pair is marked; fmax[ti * kMaxTypes + tj] its cap (0 = none), staged in LDS
// beside the pairs' other parameters (res_stage_caps).
template <typename R> struct ResArgs { const double2* stamp; const double* alpha; const int* tag; const unsigned int* mask; const R* fmax; long long step; };
__device__ __forceinline__ double res_lambda_dev(const double2* __restrict__ stamp, const double* __restrict__ alpha, long long step, int tg, int ty) {
#pragma clang fp contract(off)
  const double2 st = stamp[tg];
  const double ramp = alpha[ty & (kMaxTypes - 1)] * (double)(step - (long long)st.y);
  const double l = st.x + ramp;
  return l < 1.0 ? l : 1.0;
}
template <typename R> __device__ __forceinline__ void res_stage_caps(R* sfm, const R* __restrict__ fmax) {      // (caller synchronises)
  for (int k = threadIdx.x; k < kMaxTypes * kMaxTypes; k += blockDim.x) sfm[k] = fmax[k];
}
// one listed pair of a resolution context: li, lj the two lambdas, on = the type pair's mask bit, fcap its force cap.
// PT(tx, ty, tz, e1, e2, v) accumulates the unscaled term.  An unmarked pair is evaluated as everywhere else; a marked pair
// with w == 0 is not evaluated at all; the virial share is r.F of the force that was applied.
template <typename R, bool ENERGY, class PT>
__device__ __forceinline__ void res_pair(PT&& term, R li, R lj, bool on, R fcap, R dx, R dy, R dz, R& fx, R& fy, R& fz, double& e_lj, double& e_tab, double& vir) {
  if (!on) { term(fx, fy, fz, e_lj, e_tab, vir); return; }
  const R w = li * lj;
  if (w == (R)0) return;
  R tx = 0, ty = 0, tz = 0; double te1 = 0, te2 = 0, tv = 0;
  term(tx, ty, tz, te1, te2, tv);
  tx *= w; ty *= w; tz *= w;
  if (fcap > (R)0) {
    const R f2 = tx * tx + ty * ty + tz * tz;
    if (f2 > fcap * fcap) { const R sc = fcap * rsqrt_r(f2); tx *= sc; ty *= sc; tz *= sc; }
  }
  fx += tx; fy += ty; fz += tz;
  if (ENERGY) { e_lj += (double)w * te1; e_tab += (double)w * te2; vir += (double)(tx * dx + ty * dy + tz * dz); }
}

// Capped pairs (VerletListTabulatedCapped / VerletListLennardJonesCapped; rule set in include/chem_mi355.h, chem_nb_cap): inside
// the cap radius c of its type pair a pair is evaluated at r_e = c instead of r -- force magnitude f(c) along r_ij, energy U(c),
// virial share f(c) r.  c2[ti * kMaxTypes + tj] = c^2 (0 = the pair is not capped), staged in LDS beside the pairs' other
// parameters (cap_stage_radii); the decision is taken on the squares.
template <typename R> struct CapArgs { const R* c2; };
template <typename R> __device__ __forceinline__ void cap_stage_radii(R* sc2, const R* __restrict__ c2) {      // (caller synchronises)
  for (int k = threadIdx.x; k < kMaxTypes * kMaxTypes; k += blockDim.x) sc2[k] = c2[k];
}

// CUBIC: the host selects these instantiations only while a type pair of kind 3 exists, so that the others stay what they were
// CAPPED (with c2 = the type pair's squared cap radius): likewise only while a type pair is capped.  r2 is clamped to c2 before
// the branch on the kind; every kind then scales its f(r_e) / r_e by r_e / r (0 at r = 0: the one guard, the direction is undefined there)
template <typename R, bool ENERGY, bool CUBIC = false, bool CAPPED = false>
__device__ __forceinline__ void pair_term(const PairCore<R> pc, const PairExt<R>* __restrict__ pext, int pidx,
                                          const Vec4<R>* __restrict__ tab, R r2, R dx, R dy, R dz,
                                          R& fx, R& fy, R& fz, double& e_lj, double& e_tab, double& vir, R c2 = (R)0) {
  if (r2 <= pc.rc2) {
    [[maybe_unused]] R sc = (R)1;      // r_e / r
    const R rt2 = r2;                   // the pair's own r^2 (virial share: r.F of the applied force)
    if constexpr (CAPPED) {
      if (r2 < c2) { sc = r2 > (R)0 ? sqrt_r(c2) * rsqrt_r(r2) : (R)0; r2 = c2; }
    }
    if (CUBIC && pc.kind == (R)3) {
      const PairExt<R> px = pext[pidx];
      const R r = sqrt_r(r2);
      R t = (r - px.r0) * px.inv_dr;
      const R tmax = (R)(px.nrow - 1);
      t = t < (R)0 ? (R)0 : (t > tmax ? tmax : t);
      int k = (int)t;
      if (k > px.nrow - 2) k = px.nrow - 2;
      const R w = t - (R)k;
      const Vec4<R> cf = tab[px.toff + 2 * k];      // force coefficients; the energy row behind it is read with ENERGY only
      R ff = (cf.x + w * (cf.y + w * (cf.z + w * cf.w))) / r;
      if constexpr (CAPPED) ff *= sc;
      fx += ff * dx; fy += ff * dy; fz += ff * dz;
      if (ENERGY) { const Vec4<R> ce = tab[px.toff + 2 * k + 1]; e_tab += (double)(ce.x + w * (ce.y + w * (ce.z + w * ce.w))); vir += (double)(ff * rt2); }
    } else if (pc.kind == (R)1) {
      const R r2i = rcp_r(r2), r6i = r2i * r2i * r2i;
      R ff = r6i * (pc.lj1 * r6i - pc.lj2) * r2i;
      if constexpr (CAPPED) ff *= sc;
      fx += ff * dx; fy += ff * dy; fz += ff * dz;
      if (ENERGY) { const PairExt<R> px = pext[pidx]; e_lj += (double)(r6i * (px.e1 * r6i - px.e2) + px.shift); vir += (double)(ff * rt2); }
    } else {
      const PairExt<R> px = pext[pidx];
      const R r = sqrt_r(r2);
      R t = (r - px.r0) * px.inv_dr;
      const R tmax = (R)(px.nrow - 1);
      t = t < (R)0 ? (R)0 : (t > tmax ? tmax : t);
      int k = (int)t;
      if (k > px.nrow - 2) k = px.nrow - 2;
      const R wgt = t - (R)k;
      const Vec4<R> row = tab[px.toff + k];  // (f_k, df_k, e_k, de_k)
      R ff = (row.x + wgt * row.y) / r;
      if constexpr (CAPPED) ff *= sc;
      fx += ff * dx; fy += ff * dy; fz += ff * dz;
      if (ENERGY) { e_tab += (double)(row.z + wgt * row.w); vir += (double)(ff * rt2); }
    }
  }
}

// COUL: plus the truncated Coulomb term, charges read through tag[j] (launched only while a Coulomb pair is registered; these
// instantiations know both table kinds)
// RES: marked type pairs scaled by lambda_i lambda_j and capped (k_pair_force_res, launched only while a type pair is marked;
// both table kinds); lambda through tag[j] -> stamp, evaluated per neighbour
// (the body of k_pair_force and of k_pair_force_res, which alone takes the resolution arguments)
// CAPPED: type pairs with a cap radius (k_pair_force_cap, k_pair_force_rescap, launched only while a type pair is capped)
// TENSOR (k_pair_force_tensor, K13): the pair's whole term -- law, resolution weight and cap, Coulomb term -- goes into zeroed
// temporaries first, as res_pair does, and d_a t_b is added to six fp64 sums; tout[6 * block + c] = the block's half sums
// (xx, yy, zz, xy, xz, yz).  Not compiled into the instantiations of the step.
__device__ __forceinline__ void tensor_add(double (&tw)[6], double dx, double dy, double dz, double tx, double ty, double tz) {
  tw[0] += dx * tx; tw[1] += dy * ty; tw[2] += dz * tz; tw[3] += dx * ty; tw[4] += dx * tz; tw[5] += dy * tz;
}
// the six sums of a block of NW waves: wave reduction, then the waves' words in their order; `scale` times the sum to out[0..5]
template <int NW>
__device__ __forceinline__ void tensor_block_out(double (&tw)[6], double scale, double* __restrict__ out) {
  __shared__ double tred[6][NW];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    for (int o = 32; o > 0; o >>= 1) tw[c] += __shfl_xor(tw[c], o);
    if (lane_id() == 0) tred[c][threadIdx.x >> 6] = tw[c];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double s = 0;
    for (int k = 0; k < NW; ++k) s += tred[threadIdx.x][k];
    out[threadIdx.x] = scale * s;
  }
}
template <typename R, int TPP, bool ENERGY, bool CUBIC, bool COUL, bool RES, bool CAPPED = false, bool TENSOR = false>
__device__ __forceinline__ void pair_force_body(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                    const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                    const Box<R>& box, const PairCore<R>* __restrict__ pcore,
                                                    const PairExt<R>* __restrict__ pext, int ntypes,
                                                    const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                    double half_skin, DevCtl* ctl, const CoulArgs<R>& ca, const ResArgs<R>& ra,
                                                    const CapArgs<R>& cp = CapArgs<R>{}, double* __restrict__ tout = nullptr) {
  __shared__ PairCore<R> spc[kMaxTypes * kMaxTypes];
  for (int k = threadIdx.x; k < ntypes * ntypes; k += blockDim.x) spc[k] = pcore[k];
  [[maybe_unused]] const R* sfm = nullptr;
  if constexpr (RES) { __shared__ R sfm_[kMaxTypes * kMaxTypes]; res_stage_caps<R>(sfm_, ra.fmax); sfm = sfm_; }
  [[maybe_unused]] const R* sc2 = nullptr;
  if constexpr (CAPPED) { __shared__ R sc2_[kMaxTypes * kMaxTypes]; cap_stage_radii<R>(sc2_, cp.c2); sc2 = sc2_; }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && ctl->acc_maxdist > half_skin) ctl->skin_violation = 1;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid / TPP, sub = gid % TPP;
  R fx = 0, fy = 0, fz = 0;
  double e_lj = 0, e_tab = 0, vir = 0;
  [[maybe_unused]] double e_q = 0, v_q = 0;
  [[maybe_unused]] double tw[6] = {0, 0, 0, 0, 0, 0};
  if (i < n) {
    const Vec4<R> xi = x4[i];
    const int ti = (int)xi.w;
    const int cnt = nn[i];
    const int4* row = reinterpret_cast<const int4*>(nlist + (size_t)i * S);
    const int pbase = ti * ntypes;
    [[maybe_unused]] R kqi = 0; [[maybe_unused]] unsigned int crow = 0;
    if constexpr (COUL) { kqi = ca.k * ca.qtag[ca.tag[i]]; crow = ca.mask[ti]; }
    [[maybe_unused]] R lami = 1; [[maybe_unused]] unsigned int rrow = 0;
    if constexpr (RES) { lami = (R)res_lambda_dev(ra.stamp, ra.alpha, ra.step, ra.tag[i], ti); rrow = ra.mask[ti]; }
    // lane `sub` takes 4 consecutive neighbours per trip: one 16-byte index load, then four
    // independent position gathers in flight (rows are padded with the self index)
    for (int k = sub * 4; k < cnt; k += TPP * 4) {
      const int4 jj = row[k >> 2];
      const Vec4<R> xa = x4[jj.x], xb = x4[jj.y], xc = x4[jj.z], xd = x4[jj.w];
      const Vec4<R> xs[4] = {xa, xb, xc, xd};
      [[maybe_unused]] R qs[4] = {0, 0, 0, 0};
      if constexpr (COUL) {
        const int ta = ca.tag[jj.x], tb = ca.tag[jj.y], tc = ca.tag[jj.z], td = ca.tag[jj.w];
        qs[0] = ca.qtag[ta]; qs[1] = ca.qtag[tb]; qs[2] = ca.qtag[tc]; qs[3] = ca.qtag[td];
      }
      [[maybe_unused]] R ls[4] = {1, 1, 1, 1};
      if constexpr (RES) {
        const int ta = ra.tag[jj.x], tb = ra.tag[jj.y], tc = ra.tag[jj.z], td = ra.tag[jj.w];
        ls[0] = (R)res_lambda_dev(ra.stamp, ra.alpha, ra.step, ta, (int)xa.w); ls[1] = (R)res_lambda_dev(ra.stamp, ra.alpha, ra.step, tb, (int)xb.w);
        ls[2] = (R)res_lambda_dev(ra.stamp, ra.alpha, ra.step, tc, (int)xc.w); ls[3] = (R)res_lambda_dev(ra.stamp, ra.alpha, ra.step, td, (int)xd.w);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const Vec4<R> xj = xs[u];
        const R dx = pos_delta(xi.x, xj.x, 0, box), dy = pos_delta(xi.y, xj.y, 1, box), dz = pos_delta(xi.z, xj.z, 2, box);
        R r2 = dx * dx + dy * dy + dz * dz;
        r2 = (k + u < cnt) ? r2 : (R)1e30;     // padding entries (self index) never interact
        const int pidx = pbase + (int)xj.w;
        [[maybe_unused]] R c2 = (R)0;
        if constexpr (CAPPED) c2 = sc2[ti * kMaxTypes + (int)xj.w];
        if constexpr (TENSOR) {
          R tx = 0, ty = 0, tz = 0;
          if constexpr (RES) {
            const int tj = (int)xj.w;
            res_pair<R, ENERGY>([&](R& ax, R& ay, R& az, double& a1, double& a2, double& av) { pair_term<R, ENERGY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, ax, ay, az, a1, a2, av, c2); },
                                lami, ls[u], ((rrow >> tj) & 1u) != 0, sfm[ti * kMaxTypes + tj], dx, dy, dz, tx, ty, tz, e_lj, e_tab, vir);
          } else
          pair_term<R, ENERGY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, tx, ty, tz, e_lj, e_tab, vir, c2);
          if constexpr (COUL) coul_term<R, ENERGY>(kqi, qs[u], ((crow >> (int)xj.w) & 1u) != 0, ca.rc2, r2, dx, dy, dz, tx, ty, tz, e_q, v_q);
          fx += tx; fy += ty; fz += tz;
          tensor_add(tw, (double)dx, (double)dy, (double)dz, (double)tx, (double)ty, (double)tz);
        } else {
        if constexpr (RES) {
          const int tj = (int)xj.w;
          res_pair<R, ENERGY>([&](R& ax, R& ay, R& az, double& a1, double& a2, double& av) { pair_term<R, ENERGY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, ax, ay, az, a1, a2, av, c2); },
                              lami, ls[u], ((rrow >> tj) & 1u) != 0, sfm[ti * kMaxTypes + tj], dx, dy, dz, fx, fy, fz, e_lj, e_tab, vir);
        } else
        pair_term<R, ENERGY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, fx, fy, fz, e_lj, e_tab, vir, c2);
        if constexpr (COUL) coul_term<R, ENERGY>(kqi, qs[u], ((crow >> (int)xj.w) & 1u) != 0, ca.rc2, r2, dx, dy, dz, fx, fy, fz, e_q, v_q);
        }
      }
    }
  }
  if (TPP > 1) {
#pragma unroll
    for (int o = TPP / 2; o > 0; o >>= 1) {
      fx += __shfl_xor(fx, o); fy += __shfl_xor(fy, o); fz += __shfl_xor(fz, o);
    }
  }
  if (i < n && sub == 0) f4[i] = mk4<R>(fx, fy, fz, (R)0);
  if (ENERGY) {
    // full list: every pair is visited from both ends -> half weights
    __shared__ double red[COUL ? 5 : 3][4];
    for (int o = 32; o > 0; o >>= 1) { e_lj += __shfl_xor(e_lj, o); e_tab += __shfl_xor(e_tab, o); vir += __shfl_xor(vir, o); }
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = e_lj; red[1][threadIdx.x >> 6] = e_tab; red[2][threadIdx.x >> 6] = vir; }
    if constexpr (COUL) {
      for (int o = 32; o > 0; o >>= 1) { e_q += __shfl_xor(e_q, o); v_q += __shfl_xor(v_q, o); }
      if (lane_id() == 0) { red[3][threadIdx.x >> 6] = e_q; red[4][threadIdx.x >> 6] = v_q; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0, b = 0, c = 0;
      for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { a += red[0][k]; b += red[1][k]; c += red[2][k]; }
      eout[3 * blockIdx.x + 0] = 0.5 * a; eout[3 * blockIdx.x + 1] = 0.5 * b; eout[3 * blockIdx.x + 2] = 0.5 * c;
      if constexpr (COUL) {
        double d = 0, e = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { d += red[3][k]; e += red[4][k]; }
        ca.eout[2 * blockIdx.x + 0] = 0.5 * d; ca.eout[2 * blockIdx.x + 1] = 0.5 * e;
      }
    }
  }
  if constexpr (TENSOR) tensor_block_out<4>(tw, 0.5, tout + 6 * (size_t)blockIdx.x);      // (full list: half weights, as above)
}
template <typename R, int TPP, bool ENERGY, bool CUBIC = false, bool COUL = false>
__global__ __launch_bounds__(256) void k_pair_force(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                    const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                    Box<R> box, const PairCore<R>* __restrict__ pcore,
                                                    const PairExt<R>* __restrict__ pext, int ntypes,
                                                    const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                    double half_skin, DevCtl* ctl, CoulArgs<R> ca = CoulArgs<R>{}) {
  pair_force_body<R, TPP, ENERGY, CUBIC, COUL, false>(n, x4, f4, nlist, nn, S, box, pcore, pext, ntypes, tab, eout, half_skin, ctl, ca, ResArgs<R>{});
}
template <typename R, int TPP, bool ENERGY>
__global__ __launch_bounds__(256) void k_pair_force_res(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                        const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                        Box<R> box, const PairCore<R>* __restrict__ pcore,
                                                        const PairExt<R>* __restrict__ pext, int ntypes,
                                                        const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                        double half_skin, DevCtl* ctl, ResArgs<R> ra) {
  pair_force_body<R, TPP, ENERGY, true, false, true>(n, x4, f4, nlist, nn, S, box, pcore, pext, ntypes, tab, eout, half_skin, ctl, CoulArgs<R>{}, ra);
}
// capped general and capped resolution builds (both table kinds): entry points of their own, so that the argument blocks of
// k_pair_force and k_pair_force_res stay what they are
template <typename R, int TPP, bool ENERGY>
__global__ __launch_bounds__(256) void k_pair_force_cap(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                        const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                        Box<R> box, const PairCore<R>* __restrict__ pcore,
                                                        const PairExt<R>* __restrict__ pext, int ntypes,
                                                        const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                        double half_skin, DevCtl* ctl, CapArgs<R> cp) {
  pair_force_body<R, TPP, ENERGY, true, false, false, true>(n, x4, f4, nlist, nn, S, box, pcore, pext, ntypes, tab, eout, half_skin, ctl, CoulArgs<R>{}, ResArgs<R>{}, cp);
}
template <typename R, int TPP, bool ENERGY>
__global__ __launch_bounds__(256) void k_pair_force_rescap(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                           const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                           Box<R> box, const PairCore<R>* __restrict__ pcore,
                                                           const PairExt<R>* __restrict__ pext, int ntypes,
                                                           const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                           double half_skin, DevCtl* ctl, ResArgs<R> ra, CapArgs<R> cp) {
  pair_force_body<R, TPP, ENERGY, true, false, true, true>(n, x4, f4, nlist, nn, S, box, pcore, pext, ntypes, tab, eout, half_skin, ctl, CoulArgs<R>{}, ra, cp);
}

// =======================================================================================
// Tiled path (production for boxes with >= HX+2, HY+2, HZ+2 cells per axis).
//
// A tile = a block of HX x HY x HZ home cells.  Its stencil, (HX+2) x (HY+2) x (HZ+2) cells,
// is staged ONCE per workgroup into LDS with the periodic shift applied (coalesced 16-byte
// loads, each cache line fetched once), instead of 74 divergent 16-byte gathers per particle
// that cost one L1 line lookup each.  The neighbour list stores 16-bit slots of that LDS
// image (tile-local indices): half the HBM bytes of an int32 list, no minimum-image
// arithmetic in the pair loop, and the position gathers become ds_read_b128.
// The staged order is a pure function of cell_start, which only changes at a rebuild, so the
// build kernel and every later force launch see the same slot numbering.
// =======================================================================================
// HX, HY, HZ (CHEM_HX/HY/HZ, default 3), SX, SY, SZ and the tiles of a row along x (tile_nbx, tile_ntx, tile_xrange) live in
// chem_geom_host.hpp, shared with the host's planning rules.
constexpr int NROW = SY * SZ;          // x-rows of the stencil
constexpr int NHSEG = HY * HZ;         // home x-runs (contiguous in memory)

// positions live in dynamic LDS (capacity chosen at run time from the cell occupancy):
// sx[0..cap], slot `total` is a far-away dummy used as row padding
template <typename R> struct TileLDS {
  int rowoff[NROW + 1];                // first slot of each stencil row
  int celloff[NROW][SX + 1];           // slot offset of every cell inside its row
  int cellg[NROW][SX];                 // global index of the first particle of the cell
  R cellshx[NROW][SX];                 // periodic shift in x (per cell), y/z (per row)
  R rowshy[NROW], rowshz[NROW];
  int hstart[NHSEG], hoff[NHSEG + 1];  // home x-runs: global start, prefix of counts
  int geom[8];                         // hx, hy, hz, total, nhome, hbase, origin cell (10 bits per axis)
  // list build only: x sub-bin prefixes of every stencil cell (cell_sub, see dev_sort_gather; -1 = unknown),
  // staged coordinates of the lower corner of stencil cell (0,0,0), cell edges, sub-bins per unit length
  int cellsub[NROW][SX];
  // org: reference point of the staged coordinates = lower corner of stencil cell (0,0,0) + kRefCells cell edges (the centre of
  // a full 5x5x5 stencil: |staged coordinate| <= 2.5 edges + skin/2, the smallest magnitudes fp32 can be given), in the
  // encoding of the position arrays (pos_enc); clen: cell edges; subinv: sub-bins per unit length; qs: fixed-point scale
  R org[3], clen[3], subinv, pad_;
  R qs[3], pad2_;
};
constexpr float kRefCells = 2.5f;

// NOTE: the pointer must stay a plain local derived from the extern array (no integer
// round-trip, never stored in memory) so that the compiler keeps it in the LDS address space
// and emits ds_read/ds_write instead of flat_* accesses.
#define CHEM_DYN_LDS(R) \
  extern __shared__ __attribute__((aligned(16))) unsigned char chem_dyn_lds[]; \
  Vec4<R>* const sx = reinterpret_cast<Vec4<R>*>(chem_dyn_lds)

// Bytes of the force kernel's staged image of a tile of `cap` slots (fp32: 16-byte slots; fp64: 24-byte slots + type bytes, see
// tile_fill), and where the charge words of k_pair_tiles MODE 4 start behind it: one R per slot, 16-byte aligned.
template <typename R> __host__ __device__ constexpr size_t pair_img_bytes(int cap) {
  return sizeof(R) == 8 ? (size_t)(cap + 5) * 25 + 64 : (size_t)(cap + 5) * 16 + 16;
}
template <typename R> __host__ __device__ constexpr size_t coul_q_offset(int cap) { return (pair_img_bytes<R>(cap) + 15) & ~(size_t)15; }
template <typename R> __host__ __device__ constexpr size_t coul_img_bytes(int cap) { return coul_q_offset<R>(cap) + (size_t)(cap + 4) * sizeof(R); }

// Descriptor tables of one tile, computed ONCE per rebuild by k_tile_desc and kept in HBM
// (~1.3 KB per tile); every later launch copies them into LDS with one coalesced read instead
// of re-deriving them through dependent global loads and three barrier phases.
template <typename R>
__device__ __forceinline__ void tile_tables(TileLDS<R>& T, const int CAP, int tile, const int* __restrict__ cell_start,
                                            const Box<R>& box, DevCtl* ctl, const int* __restrict__ cell_sub = nullptr) {
  const int nx = box.nc[0], ny = box.nc[1], nz = box.nc[2];
  const int ntx = tile_ntx(nx, box.xs_nb, box.xs_w), nty = (ny + HY - 1) / HY;
  const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
  // z-ghost mode: layers 1..nz-2 are own, the stencil reaches into the ghost layers 0 and nz-1
  const int zg = box.zghost;
  int cx0, hx;
  tile_xrange(tx, nx, box.xs_nb, box.xs_w, cx0, hx);
  const int cy0 = ty * HY, cz0 = tz * HZ + zg;
  const int hy = min(HY, ny - cy0), hz = min(HZ, nz - zg - cz0);
  const int t = threadIdx.x;
  if (t < NROW * SX) {
    const int r = t / SX, k = t % SX, ry = r % SY, rz = r / SY;
    int cnt = 0, g = 0, sub = 0; R shx = 0;
    if (ry < hy + 2 && rz < hz + 2 && k < hx + 2) {
      int ox = cx0 - 1 + k, oy = cy0 - 1 + ry, oz = cz0 - 1 + rz;
      R shy = 0, shz = 0;
      if (ox < 0) { ox += nx; shx = pos_shift(-1, 0, box); } else if (ox >= nx) { ox -= nx; shx = pos_shift(1, 0, box); }
      if (oy < 0) { oy += ny; shy = pos_shift(-1, 1, box); } else if (oy >= ny) { oy -= ny; shy = pos_shift(1, 1, box); }
      if (zg) { shz = oz == 0 ? box.shz_lo : (oz == nz - 1 ? box.shz_hi : (R)0); }
      else if (oz < 0) { oz += nz; shz = pos_shift(-1, 2, box); } else if (oz >= nz) { oz -= nz; shz = pos_shift(1, 2, box); }
      const int oc = (oz * ny + oy) * nx + ox;
      g = cell_start[oc]; cnt = cell_start[oc + 1] - g;
      sub = cell_sub ? cell_sub[oc] : -1;
      if (k == 0) { T.rowshy[r] = shy; T.rowshz[r] = shz; }
    } else if (k == 0) { T.rowshy[r] = 0; T.rowshz[r] = 0; }
    T.cellg[r][k] = g; T.cellshx[r][k] = shx; T.cellsub[r][k] = sub;
    T.celloff[r][k + 1] = cnt;   // turned into a prefix below
  }
  __syncthreads();
  if (t < NROW) {
    int o = 0; T.celloff[t][0] = 0;
    for (int k = 0; k < SX; ++k) { o += T.celloff[t][k + 1]; T.celloff[t][k + 1] = o; }
  }
  __syncthreads();
  // Third step, three waves side by side, everything from the LDS tables of the first two steps (the home cells are
  // among the 125 stencil cells): a single thread walking 25 rows and 9 home runs with dependent loads cost ~10 us
  // per tile in the rebuild, where these tables are computed (the force kernel reads them back from HBM).
  const int wv = t >> 6, ln = t & 63;
  if (wv == 0) {          // first slot of every stencil row
    const int len = ln < NROW ? T.celloff[ln][SX] : 0;
    int incl = len;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) { const int u = __shfl_up(incl, o); if (ln >= o) incl += u; }
    if (ln < NROW) T.rowoff[ln] = incl - len;
    if (ln == NROW - 1) {
      T.rowoff[NROW] = incl;
      if (incl > CAP) atomicMax(&ctl->stage_overflow, incl);
      T.geom[3] = incl < CAP ? incl : CAP;
    }
  } else if (wv == 1) {   // (blocks of >= 128 threads) home x-runs (contiguous in memory): global start, prefix of counts
    const int hyi = ln % HY, hzi = ln / HY;
    int st = 0, cn = 0;
    if (ln < NHSEG && hyi < hy && hzi < hz) {
      const int hr = (hzi + 1) * SY + (hyi + 1);
      st = T.cellg[hr][1]; cn = T.celloff[hr][hx + 1] - T.celloff[hr][1];
    }
    int incl = cn;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const int u = __shfl_up(incl, o); if (ln >= o) incl += u; }
    if (ln < NHSEG) { T.hstart[ln] = st; T.hoff[ln] = incl - cn; }
    if (ln == NHSEG - 1) { T.hoff[NHSEG] = incl; T.geom[4] = incl; }
  }
  if (t == (int)blockDim.x - 1) {
    T.geom[0] = hx; T.geom[1] = hy; T.geom[2] = hz;
    T.geom[6] = cx0 | (cy0 << 10) | (cz0 << 20);   // first home cell (list build: slot of an excluded partner)
    T.geom[7] = 0;                                 // set by list_stage_f32: a stencil cell without x-slice information
    // geometry of the staged image (list build, x-window of a row).  In z-ghost mode layer l of the slab is the
    // global layer z0g + l - 1; the staged z of the ghost layers carries shz_lo / shz_hi, which continues the
    // same affine map across the periodic boundary.
    const double clx = 2.0 * box.qh[0] / nx, cly = 2.0 * box.qh[1] / ny, clz = 2.0 * box.qh[2] / (zg ? box.nzg : nz);   // (qh = L / 2 in fp64)
    T.clen[0] = (R)clx; T.clen[1] = (R)cly; T.clen[2] = (R)clz;
    T.org[0] = pos_enc(((double)(cx0 - 1) + kRefCells) * clx, 0, box); T.org[1] = pos_enc(((double)(cy0 - 1) + kRefCells) * cly, 1, box);
    T.org[2] = pos_enc(((double)(zg ? box.z0g + cz0 - 2 : cz0 - 1) + kRefCells) * clz, 2, box);
    T.subinv = (R)((double)NSUB / clx); T.pad_ = 0;
    T.qs[0] = box.qsf[0]; T.qs[1] = box.qsf[1]; T.qs[2] = box.qsf[2]; T.pad2_ = 0;
  }
  __syncthreads();
}

template <typename R>
__global__ __launch_bounds__(128) void k_tile_desc(int ntiles, int CAP, const int* __restrict__ cell_start, Box<R> box,
                                                   TileLDS<R>* __restrict__ desc, DevCtl* ctl, const int* __restrict__ cell_sub) {
  if (!ctl->need_rebuild) return;
  __shared__ TileLDS<R> T;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    tile_tables<R>(T, CAP, tile, cell_start, box, ctl, cell_sub);
    const int* src = reinterpret_cast<const int*>(&T);
    int* dst = reinterpret_cast<int*>(&desc[tile]);
    for (int k = threadIdx.x; k < (int)(sizeof(TileLDS<R>) / 4); k += blockDim.x) dst[k] = src[k];
  }
}

template <typename R>
__device__ __forceinline__ void tile_load_desc(TileLDS<R>& T, const TileLDS<R>* __restrict__ desc, int tile) {
  const int* src = reinterpret_cast<const int*>(&desc[tile]);
  int* dst = reinterpret_cast<int*>(&T);
  for (int k = threadIdx.x; k < (int)(sizeof(TileLDS<R>) / 4); k += blockDim.x) dst[k] = src[k];
}

// stages the stencil of the tile described by T into sx.  wmode 0: .w = particle type (force
// kernel), 1: .w = (global index << 5 | type) (list build; bit 4 stays clear so that v_bfe can take .w as its offset).  Caller synchronises afterwards.
// All global loads of a wave are issued before the first LDS write so that the staging costs one
// memory latency, not one per row chunk.
// D3 (fp64 force kernel): 24-byte slots (x, y, z) with the types in a byte array behind the image instead of 32-byte
// (x, y, z, type) slots -- 70 KB instead of 90 KB at C5, i.e. two workgroups per CU instead of one
template <typename R> __device__ __forceinline__ unsigned char* d3_types(Vec4<R>* sx, int CAP) { return reinterpret_cast<unsigned char*>(sx) + (size_t)(CAP + 1) * 24; }
template <typename R, bool D3>
__device__ __forceinline__ void slot_store(Vec4<R>* const sx, const int CAP, int dst, const Vec4<R>& p) {
  if constexpr (D3) {
    R* s3 = reinterpret_cast<R*>(sx) + 3 * dst;
    s3[0] = p.x; s3[1] = p.y; s3[2] = p.z;
    d3_types<R>(sx, CAP)[dst] = (unsigned char)(int)p.w;
  } else sx[dst] = p;
}
// QW (k_pair_tiles MODE 4, not LEAN): one charge word per slot into sq[], tag[g] -> qtag; these loads too are issued before the
// first LDS write (two dependent latencies instead of one; the dummy slot carries charge 0)
// RW (k_pair_tiles MODE 5, with QW): the word is the slot's resolution lambda instead, computed here from the by-tag stamp, the
// slot's type and the step of the forces (ResFill; res_lambda_dev) -- the dummy slot carries lambda 0
struct ResFill { const double2* stamp; const double* alpha; long long step; };
template <typename R, int BS, bool LEAN = false, bool D3 = false, bool QW = false, bool RW = false>
__device__ __forceinline__ void tile_fill(const TileLDS<R>& T, Vec4<R>* const sx, const int CAP,
                                          const Vec4<R>* __restrict__ x4, int wmode, const int* __restrict__ tagv = nullptr,
                                          const R* __restrict__ qtag = nullptr, R* const sq = nullptr, const ResFill rf = ResFill{}) {
  constexpr int NW = BS / 64, RPW = (NROW + NW - 1) / NW;
  const int t = threadIdx.x;
  const int w = t >> 6, l = t & 63;
  if (t == 0) slot_store<R, D3>(sx, CAP, T.geom[3], mk4<R>((R)1e18, (R)1e18, (R)1e18, (R)0));
  if constexpr (QW) { if (t == 0) sq[T.geom[3]] = (R)0; }
  if constexpr (LEAN) {
    // register-lean variant (list build: staging is <2 % of the tile's time, occupancy matters more)
    for (int r = w; r < NROW; r += NW) {
      const int len = T.celloff[r][SX], o0 = T.rowoff[r];
      for (int e = l; e < len; e += 64) {
        int k = 0;
#pragma unroll
        for (int q = 1; q < SX; ++q) k += (e >= T.celloff[r][q]) ? 1 : 0;
        const int g = T.cellg[r][k] + (e - T.celloff[r][k]);
        const int dst = o0 + e;
        if (dst < CAP) {
          Vec4<R> p = x4[g];
          p.x = pos_local(p.x, T.cellshx[r][k], T.org[0], T.qs[0]); p.y = pos_local(p.y, T.rowshy[r], T.org[1], T.qs[1]); p.z = pos_local(p.z, T.rowshz[r], T.org[2], T.qs[2]);
          if (wmode) p.w = idx_as_real((g << 5) | (int)p.w, (R)0);
          slot_store<R, D3>(sx, CAP, dst, p);
        }
      }
    }
    return;
  }
  Vec4<R> pv[RPW][2];
  int pk_[RPW][2], pg[RPW][2];
  [[maybe_unused]] int ptg[RPW][2];
  [[maybe_unused]] R pq[RPW][2];
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int r = w + rr * NW;
    const int len = r < NROW ? T.celloff[r][SX] : 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int e = l + 64 * c;
      pk_[rr][c] = -1;
      if (e < len) {
        int k = 0;
#pragma unroll
        for (int q = 1; q < SX; ++q) k += (e >= T.celloff[r][q]) ? 1 : 0;
        const int g = T.cellg[r][k] + (e - T.celloff[r][k]);
        pk_[rr][c] = k; pg[rr][c] = g;
        pv[rr][c] = x4[g];
        if constexpr (QW) ptg[rr][c] = tagv[g];
      }
    }
  }
  if constexpr (QW) {
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if constexpr (RW) pq[rr][c] = pk_[rr][c] >= 0 ? (R)res_lambda_dev(rf.stamp, rf.alpha, rf.step, ptg[rr][c], (int)pv[rr][c].w) : (R)0;
        else pq[rr][c] = pk_[rr][c] >= 0 ? qtag[ptg[rr][c]] : (R)0;
      }
  }
#pragma unroll
  for (int rr = 0; rr < RPW; ++rr) {
    const int r = w + rr * NW;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int k = pk_[rr][c];
      if (k >= 0) {
        const int dst = T.rowoff[r] + l + 64 * c;
        if (dst < CAP) {
          Vec4<R> p = pv[rr][c];
          p.x = pos_local(p.x, T.cellshx[r][k], T.org[0], T.qs[0]); p.y = pos_local(p.y, T.rowshy[r], T.org[1], T.qs[1]); p.z = pos_local(p.z, T.rowshz[r], T.org[2], T.qs[2]);
          if (wmode) p.w = idx_as_real((pg[rr][c] << 5) | (int)p.w, (R)0);
          slot_store<R, D3>(sx, CAP, dst, p);
          if constexpr (QW) sq[dst] = pq[rr][c];
        }
      }
    }
  }
  // rows longer than 128 particles (crowded cells): remainder, serial
  for (int r = w; r < NROW; r += NW) {
    const int len = T.celloff[r][SX], o0 = T.rowoff[r];
    for (int e = l + 128; e < len; e += 64) {
      int k = 0;
#pragma unroll
      for (int q = 1; q < SX; ++q) k += (e >= T.celloff[r][q]) ? 1 : 0;
      const int g = T.cellg[r][k] + (e - T.celloff[r][k]);
      const int dst = o0 + e;
      if (dst < CAP) {
        Vec4<R> p = x4[g];
        p.x = pos_local(p.x, T.cellshx[r][k], T.org[0], T.qs[0]); p.y = pos_local(p.y, T.rowshy[r], T.org[1], T.qs[1]); p.z = pos_local(p.z, T.rowshz[r], T.org[2], T.qs[2]);
        if (wmode) p.w = idx_as_real((g << 5) | (int)p.w, (R)0);
        slot_store<R, D3>(sx, CAP, dst, p);
        if constexpr (RW) sq[dst] = (R)res_lambda_dev(rf.stamp, rf.alpha, rf.step, tagv[g], (int)p.w);
        else if constexpr (QW) sq[dst] = qtag[tagv[g]];
      }
    }
  }
}

// List build, fp32: LDS layout of one staged tile (inside the same dynamic LDS block the force kernel uses for its
// float4 image -- 12 + ntypes/8 bytes per slot instead of 16):
//   img   groups of FOUR slots in SoA order, 64 bytes (+16 of padding, kGrpF) per group: u0..u3 | v0..v3 | w0..w3 | q0..q3 with (u,v,w) the
//         position relative to the lower corner of the tile's stencil (|u| <= 5 cell edges) and q = u^2+v^2+w^2.  The
//         test of a candidate is  rl^2 + delta - |ri|^2 - q + 2 ri.(u,v,w) >= 0 : one packed add and three packed FMAs per
//         TWO candidates instead of 3 sub + 1 mul + 2 fma + 1 sub each -- the loop is bound by VALU issue.  The
//         expanded form loses ~6e-5 absolute on r^2 (coordinates <= 14), which `delta` covers: the 16-bit force list
//         is a SUPERSET by a shell of 5e-5 (the force kernel applies the exact cutoff); the int32 rows re-test their
//         hits with the difference form and stay exact;
//   tmask one bit per slot and home type ti: "the pair (ti, type of the slot) carries a potential" (MSB first: slot s
//         is bit 31 - (s & 31) of word s >> 5).  The type filter of a 32-candidate segment is one funnel shift of two
//         words instead of two instructions per candidate;
//   bnd   slot offset (inside its row) of every x-slice boundary of every stencil row: 5 cells x 4 slices + 1 values,
//         so that the x-window of a row is two 16-bit reads (was: two table reads and bit-field arithmetic per end).
// geom[7] of the tile tables is set when a stencil cell has no slice information (crowded cell): whole-cell windows then.
struct ActMask { unsigned int row[kMaxTypes]; };   // bit tj of row[ti]: pair (ti,tj) has a potential
#define CHEM_LDS __attribute__((address_space(3)))
constexpr int NBND = SX * NSUB + 1;
#ifndef CHEM_LIST_DELTA
#define CHEM_LIST_DELTA 2.5e-4f
#endif
constexpr float kListDelta = CHEM_LIST_DELTA;
// floats per group of four slots in the list-build image: 16 used + 4 of padding.  With a stride of 16 words the reads
// of lanes on groups g and g + 4 hit the same banks (SQ_LDS_BANK_CONFLICT was 47 % of the LDS cycles of the rebuild);
// 20 words put 16 consecutive groups on 16 different bank quads.
constexpr int kGrpF = 20;   // see the layout note below: what the expanded distance form may lose on r^2
struct ListLDS { int img_bytes, nwords, tmask_off, bnd_off; };
__device__ __forceinline__ ListLDS list_lds_layout(int CAP, int ntypes) {
  ListLDS L;
  L.img_bytes = (((CAP + 3) >> 2) + 3) * kGrpF * 4;          // (+ three groups: the pipelined reads run up to two groups past the last slot)
  L.nwords = ((CAP + 31) >> 5) + 2;
  L.tmask_off = L.img_bytes;
  L.bnd_off = L.tmask_off + ntypes * L.nwords * 4;
  return L;
}
__host__ __device__ constexpr size_t list_lds_bytes(int CAP, int ntypes) {
  return (size_t)(((CAP + 3) >> 2) + 3) * kGrpF * 4 + (size_t)ntypes * (((CAP + 31) >> 5) + 2) * 4 + (size_t)NROW * NBND * 2 + 16;
}

// zeroes the type masks (call before the workgroup barriers of tile_tables) ...
template <int BS>
__device__ __forceinline__ void list_stage_clear(unsigned char* lds, const ListLDS& L, int ntypes) {
  CHEM_LDS unsigned int* tm = (CHEM_LDS unsigned int*)((CHEM_LDS unsigned char*)lds + L.tmask_off);
  for (int k = threadIdx.x; k < ntypes * L.nwords; k += BS) tm[k] = 0u;
}
// ... and stages coordinates, type masks and slice boundaries of the tile described by T (caller synchronises afterwards)
// RS = precision of the particle arrays and tile tables: the image itself is always fp32 (tile-local coordinates, the
// subtraction of the stencil corner done in RS) -- the force list it yields may be a superset, so the fp64 build uses
// this list build too and keeps its exact fp64 one for the int32 Verlet rows only
template <typename RS, int BS>
__device__ __forceinline__ void list_stage_f32(TileLDS<RS>& T, unsigned char* lds, const ListLDS& L, const int CAP,
                                               const Vec4<RS>* __restrict__ x4, const ActMask& act, int ntypes) {
  constexpr int NW = BS / 64;
  // explicit LDS address space: through a generic pointer these become flat_* accesses (and flat atomics)
  CHEM_LDS unsigned char* const l3 = (CHEM_LDS unsigned char*)lds;
  CHEM_LDS float* img = (CHEM_LDS float*)l3;
  CHEM_LDS unsigned int* tm = (CHEM_LDS unsigned int*)(l3 + L.tmask_off);
  CHEM_LDS unsigned short* bnd = (CHEM_LDS unsigned short*)(l3 + L.bnd_off);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int t = threadIdx.x; t < NROW * NBND; t += BS) {
    const int r = t / NBND, f = t - r * NBND, k = f >> 2, j = f & 3;
    int v = T.celloff[r][k < SX ? k : SX];
    if (k < SX && j) {
      const int pk = T.cellsub[r][k];
      if (pk < 0) { if (T.celloff[r][k + 1] > T.celloff[r][k]) T.geom[7] = 1; }
      else v += (pk >> (8 * (j - 1))) & 0xff;
    }
    bnd[t] = (unsigned short)v;
  }
  for (int r = w; r < NROW; r += NW) {
    const int len = T.celloff[r][SX], o0 = T.rowoff[r];
    for (int e0 = 0; e0 < len; e0 += 64) {          // (wave-uniform trip count: the type masks are built with ballots)
      const int e = e0 + l;
      int tj = -1;
      if (e < len) {
        int k = 0;
#pragma unroll
        for (int q = 1; q < SX; ++q) k += (e >= T.celloff[r][q]) ? 1 : 0;
        const int g = T.cellg[r][k] + (e - T.celloff[r][k]);
        const int dst = o0 + e;
        if (dst < CAP) {
          const Vec4<RS> p = x4[g];
          CHEM_LDS float* grp = img + (dst >> 2) * kGrpF + (dst & 3);
          const float u = (float)pos_local(p.x, T.cellshx[r][k], T.org[0], T.qs[0]), v = (float)pos_local(p.y, T.rowshy[r], T.org[1], T.qs[1]),
                      w_ = (float)pos_local(p.z, T.rowshz[r], T.org[2], T.qs[2]);
          grp[0] = u; grp[4] = v; grp[8] = w_; grp[12] = fmaf(u, u, fmaf(v, v, w_ * w_));   // (explicit: the same rounding in every kernel this is inlined into)
          tj = (int)p.w & 15;
        }
      }
      // 64 consecutive slots = 2 or 3 mask words: one ballot per home type, the three words assembled by shifts and
      // bit reversal, one atomic each (a per-slot atomic OR is a 32-way same-address conflict in the LDS)
      const int slot0 = o0 + e0, sh = slot0 & 31, wbase = slot0 >> 5;
      for (int ti = 0; ti < ntypes; ++ti) {
        const unsigned long long m = __ballot(tj >= 0 && ((act.row[ti] >> tj) & 1u));
        if (m == 0ull) continue;
        const unsigned long long lo = m << sh;
        const unsigned int w2 = sh ? (unsigned int)(m >> (64 - sh)) : 0u;
        const unsigned int part = l == 0 ? (unsigned int)lo : (l == 1 ? (unsigned int)(lo >> 32) : w2);
        if (l < 3 && part) __hip_atomic_fetch_or(&tm[ti * L.nwords + wbase + l], __brev(part), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 nt_load_u4(const uint4* p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

// XCD-aware work-item order (speed only, never correctness): workgroups are dealt round-robin
// over the 8 XCDs, so block b and b+8 share an L2.  Remapping gives every XCD one contiguous
// range of tiles (a z-slab of the box): its 4 MiB L2 then holds the slab's positions and the
// stencil staging hits L2 instead of pulling the whole position array through the fabric.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}


// ---- list build on tiles.  Two products from one sweep:
//   nl16/nnh  : 16-bit LDS slots of the pairs that carry a non-bonded potential (type-pair mask
//               `act`; e.g. A-B and A-D of chain_growth_catalytic/topol.top:16-17 are off) -- read by
//               the force kernel every step.  Layout is tile-major and transposed: the 8-slot chunk c
//               of home particle q of a tile lives at  base + (c*nhome + q)*8,  so that consecutive
//               lanes (= consecutive home particles) read consecutive 16-byte words.
//               nnh holds one word per stored row: its entries in the lower half, in the upper half the home particle (index
//               in the tile's cell-run order) the row belongs to -- the natural order here, q itself; the fused rebuild may
//               store a tile's rows in another order (dev_row_order, chem_roworder_host.hpp).
//   nlist/nn  : int32 global indices of ALL non-excluded pairs within rc+skin (the Verlet list the
//               reaction scan and diagnostics traverse) -- only when `nlist` is non-null.
// One lane per home particle walks the nine x-runs of its 27-cell stencil in the staged LDS image:
// no cross-lane traffic, every lane does useful work (the wave-per-particle ballot version spent
// ~7x more instructions per accepted pair).

// list build of ONE staged tile (T and sx filled, block synchronised): see k_nlist_tiles
template <typename R, int BS>
__device__ __forceinline__ void dev_nlist_tile(const TileLDS<R>& T, Vec4<R>* const sx, const int* tag, const R rl2,
                                               const int* excl_start, const int* excl_list, const int has_excl, const ActMask& act,
                                               unsigned short* nl16, const int S16, int* nnh, int* nlist, const int S, int* nn, DevCtl* ctl,
                                               const Box<R>* bx = nullptr, const int* rtag = nullptr, const Vec4<R>* x4 = nullptr, const R rl2_rows_ = (R)-1,
                                               const int hbase_out = -1) {
    // (hbase_out >= 0: the rows and counts go to that row base of nl16 / nnh instead of the tile's own -- the staging region of
    //  the row order, see dev_row_order)
    const R rl2_rows = rl2_rows_ > (R)0 ? rl2_rows_ : rl2;   // int32 Verlet rows: the workload's rc+skin (see dev_nlist_tile_f32)
    const int hx = T.geom[0], total = T.geom[3], nhome = T.geom[4], hbase = hbase_out >= 0 ? hbase_out : T.geom[5];
    unsigned short* reg16 = nl16 + (size_t)hbase * S16;
    for (int q = threadIdx.x; q < nhome; q += BS) {
      int sgi = 0;
#pragma unroll
      for (int k = 1; k < NHSEG; ++k) sgi += (q >= T.hoff[k]) ? 1 : 0;
      const int inrun = q - T.hoff[sgi];
      const int p = T.hstart[sgi] + inrun;
      const int ly = sgi % HY, lz = sgi / HY;
      const int hr = (lz + 1) * SY + (ly + 1);
      const int eh = inrun + T.celloff[hr][1];
      int lx = 0;
      for (int k = 2; k <= hx; ++k) lx += (eh >= T.celloff[hr][k]) ? 1 : 0;
      const int sself = T.rowoff[hr] + eh;
      const Vec4<R> xi = sx[sself];
      const unsigned int arow = act.row[real_as_idx(xi.w) & 15];
      int e0 = 0, e1 = 0;
      if (has_excl) { const int tg = tag[p]; e0 = excl_start[tg]; e1 = excl_start[tg + 1]; }
      int cnt = 0, cnt16 = 0;
      int* row32 = nlist ? nlist + (size_t)p * S : nullptr;
      uint4* regq = reinterpret_cast<uint4*>(reg16) + q;   // chunk c of this particle: regq[c * nhome]
      // accepted slots are shifted into a 128-bit register; every 8th append stores one whole
      // 16-byte chunk (instead of eight scattered 2-byte stores)
      uint4 acc = make_uint4(0, 0, 0, 0);
      auto push = [&](unsigned int sl) {
        acc.x = __builtin_amdgcn_alignbit(acc.y, acc.x, 16);
        acc.y = __builtin_amdgcn_alignbit(acc.z, acc.y, 16);
        acc.z = __builtin_amdgcn_alignbit(acc.w, acc.z, 16);
        acc.w = (acc.w >> 16) | (sl << 16);
        if ((cnt16 & 7) == 7 && cnt16 < S16) regq[(size_t)(cnt16 >> 3) * nhome] = acc;
        ++cnt16;
      };
      auto hit = [&](int s, int jw) {
        const int j = jw >> 5;
        bool ok = j != p;
        if (ok && e1 > e0) {
          const int tgj = tag[j];
          for (int e = e0; e < e1; ++e) if (excl_list[e] == tgj) { ok = false; break; }
        }
        if (ok) {
          if ((arow >> (jw & 15)) & 1u) push((unsigned int)s);
          if (row32) {
            bool in_rows = true;
            if (rl2_rows < rl2) { const Vec4<R> xj = sx[s]; const R dx = xi.x - xj.x, dy_ = xi.y - xj.y, dz_ = xi.z - xj.z; in_rows = dx * dx + dy_ * dy_ + dz_ * dz_ <= rl2_rows; }
            if (in_rows) { if (cnt < S) row32[cnt] = j; ++cnt; }
          }
        }
      };
      // Two passes per x-run segment of <= 64 staged candidates:
      //  1. distance tests only, results OR-ed into a 64-bit per-lane hit mask (no branches);
      //  2. the few hits (~15 %) are peeled off the mask one by one for the type / exclusion /
      //     activity filters and the chunked store.
      // The branchy hit handling no longer sits in the loop that runs 475 times per particle.
      // x-window of every stencil row: a candidate in row (dy, dz) is at least (dyv, dzv) away in y and z
      // (distance of the home particle from that row's slab), so only x within sqrt(rl^2 - dyv^2 - dzv^2)
      // can be a neighbour -- on average 46 % of the 3-cell run.  The cells are sorted by x sub-bin
      // (dev_sort_gather), whose prefix counts turn the window into a slot range; `weps` absorbs every
      // rounding difference between the binning arithmetic and this one (bins only prune, the distance test
      // below decides membership).
      auto suboff = [&](int r, int f, bool lower) {
        const int k = f >> 2, j = f & 3;
        const int base = T.celloff[r][k];
        if (j == 0) return base;
        const int pk = T.cellsub[r][k];
        if (pk < 0) return lower ? base : T.celloff[r][k + 1];
        return base + ((pk >> (8 * (j - 1))) & 0xff);
      };
#pragma unroll 1
      for (int dzy = 0; dzy < 9; ++dzy) {
        const int dz = dzy / 3, dy = dzy - 3 * dz;
        const int r = (lz + dz) * SY + (ly + dy);
        // (everything is recomputed per row from the LDS tables: keeping it live across the row loop spills)
        const R weps = T.clen[0] * (R)2e-4;
        const R ylo = ((R)(ly + 1) - (R)kRefCells) * T.clen[1], zlo = ((R)(lz + 1) - (R)kRefCells) * T.clen[2];   // (staged coordinates are relative to T.org)
        R ddy = dy == 0 ? xi.y - ylo - weps : (dy == 2 ? ylo + T.clen[1] - xi.y - weps : (R)0);
        R ddz = dz == 0 ? xi.z - zlo - weps : (dz == 2 ? zlo + T.clen[2] - xi.z - weps : (R)0);
        ddy = ddy > 0 ? ddy : (R)0; ddz = ddz > 0 ? ddz : (R)0;
        const R w2 = rl2 - ddy * ddy - ddz * ddz;
        if (w2 < (R)0) continue;
        const R ws = (sqrt_r(w2) + weps) * T.subinv, sxi = (xi.x + (R)kRefCells * T.clen[0]) * T.subinv;
        int f_lo = (int)(sxi - ws), f_hi = (int)(sxi + ws);     // truncation == floor where it matters (clamped below at >= 0)
        f_lo = f_lo > lx * NSUB ? f_lo : lx * NSUB;
        f_hi = f_hi < (lx + 3) * NSUB - 1 ? f_hi : (lx + 3) * NSUB - 1;
        const int a = T.rowoff[r] + suboff(r, f_lo, true);
        int b = T.rowoff[r] + suboff(r, f_hi + 1, false);
        b = b < total ? b : total;
        for (int s0 = a; s0 < b; s0 += 64) {
          const int len = (b - s0) < 64 ? (b - s0) : 64;
          unsigned int mlo = 0, mhi = 0;
          for (int k = 0; k < len; k += 4) {
            Vec4<R> xj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xj[u] = sx[(k + u < len) ? s0 + k + u : total];   // past the run: far-away dummy
            unsigned int bits = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const R dx = xi.x - xj[u].x, dy_ = xi.y - xj[u].y, dz_ = xi.z - xj[u].z;
              const R r2 = dx * dx + dy_ * dy_ + dz_ * dz_;
              bits |= (r2 <= rl2) ? (1u << u) : 0u;
            }
            if (k < 32) mlo |= bits << k; else mhi |= bits << (k - 32);
          }
          unsigned long long m = ((unsigned long long)mhi << 32) | mlo;
          while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int s = s0 + k;
            hit(s, real_as_idx(sx[s].w));
          }
        }
      }
      // pad the last chunk with the far-away dummy slot (chunks are read whole)
      const int real16 = cnt16;
      if (real16 <= S16) while (cnt16 & 7) push((unsigned int)total);
      nnh[hbase + q] = row_word(real16 < S16 ? real16 : S16, q);
      if (real16 > S16) atomicMax(&ctl->nl_overflow, real16);
      if (row32) {
        const int c32 = cnt < S ? cnt : S;
        for (int k = c32; k < ((c32 + 3) & ~3); ++k) row32[k] = p;
        nn[p] = c32;
        if (cnt > S) atomicMax(&ctl->nl_overflow, cnt);
      }
    }
}

// fp32 list build of ONE tile staged by list_stage_f32 (workgroup synchronised).  Same products as dev_nlist_tile.
// Per home particle (one lane each) and stencil row: x-window [a, b) from the slice-boundary table, then segments of
// up to 32 candidates = 8 groups of four slots, two groups per trip on ping-pong registers: the four ds_read_b128 of the
// group after next are in flight while one is tested, and the window of the NEXT row is looked up before this row's
// candidates are walked, so that the LDS latencies hide behind arithmetic instead of adding up (16 waves per CU: the
// rebuild kernel runs two workgroups per CU at 128 registers).  A test (expanded form, see the layout note above)
// leaves its result in the sign bit of rl^2 + delta - r^2, which one v_alignbit per candidate
// shifts into the segment's miss mask.  Hits surviving the type mask (and, located as slots, the self pair and up to
// four excluded partners) are peeled off and appended to the lane's 16-byte chunk register.
// The home particles behind the last full pass of BS (nhome % BS of them) are swept by nine lanes each, one per stencil
// row (`coop_on`, option coop_overflow): see the cooperative rounds at the end.
template <typename RS, int BS>
__device__ __forceinline__ void dev_nlist_tile_f32(const TileLDS<RS>& T, unsigned char* lds, const ListLDS& L, const int* tag, const float rl2,
                                                   const int* excl_start, const int* excl_list, const int has_excl,
                                                   unsigned short* nl16, const int S16, int* nnh, int* nlist, const int S, int* nn, DevCtl* ctl,
                                                   const Box<RS>* bx, const int* rtag, const Vec4<RS>* x4, const int ablate = 0, const float rl2_rows_ = -1.f,
                                                   const BondRecs bslots = BondRecs{}, const int* gtag = nullptr, const int real0 = 0, const int real1 = 0x7fffffff,
                                                   const int coop_on = 0, const int hbase_out = -1) {
  // (gtag, real0, real1: slab decomposition -- index of a tag's GHOST copy on this rank, range of the real particles;
  //  hbase_out >= 0: row base of the rows and counts in nl16 / nnh instead of the tile's own, see dev_row_order)
  const float rl2_rows = rl2_rows_ > 0.f ? rl2_rows_ : rl2;   // int32 Verlet rows: the workload's rc+skin (the 16-bit force list may use a wider list skin)
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) const volatile f32x4 lds_f32x4;   // volatile: keeps the 16-byte reads and their order
  CHEM_LDS unsigned char* const l3 = (CHEM_LDS unsigned char*)lds;   // (explicit LDS address space: ds_read, not flat_load)
  const CHEM_LDS float* img = (const CHEM_LDS float*)l3;
  const CHEM_LDS unsigned int* tmask = (const CHEM_LDS unsigned int*)(l3 + L.tmask_off);
  const CHEM_LDS unsigned short* bnd = (const CHEM_LDS unsigned short*)(l3 + L.bnd_off);
  const int hx = T.geom[0], total = T.geom[3], nhome = T.geom[4], hbase = hbase_out >= 0 ? hbase_out : T.geom[5];
  const bool nowin = T.geom[7] != 0;
  unsigned short* reg16 = nl16 + (size_t)hbase * S16;
  const float clen0 = (float)T.clen[0], clen1 = (float)T.clen[1], clen2 = (float)T.clen[2], subinv = (float)T.subinv;
  const float weps = clen0 * 2e-4f;

  // What a sweep needs to know about its home particle q (one lane per home, or the nine lanes of the cooperative pass).
  struct Home {
    int p, ly, lz, sself, e0, e1, xs0, xs1, xs2, xs3, fmin, fmax;
    float xix, xiy, xiz, cq, dylo, dyhi, dzlo, dzhi, sxi;
    const CHEM_LDS unsigned int* tmrow;
    bool fastx;
  };
  auto home_setup = [&](const int q, Home& h) __attribute__((always_inline)) {
    int sgi = 0;
#pragma unroll
    for (int k = 1; k < NHSEG; ++k) sgi += (q >= T.hoff[k]) ? 1 : 0;
    const int inrun = q - T.hoff[sgi];
    const int p = T.hstart[sgi] + inrun;
    const int ly = sgi % HY, lz = sgi / HY;
    const int hr = (lz + 1) * SY + (ly + 1);
    const int eh = inrun + T.celloff[hr][1];
    int lx = 0;
    for (int k = 2; k <= hx; ++k) lx += (eh >= T.celloff[hr][k]) ? 1 : 0;
    const int sself = T.rowoff[hr] + eh;
    const CHEM_LDS float* self = img + (sself >> 2) * kGrpF + (sself & 3);
    const float xix = self[0], xiy = self[4], xiz = self[8];             // relative to the stencil's lower corner
    h.p = p; h.ly = ly; h.lz = lz; h.sself = sself; h.xix = xix; h.xiy = xiy; h.xiz = xiz;
    h.cq = rl2 + kListDelta - self[12];
    const int ti = (int)x4[p].w & 15;                 // home cells carry no periodic shift: x4[p] is the staged particle
    h.tmrow = tmask + ti * L.nwords;
    int e0 = 0, e1 = 0;
    if (has_excl && ablate != 5) { const int tg = tag[p]; e0 = excl_start[tg]; e1 = excl_start[tg + 1]; }      // (ablate 5, diagnostic: exclusions ignored)
    h.e0 = e0; h.e1 = e1;
    // Exclusions without leaving the plain path: the few excluded partners of a particle are located
    // in the staged tile ONCE (tag -> index -> position -> cell -> slot, the binning arithmetic repeated on the same
    // bits) and their bits are cleared from the hit masks, like the self pair.  More than 4 exclusions: generic path.
    // On a slab (z-ghost mode) a partner across the slab boundary is a GHOST copy with its own index: rtag names the real
    // particle where it is owned here, else the ghost; gtag names the ghost copy in any case (a one-rank slab holds both).
    // The copy that counts is the one in a cell layer next to the home particle's (a partner is closer than one cell edge).
    int xs0 = -1, xs1 = -1, xs2 = -1, xs3 = -1;
    bool fastx = false;
    if (bx && e1 > e0 && e1 - e0 <= 4 && !nlist) {
      fastx = true;
      const int org = T.geom[6];
      const int nx = bx->nc[0], ny = bx->nc[1], nz = bx->nc[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int slot = -1;
        if (e0 + k < e1) {
          const int tj = excl_list[e0 + k];
          int g = rtag[tj];
          for (int copy = 0; copy < 2 && slot < 0; ++copy) {      // (second trip: slabs only, the tag's ghost copy)
            if (copy) { if (!gtag) break; const int g2 = gtag[tj]; if (g2 == g) break; g = g2; }
            if (g < 0) continue;
            const Vec4<RS> xg = x4[g];
            const int cx = pos_cell(xg.x, 0, nx, *bx), cy = pos_cell(xg.y, 1, ny, *bx);   // (the binning arithmetic on the same bits)
            int kx = cx - (org & 1023) + 1, ky = cy - ((org >> 10) & 1023) + 1, kz;
            kx += kx < 0 ? nx : 0; kx -= kx >= nx ? nx : 0;
            ky += ky < 0 ? ny : 0; ky -= ky >= ny ? ny : 0;
            if (bx->zghost) {      // local layer: ghosts by their index range, reals by the binning arithmetic (dev_bin)
              const int lzc = g < real0 ? 0 : (g >= real1 ? nz - 1 : pos_cell(xg.z, 2, bx->nzg, *bx) - bx->z0g + 1);
              kz = lzc - (org >> 20) + 1;
              const int dl = kz - (lz + 1);
              if (kz < 0 || dl < -1 || dl > 1) continue;      // the far copy (or none here)
            } else {
              kz = pos_cell(xg.z, 2, nz, *bx) - (org >> 20) + 1;
              kz += kz < 0 ? nz : 0; kz -= kz >= nz ? nz : 0;
            }
            if (kx < hx + 2 && ky < T.geom[1] + 2 && kz < T.geom[2] + 2) {
              const int rr = kz * SY + ky, off = g - T.cellg[rr][kx];
              if (off >= 0 && off < T.celloff[rr][kx + 1] - T.celloff[rr][kx]) slot = T.rowoff[rr] + T.celloff[rr][kx] + off;
              else ctl->excl_slot_error = 1;
            }
          }
        }
        if (k == 0) xs0 = slot; else if (k == 1) xs1 = slot; else if (k == 2) xs2 = slot; else xs3 = slot;
      }
    }
    h.xs0 = xs0; h.xs1 = xs1; h.xs2 = xs2; h.xs3 = xs3; h.fastx = fastx;
    // x-window of a stencil row: a candidate in row (dy, dz) is at least (ddy, ddz) away in y and z (distance of the
    // home particle from that row's slab), so only x within sqrt(rl^2 - ddy^2 - ddz^2) can be a neighbour -- 46 % of the
    // 3-cell run on average.  `weps` absorbs every rounding difference between the binning arithmetic and this one (the
    // slices only prune, the distance test decides membership).
    const float ylo = ((float)(ly + 1) - kRefCells) * clen1, zlo = ((float)(lz + 1) - kRefCells) * clen2;   // (image coordinates are relative to T.org)
    h.dylo = fmaxf(xiy - ylo - weps, 0.f); h.dyhi = fmaxf(ylo + clen1 - xiy - weps, 0.f);
    h.dzlo = fmaxf(xiz - zlo - weps, 0.f); h.dzhi = fmaxf(zlo + clen2 - xiz - weps, 0.f);
    h.sxi = (xix + kRefCells * clen0) * subinv;
    h.fmin = lx * NSUB; h.fmax = (lx + 3) * NSUB - 1;
  };
  // Inline bonds (force kernel epilogue).  The host enables this only where the exclusion set IS the bond set and all bonds
  // share one harmonic parameter set (chain-growth systems: every reaction bond is excluded, nothing else is): the LDS slots
  // of the excluded partners are the bonded partners -- recorded as they are (a BondRec of four 16-bit slots per home particle, a second one behind a full first),
  // no bonded table is consulted.  Located partners (<= 4 exclusions) are written here; on the generic path (5..8 exclusions,
  // or int32 rows wanted) every excluded hit is recorded as it is met in the sweep below.  More than kBondSlots exclusions:
  // the particle's bonds stay with the work list.
  auto bonds_located = [&](const Home& h) __attribute__((always_inline)) {
    unsigned int w0 = ~0u, w1 = ~0u, w2 = ~0u, w3 = ~0u;
    if (h.fastx) {
      if (h.xs0 >= 0) w0 = (unsigned int)h.xs0; else if (h.e0 + 0 < h.e1) ctl->bond_slot_miss = 1;
      if (h.xs1 >= 0) w1 = (unsigned int)h.xs1; else if (h.e0 + 1 < h.e1) ctl->bond_slot_miss = 1;
      if (h.xs2 >= 0) w2 = (unsigned int)h.xs2; else if (h.e0 + 2 < h.e1) ctl->bond_slot_miss = 1;
      if (h.xs3 >= 0) w3 = (unsigned int)h.xs3; else if (h.e0 + 3 < h.e1) ctl->bond_slot_miss = 1;
    }
    bslots.rec0[h.p] = bond_rec_pack(w0, w1, w2, w3);
    if (w3 != ~0u) bslots.rec1[h.p] = bond_rec_none();   // (the second word is only read behind a full first one)
  };
  auto window = [&](const Home& h, const int dzy, int& a, int& b) __attribute__((always_inline)) {
    const int dz = dzy / 3, dy = dzy - 3 * dz;
    const int r = (h.lz + dz) * SY + (h.ly + dy);
    const float ddy = dy == 0 ? h.dylo : (dy == 2 ? h.dyhi : 0.f), ddz = dz == 0 ? h.dzlo : (dz == 2 ? h.dzhi : 0.f);
    const float w2 = rl2 - ddy * ddy - ddz * ddz;
    int f_lo = h.fmin, f_hi = h.fmax;
    if (!nowin) {
      const float ws = (__builtin_amdgcn_sqrtf(fmaxf(w2, 0.f)) + weps) * subinv;
      const int g_lo = (int)(h.sxi - ws), g_hi = (int)(h.sxi + ws);     // truncation == floor where it matters (clamped at >= fmin)
      f_lo = g_lo > h.fmin ? g_lo : h.fmin; f_lo = f_lo < h.fmax ? f_lo : h.fmax; f_hi = g_hi < h.fmax ? g_hi : h.fmax; f_hi = f_hi > h.fmin ? f_hi : h.fmin;
    }
    const int ro = T.rowoff[r];
    a = ro + (int)((const volatile CHEM_LDS unsigned short*)bnd)[r * NBND + f_lo];
    b = ro + (int)((const volatile CHEM_LDS unsigned short*)bnd)[r * NBND + f_hi + 1];
    b = b < total ? b : total;
    if (w2 < 0.f) b = a;                                            // the whole row is out of reach
  };
  // The 32 slots from s0 of the window [a, b): candidates within the list radius, the self pair taken out (candidate u ->
  // bit 31-u); tm = type-pair filter of the same slots.
  auto segment = [&](const Home& h, const int s0, const int a, const int b, unsigned int& tm) __attribute__((always_inline)) -> unsigned int {
    const f32x2 ax = {2.f * h.xix, 2.f * h.xix}, ay = {2.f * h.xiy, 2.f * h.xiy}, az = {2.f * h.xiz, 2.f * h.xiz}, cc = {h.cq, h.cq};
    const int len = (b - s0) < 32 ? (b - s0) : 32;
    const int ng = (len + 3) >> 2;
    lds_f32x4* gp = (lds_f32x4*)(l3) + (kGrpF / 4) * (s0 >> 2);
    const unsigned int w0 = h.tmrow[s0 >> 5], w1 = h.tmrow[(s0 >> 5) + 1];
    // two groups per trip, ping-pong registers: the reads of the group after next are in flight while one is tested
    f32x4 X0 = gp[0], Y0 = gp[1], Z0 = gp[2], Q0 = gp[3];
    unsigned int miss = 0;
    auto test4 = [&](const f32x4& X, const f32x4& Y, const f32x4& Z, const f32x4& Q) {
      f32x2 lo = cc - Q.xy, hi = cc - Q.zw;                       // sign bit set at the end: outside
      lo = __builtin_elementwise_fma(az, Z.xy, lo); hi = __builtin_elementwise_fma(az, Z.zw, hi);
      lo = __builtin_elementwise_fma(ay, Y.xy, lo); hi = __builtin_elementwise_fma(ay, Y.zw, hi);
      lo = __builtin_elementwise_fma(ax, X.xy, lo); hi = __builtin_elementwise_fma(ax, X.zw, hi);
      miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(lo.x), 31);
      miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(lo.y), 31);
      miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(hi.x), 31);
      miss = __builtin_amdgcn_alignbit(miss, __float_as_uint(hi.y), 31);
    };
    const int ng2 = (ng + 1) & ~1;                                // (the odd group's bits fall behind `len` and are masked)
    for (int g = 0; g < ng2; g += 2) {
      const f32x4 X1 = gp[kGrpF / 4], Y1 = gp[kGrpF / 4 + 1], Z1 = gp[kGrpF / 4 + 2], Q1 = gp[kGrpF / 4 + 3];
      test4(X0, Y0, Z0, Q0);
      gp += 2 * (kGrpF / 4);
      X0 = gp[0]; Y0 = gp[1]; Z0 = gp[2]; Q0 = gp[3];             // (up to two groups past the run: allocated, never used)
      test4(X1, Y1, Z1, Q1);
    }
    unsigned int m = ng2 < 8 ? ~miss << (32 - 4 * ng2) : ~miss;  // candidate u -> bit 31-u
    m &= ~(len < 32 ? (0xffffffffu >> len) : 0u);                 // slots behind the run
    m &= 0xffffffffu >> (a > s0 ? a - s0 : 0);                    // slots in front of a run that starts inside a group
    const int sh = s0 & 31;
    tm = sh ? __builtin_amdgcn_alignbit(w0, w1, 32 - sh) : w0;    // type-pair filter of these 32 slots
    const unsigned int ks = (unsigned int)(h.sself - s0);
    if (ks < 32u) m &= ~(0x80000000u >> ks);
    return m;
  };
  // the located exclusions of a plain home taken out of a segment's hits (like the self pair)
  auto clear_located = [&](const Home& h, const int s0, unsigned int m) __attribute__((always_inline)) -> unsigned int {
    const unsigned int k0 = (unsigned int)(h.xs0 - s0), k1 = (unsigned int)(h.xs1 - s0), k2 = (unsigned int)(h.xs2 - s0), k3 = (unsigned int)(h.xs3 - s0);
    if (k0 < 32u) m &= ~(0x80000000u >> k0);
    if (k1 < 32u) m &= ~(0x80000000u >> k1);
    if (k2 < 32u) m &= ~(0x80000000u >> k2);
    if (k3 < 32u) m &= ~(0x80000000u >> k3);
    return m;
  };

  // one lane sweeps the nine rows of home particle q
  auto sweep = [&](const int q) __attribute__((always_inline)) {
    Home h;
    home_setup(q, h);
    const int p = h.p, e0 = h.e0, e1 = h.e1;
    const bool fastx = h.fastx;
    int cnt = 0, cnt16 = 0;
    int* row32 = nlist ? nlist + (size_t)p * S : nullptr;
    const bool bsw = (bool)bslots;      // (the record is indexed by the particle's place in the sorted arrays)
    int nbw = 0;
    const bool bond_rec = bsw && !fastx && e1 > e0 && e1 - e0 <= kBondSlots;      // generic path records while sweeping
    if (bsw && (fastx || e1 == e0)) bonds_located(h);
    const bool plain = (e1 == e0 || fastx) && !row32;
    uint4* regq = reinterpret_cast<uint4*>(reg16) + q;   // chunk c of this particle: regq[c * nhome]
    // accepted slots are shifted into a 128-bit register; every 8th append stores one whole 16-byte chunk (one
    // predicated 2-byte store per hit instead was measured slower: tile phase 269 -> 284 us)
    uint4 acc = make_uint4(0, 0, 0, 0);
    auto push = [&](unsigned int sl) {
      acc.x = __builtin_amdgcn_alignbit(acc.y, acc.x, 16);
      acc.y = __builtin_amdgcn_alignbit(acc.z, acc.y, 16);
      acc.z = __builtin_amdgcn_alignbit(acc.w, acc.z, 16);
      acc.w = (acc.w >> 16) | (sl << 16);
      if ((cnt16 & 7) == 7 && cnt16 < S16 && ablate != 2) regq[(size_t)(cnt16 >> 3) * nhome] = acc;
      ++cnt16;
    };
    int a_n, b_n;
    window(h, 0, a_n, b_n);
#pragma unroll 1
    for (int dzy = 0; dzy < 9; ++dzy) {
      const int a = a_n, b = b_n;
      if (dzy < 8) window(h, dzy + 1, a_n, b_n);
      const int r = (h.lz + dzy / 3) * SY + (h.ly + dzy % 3);
      for (int s0 = a & ~3; s0 < b; s0 += 32) {
        unsigned int tm;
        unsigned int m = segment(h, s0, a, b, tm);
        if (ablate == 3) { cnt16 += __popc(m & tm); continue; }
        if (plain) {
          // no exclusions (or located as slots) and no int32 row: a hit needs nothing from memory
          m &= tm;
          if (fastx) m = clear_located(h, s0, m);
          while (m) {
            const int k = __clz((int)m);
            m &= ~(0x80000000u >> k);
            push((unsigned int)(s0 + k));
          }
        } else {
          while (m) {
            const int k = __clz((int)m);
            const unsigned int bit = 0x80000000u >> k;
            m &= ~bit;
            const int sl = s0 + k;
            // global index of the slot from the row's cell tables (this path is rare: int32 rows wanted, or > 4 exclusions)
            const int e = sl - T.rowoff[r];
            int kc = 0;
#pragma unroll
            for (int qq = 1; qq < SX; ++qq) kc += (e >= T.celloff[r][qq]) ? 1 : 0;
            const int j = T.cellg[r][kc] + (e - T.celloff[r][kc]);
            const CHEM_LDS float* cj = img + (sl >> 2) * kGrpF + (sl & 3);
            const float ddx = h.xix - cj[0], ddy = h.xiy - cj[4], ddz = h.xiz - cj[8];
            const bool exact = ddx * ddx + ddy * ddy + ddz * ddz <= rl2_rows;  // difference form: the mask is a superset by the delta shell
            bool ok = true;
            if (e1 > e0) {
              const int tgj = tag[j];
              for (int ee = e0; ee < e1; ++ee) if (excl_list[ee] == tgj) { ok = false; break; }
              if (!ok && bond_rec && nbw < kBondSlots) *bond_rec_slot(bslots, (size_t)p, nbw++) = (unsigned short)sl;      // inline bonds: an excluded hit is a bonded partner
            }
            if (ok) {
              if (tm & bit) push((unsigned int)sl);      // (shell pairs included, as on the plain path: the force list does not depend on the path)
              if (row32 && exact) { if (cnt < S) row32[cnt] = j; ++cnt; }
            }
          }
        }
      }
    }
    if (bsw && !fastx && e1 > e0) {       // generic path: close the record (or leave it empty for a particle the work list keeps)
      if (bond_rec && nbw != e1 - e0) ctl->bond_slot_miss = 1;      // every excluded (= bonded) partner sits within the list radius
      for (int k = bond_rec ? nbw : 0; k < kBondSlots; ++k) *bond_rec_slot(bslots, (size_t)p, k) = (unsigned short)kBondRecNone;      // (both words, whatever the first holds: this path is rare)
    }
    // pad the last chunk with the far-away dummy slot (chunks are read whole)
    const int real16 = cnt16;
    if (real16 <= S16) while (cnt16 & 7) push((unsigned int)total);
    nnh[hbase + q] = row_word(ablate >= 2 ? (real16 < 0 ? 1 : 0) : (real16 < S16 ? real16 : S16), q);   // (diagnostic builds of the list leave no usable chunks)
    if (real16 > S16) atomicMax(&ctl->nl_overflow, real16);
    if (row32) {
      const int c32 = cnt < S ? cnt : S;
      for (int k = c32; k < ((c32 + 3) & ~3); ++k) row32[k] = p;
      nn[p] = c32;
      if (cnt > S) atomicMax(&ctl->nl_overflow, cnt);
    }
  };

  // Full passes of BS home particles, one lane each.  A tile of the flagship holds 578: the 66 behind the first pass would
  // cost the workgroup a second nine-row sweep on two waves while six wait, so they go to the cooperative rounds below --
  // unless those would be no shorter than two ordinary passes (more than 2 BS / 9 left over: crowded tiles).
  // Cooperative round: nine adjacent lanes per home particle (seven homes per wave, lane 63 idle), lane `row` owns stencil
  // row `row`.  Every lane tests its row's window and keeps the final hit masks (up to four segments = 128 slots) in
  // registers; an exclusive prefix of the hit counts over the nine lanes places each lane's hits in the home's chunks, so
  // the entries come out in the order of the one-lane sweep: rows 0..8, ascending slots inside a row.  A home this form
  // does not cover (generic exclusion path, a window beyond the kept masks) is handed to one lane of the wave, which
  // sweeps it in the next trip of the loop: one loop, so that the sweep exists once in the kernel (a second inlined copy
  // costs the kernel 100 bytes of scratch per lane).
  const int nrem = nhome % BS, nfull = nhome - nrem;
  const bool coop = coop_on && ablate == 0 && !nlist && nrem > 0 && 9 * nrem <= 2 * BS;
  const int npass = coop ? nfull / BS : (nhome + BS - 1) / BS;
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int hl = ln / 9, row = ln - 9 * hl;
  constexpr int kRound = 7 * (BS / 64);      // homes per cooperative round of the workgroup
  const int ncr = (coop && nrem > 7 * wv) ? (nrem - 7 * wv + kRound - 1) / kRound : 0;      // rounds of this wave
  int qf = -1;      // home this lane sweeps alone in the next trip (fallback of a cooperative round)
  for (int it = 0; it < npass + (ncr > 0 ? ncr + 1 : 0); ++it) {      // (wave-uniform)
    int q = qf;
    if (it < npass) {
      q = it * BS + (int)threadIdx.x;
      if (q >= nhome) q = -1;
      if (ablate == 4 && q >= BS) { nnh[hbase + q] = row_word(0, q); q = -1; }      // (diagnostic: what the sweeps behind the first pass cost)
    } else if (it - npass < ncr) {
      qf = -1;
      const int q0 = nfull + 7 * wv + kRound * (it - npass), qc = q0 + hl;
      const bool live = ln < 63 && qc < nhome;
      unsigned int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
      int s00 = 0;
      bool fb = false;      // this home falls back to the one-lane sweep
      if (live) {
        Home h;
        home_setup(qc, h);      // (redundantly in the nine lanes: the same loads from the same addresses)
        if (!(h.e1 == h.e0 || h.fastx)) fb = true;
        else {
          int a, b;
          window(h, row, a, b);
          s00 = a & ~3;
          if (b - s00 > 128) fb = true;
          else {
            if (row == 0 && bslots) bonds_located(h);
            int k = 0;
            for (int s0 = s00; s0 < b; s0 += 32, ++k) {
              unsigned int tm;
              unsigned int m = segment(h, s0, a, b, tm) & tm;
              if (h.fastx) m = clear_located(h, s0, m);
              if (k == 0) m0 = m; else if (k == 1) m1 = m; else if (k == 2) m2 = m; else m3 = m;
            }
          }
        }
      }
      // a home falls back as a whole: the verdicts of its nine lanes are collected from the wave's ballot
      const bool hfb = live && ((__ballot(fb) >> (9 * hl)) & 0x1ffull) != 0ull;
      if (hfb) { m0 = 0; m1 = 0; m2 = 0; m3 = 0; }
      const int c = __popc(m0) + __popc(m1) + __popc(m2) + __popc(m3);
      int incl = c;      // inclusive prefix over the home's nine lanes
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) { const int v = __shfl_up(incl, d); if (row >= d) incl += v; }
      if (live && !hfb) {
        int e = incl - c;
        unsigned short* const regq = reg16 + (size_t)qc * 8;      // entry e of this particle: regq[(e >> 3) * nhome * 8 + (e & 7)]
        auto peel = [&](unsigned int m, const int s0) {
          while (m) {
            const int k = __clz((int)m);
            m &= ~(0x80000000u >> k);
            if (e < S16) regq[(size_t)(e >> 3) * nhome * 8 + (e & 7)] = (unsigned short)(s0 + k);
            ++e;
          }
        };
        peel(m0, s00); peel(m1, s00 + 32); peel(m2, s00 + 64); peel(m3, s00 + 96);
        if (row == 8) {      // e = the home's row count: pad the last chunk with the far-away dummy slot, as the one-lane sweep does
          const int real16 = e;
          if (real16 <= S16) for (; e & 7; ++e) regq[(size_t)(e >> 3) * nhome * 8 + (e & 7)] = (unsigned short)total;
          nnh[hbase + qc] = row_word(real16 < S16 ? real16 : S16, qc);
          if (real16 > S16) atomicMax(&ctl->nl_overflow, real16);
        }
      }
      // fallback homes of this round: lane j takes the j-th of them (bit 9 hl of the ballot: home hl)
      unsigned long long hm = __ballot(hfb && row == 0);
      if (ln < __popcll(hm)) {
        for (int j = 0; j < ln; ++j) hm &= hm - 1;
        qf = q0 + (__ffsll((long long)hm) - 1) / 9;
      }
    }
    if (q >= 0) sweep(q);
  }
}

template <typename R, int BS>
__global__ __launch_bounds__(BS, 4) void k_nlist_tiles(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                    const TileLDS<R>* __restrict__ desc, R rl2,
                                                    const int* __restrict__ excl_start, const int* __restrict__ excl_list, int has_excl,
                                                    ActMask act, int ntypes, unsigned short* __restrict__ nl16, int S16, int* __restrict__ nnh,
                                                    int* __restrict__ nlist, int S, int* __restrict__ nn, DevCtl* ctl, R rl2_rows, BondRecs bslots,
                                                    const Box<R>* __restrict__ boxp, const int* __restrict__ rtag, const int* __restrict__ gtag, int real0, int real1, int coop) {
  // (rl2: the radius the 16-bit force list is built for, rc + list skin; rl2_rows: the int32 Verlet rows', rc + skin;
  //  boxp/rtag/gtag/real0/real1: located-partner path of the exclusions on a slab, boxp == nullptr: generic path)
  if (!ctl->need_rebuild) return;
  __shared__ TileLDS<R> T;
  __shared__ Box<R> sbox;
  if (boxp) { const int* bs_ = reinterpret_cast<const int*>(boxp); int* bd_ = reinterpret_cast<int*>(&sbox); for (int k = threadIdx.x; k < (int)(sizeof(Box<R>) / 4); k += BS) bd_[k] = bs_[k]; }
  CHEM_DYN_LDS(R);
  for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    const int tile = xcd_remap(vb, ntiles);     // gridDim.x is a multiple of 8: vb % 8 == blockIdx.x % 8
    __syncthreads();
    tile_load_desc<R>(T, desc, tile);
    const bool f32list = sizeof(R) == 4 || !nlist;      // fp64: the exact list build only where the int32 rows are wanted
    if (f32list) list_stage_clear<BS>(chem_dyn_lds, list_lds_layout(CAP, ntypes), ntypes);
    __syncthreads();
    if (f32list) {
      const ListLDS L = list_lds_layout(CAP, ntypes);
      list_stage_f32<R, BS>(T, chem_dyn_lds, L, CAP, x4, act, ntypes);
      __syncthreads();
      dev_nlist_tile_f32<R, BS>(T, chem_dyn_lds, L, tag, (float)rl2, excl_start, excl_list, has_excl, nl16, S16, nnh, nlist, S, nn, ctl,
                                boxp ? (const Box<R>*)&sbox : (const Box<R>*)nullptr, rtag, x4, 0, (float)rl2_rows, bslots, gtag, real0, real1, coop);      // (bslots: inline bonds, see dev_nlist_tile_f32)
    } else {
      tile_fill<R, BS, true>(T, sx, CAP, x4, 1);
      __syncthreads();
      dev_nlist_tile<R, BS>(T, sx, tag, rl2, excl_start, excl_list, has_excl, act, nl16, S16, nnh, nlist, S, nn, ctl, nullptr, nullptr, nullptr, rl2_rows);
    }
  }
}

// exclusive scan of the home-particle counts of all tiles -> geom[5] (base of the tile's region
// in the transposed 16-bit list / count array); single block
template <typename R>
__global__ __launch_bounds__(1024) void k_tile_scan(int ntiles, TileLDS<R>* __restrict__ desc, const DevCtl* ctl) {
  if (!ctl->need_rebuild) return;
  __shared__ int wsum[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int w = threadIdx.x >> 6;
  for (int base = 0; base < ntiles; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < ntiles ? desc[i].geom[4] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o); if (lane_id() >= o) incl += t; }
    if (lane_id() == 63) wsum[w] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int k = 0; k < 16; ++k) { if (k < w) woff += wsum[k]; tot += wsum[k]; }
    if (i < ntiles) desc[i].geom[5] = carry_s + woff + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) carry_s += tot;
    __syncthreads();
  }
}

// ---- pair forces on tiles --------------------------------------------------------------
template <typename R, bool ENERGY, bool LJONLY, bool CUBIC = false, bool CAPPED = false>
__device__ __forceinline__ void pair_accum(const PairCore<R> pc, const PairExt<R>* __restrict__ pext, int pidx,
                                           const Vec4<R>* __restrict__ tab, R r2, R dx, R dy, R dz,
                                           R& fx, R& fy, R& fz, double& e_lj, double& e_tab, double& vir, R c2 = (R)0) {
  if (LJONLY && !ENERGY) {
    const R r2i = rcp_r(r2), r6i = r2i * r2i * r2i;
    R ff = r6i * (pc.lj1 * r6i - pc.lj2) * r2i;
    ff = (r2 <= pc.rc2) ? ff * pc.kind : (R)0;   // kind (1 for LJ) keeps the read a single ds_read_b128 (b96 costs 2x the LDS cycles)
    fx += ff * dx; fy += ff * dy; fz += ff * dz;
  } else {
    pair_term<R, ENERGY, CUBIC, CAPPED>(pc, pext, pidx, tab, r2, dx, dy, dz, fx, fy, fz, e_lj, e_tab, vir, c2);
  }
}

// One neighbour = one ds_read_b128.  Where .w is not used (uniform LJ) the compiler narrows a plain float4 read to
// ds_read_b96, which takes 8 LDS-array cycles per wave instead of 4 (MI355X_MICROARCH.md, LDS table): the volatile
// 16-byte access keeps the width.
__device__ __forceinline__ float4 lds_gather4(const float4* sx, unsigned int slot) {
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  const f32x4_ v = *((const volatile __attribute__((address_space(3))) f32x4_*)sx + slot);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ double4 lds_gather4(const double4* sx, unsigned int slot) { return sx[slot]; }
// fp64 force kernel, 24-byte slots: coordinates only (the type is read from the byte array where a mode needs it)
__device__ __forceinline__ double4 lds_gather3d(const double4* sx, unsigned int slot) {
  const double* s3 = reinterpret_cast<const double*>(sx) + 3 * slot;
  return make_double4(s3[0], s3[1], s3[2], 0.0);
}
template <typename R> __device__ __forceinline__ Vec4<R> lds_gather4(const Vec4<R>* sx, unsigned int slot) { return lds_gather4(sx, slot); }

struct UniLJ { float rc2, lj1, lj2, pad; double drc2, dlj1, dlj2; };   // all listed pairs share one LJ parameter set

// One workgroup per tile; TPP lanes per home particle (lane `sub` takes chunks sub, sub+TPP, ...).
// MODE 0: general (type-pair table in LDS, tables allowed)  1: LJ/off pairs only, branch-free
//      2: uniform LJ -- every listed pair has the same parameters (kernel arguments / SGPRs)
//      3: general as 0, with the piecewise-cubic table kind (launched only while a type pair of kind 3 exists)
//      4: general as 3, plus the truncated Coulomb term (launched only while a Coulomb pair is registered; TPP 1, 512 threads).
//         One charge word per slot is staged behind the image (coul_q_offset), read with the slot; the home particle's k*q,
//         its row of the type-pair mask and rc_qq^2 are registers.  No inline bonds in this mode (the host keeps them off).
//      5: general as 3, with marked type pairs scaled by lambda_i lambda_j and capped (launched only while a type pair is marked
//         by chem_nb_resolution; TPP 1, 512 threads, k_pair_tiles_res).  One lambda word per slot is staged where MODE 4 keeps
//         its charge words (the two terms are not served together), computed in tile_fill; the home particle's lambda and its
//         row of the resolution mask are registers, the pairs' caps are staged in LDS beside spc[].  No inline bonds.
//      6: general as 3, with capped type pairs (launched only while a type pair is capped by chem_nb_cap; TPP 1, 512 threads,
//         k_pair_tiles_cap).  The squared cap radii are staged in LDS beside spc[]; no word per slot.  No inline bonds.
//      7: 5 and 6 together (k_pair_tiles_rescap): marked type pairs and capped type pairs in one context, never the same pair.
// Tiles of one launch: [base1, base1+n1) followed by [base2, ...).  The decomposed path launches the
// tiles whose stencil stays inside the own layers ("interior": they need no ghost) while the halo
// exchange is still in flight on the communication stream, and the two boundary tile layers after it.
struct TileSub { int base1, n1, base2; };
// guard == 2 (decomposed path): every workgroup of the force kernel takes the rebuild decision itself from the P
// gathered step maxima (same inputs, same arithmetic: same result), workgroup 0 publishes it -- control block, pinned
// host words the host polls -- and all leave at once when a rebuild is due: no one-block decision launch between the
// halo exchange and the forces.  The accumulated distance is double-buffered by step parity (read [par], written [par^1]).
// LDS slot of particle g (sorted index, position xg) in the staged image of the tile described by T; -1: outside its stencil.
// (cell of g by the binning arithmetic on the same bits, relative to the tile's first home cell with the periodic wrap)
// Slabs (bx.zghost): the local layer of a ghost follows from its index range (below real0: lower ghost layer, from real1 on:
// upper), that of a real particle from the binning arithmetic; hz = stencil row (z) of the home particle -- only a copy in a
// layer next to it counts (a one-rank slab holds a particle and its ghost, possibly both inside one stencil).
template <typename R>
__device__ __forceinline__ int tile_partner_slot(const TileLDS<R>& T, int g, const Vec4<R>& xg, const Box<R>& bx, DevCtl* ctl,
                                                 const int real0 = 0, const int real1 = 0x7fffffff, const int hz = 0) {
  const int nx = bx.nc[0], ny = bx.nc[1], nz = bx.nc[2], org = T.geom[6];
  int kx = pos_cell(xg.x, 0, nx, bx) - (org & 1023) + 1, ky = pos_cell(xg.y, 1, ny, bx) - ((org >> 10) & 1023) + 1, kz;
  kx += kx < 0 ? nx : 0; kx -= kx >= nx ? nx : 0;
  ky += ky < 0 ? ny : 0; ky -= ky >= ny ? ny : 0;
  if (bx.zghost) {
    const int lzc = g < real0 ? 0 : (g >= real1 ? nz - 1 : pos_cell(xg.z, 2, bx.nzg, bx) - bx.z0g + 1);
    kz = lzc - (org >> 20) + 1;
    if (kz < 0 || kz - hz < -1 || kz - hz > 1) return -1;
  } else {
    kz = pos_cell(xg.z, 2, nz, bx) - (org >> 20) + 1;
    kz += kz < 0 ? nz : 0; kz -= kz >= nz ? nz : 0;
  }
  if (kx < T.geom[0] + 2 && ky < T.geom[1] + 2 && kz < T.geom[2] + 2) {
    const int rr = kz * SY + ky, off = g - T.cellg[rr][kx];
    if (off >= 0 && off < T.celloff[rr][kx + 1] - T.celloff[rr][kx]) return T.rowoff[rr] + T.celloff[rr][kx] + off;
    ctl->excl_slot_error = 1;
  }
  return -1;
}
// The list build of the bond pass (bond_mode 2) ignores the exclusions; the partner slots of every home particle are recorded
// behind it, once per list lifetime, for the force launches up to the next rebuild (a BondRec per particle, a second one behind
// a full first).  tag -> exclusion row -> partner index -> partner position -> cell -> slot through the tile tables in LDS.
// One lane per home particle of the tile described by T; the loads of each level of the chain are issued for up to four
// partners before the first is consumed, the second word (five to eight partners, rare) takes the same path once more.
// gtag, real0, real1: slabs (the tag's ghost copy, the index range of the real particles), as in tile_partner_slot.
// Runs in the idle tail of k_rebuild_fused (single domain) and as k_bond_slots behind every other list build.  Inlined into the
// rebuild it costs 28 bytes of scratch per lane and no register (128, occupancy 4); as a real call it cost 112.
template <typename R>
__device__ __forceinline__ void bond_slots_quad(const TileLDS<R>& T, const int e0, const int ne, const int* __restrict__ excl_list,
                                                const int* __restrict__ rtag, const int* __restrict__ gtag, const int real0, const int real1,
                                                const Vec4<R>* __restrict__ x4, const Box<R>& bx, const int hz, DevCtl* ctl, unsigned int* w) {
  int tj[4], g[4];
  Vec4<R> xg[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) tj[k] = k < ne ? excl_list[e0 + k] : -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = k < ne ? rtag[tj[k]] : -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) xg[k] = g[k] >= 0 ? x4[g[k]] : Vec4<R>{};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= ne) break;
    int sl = g[k] >= 0 ? tile_partner_slot<R>(T, g[k], xg[k], bx, ctl, real0, real1, hz) : -1;
    if (sl < 0 && gtag) {      // slabs: the tag's ghost copy
      const int g2 = gtag[tj[k]];
      if (g2 >= 0 && g2 != g[k]) sl = tile_partner_slot<R>(T, g2, x4[g2], bx, ctl, real0, real1, hz);
    }
    if (sl < 0) ctl->bond_slot_miss = 1;      // every bonded partner sits inside the stencil (bond length << cell edge)
    else w[k] = (unsigned int)sl;
  }
}
template <typename R>
__device__ __forceinline__ void dev_bond_slots_tile(const TileLDS<R>& T, const int* __restrict__ tag, const int* __restrict__ excl_start,
                                                    const int* __restrict__ excl_list, const int* __restrict__ rtag, const int* __restrict__ gtag,
                                                    const int real0, const int real1, const Vec4<R>* __restrict__ x4, const Box<R>& bx,
                                                    const BondRecs bslots, DevCtl* ctl) {
  const int nhome = T.geom[4];
  for (int q = threadIdx.x; q < nhome; q += (int)blockDim.x) {
    int sgi = 0;
#pragma unroll
    for (int k = 1; k < NHSEG; ++k) sgi += (q >= T.hoff[k]) ? 1 : 0;
    const int p = T.hstart[sgi] + (q - T.hoff[sgi]);
    const int hz = bx.zghost ? sgi / HY + 1 : 0;      // stencil row (z) of the home particle
    const int tg = tag[p];
    const int e0 = excl_start[tg], ne = excl_start[tg + 1] - e0;
    unsigned int w[kBondSlots];
#pragma unroll
    for (int k = 0; k < kBondSlots; ++k) w[k] = ~0u;
    if (ne > 0 && ne <= kBondSlots) {      // (more than kBondSlots: the particle's bonds stay with the work list)
      bond_slots_quad<R>(T, e0, ne < 4 ? ne : 4, excl_list, rtag, gtag, real0, real1, x4, bx, hz, ctl, w);
      if (ne > 4) bond_slots_quad<R>(T, e0 + 4, ne - 4, excl_list, rtag, gtag, real0, real1, x4, bx, hz, ctl, w + 4);
    }
    bslots.rec0[p] = bond_rec_pack(w[0], w[1], w[2], w[3]);
    if (w[3] != ~0u) bslots.rec1[p] = bond_rec_pack(w[4], w[5], w[6], w[7]);      // (only read behind a full first word)
  }
}
// ... behind the list launch of the unfused chain and of a slab rebuild: one workgroup per tile, the tables from desc[]
template <typename R>
__global__ __launch_bounds__(256) void k_bond_slots(int ntiles, const TileLDS<R>* __restrict__ desc, const int* __restrict__ tag,
                                                    const int* __restrict__ excl_start, const int* __restrict__ excl_list,
                                                    const int* __restrict__ rtag, const int* __restrict__ gtag, int real0, int real1,
                                                    const Vec4<R>* __restrict__ x4, const Box<R> box, BondRecs bslots, DevCtl* ctl) {
  if (!ctl->need_rebuild || ctl->halt) return;      // (halt: the rebuild in front of this launch could not finish its lists)
  __shared__ TileLDS<R> T;
  tile_load_desc<R>(T, desc, blockIdx.x);
  __syncthreads();
  dev_bond_slots_tile<R>(T, tag, excl_start, excl_list, rtag, gtag, real0, real1, x4, box, bslots, ctl);
}

// (fold != nullptr: `gathered` holds n * kFoldSlots bit patterns of squared displacements -- every rank's fold words, see
//  k_integrate -- instead of n doubles; `fold` = this rank's words, cleared here for the next step)
// guard 3 (single domain, a step without a neighbour launch): `fold` = both parities of the fold words ([par] read, [par ^ 1]
// cleared for the next step's integrate), `hint` / `gen` / `istep` as in FusedArgs; gathered, n, host_flag and ticket unused.
struct DecideArgs { const double* gathered; int n; volatile int* host_flag; int ticket, par, criterion; double half_skin_ref; unsigned long long* fold;
                    IdleHint* hint; int gen; long long istep; };

// (fp64: the 32-byte-per-slot image allows one or two workgroups per CU anyway -- 128 registers instead of 80 and spills)
// DIAG = true: diagnostic instantiation with per-block phase stamps (`dbg`) and early exits (`ablate`: 1 stop after
// staging, 2 skip staging, 3 descriptor only, 4 dispatch only); the production instantiation carries neither.
// guard != 0: speculative launch of the decomposed path -- leave at once while a rebuild is pending.
// (the body of k_pair_tiles and of k_pair_tiles_q, which alone takes the Coulomb arguments: the kernels of every other mode keep
//  their argument block)
// TENSOR (k_pair_tiles_tensor, K13): as in pair_force_body; tout[6 * block + c]
template <typename R, int TPP, bool ENERGY, int BS, int MODE, bool DIAG, bool TENSOR = false>
__device__ __forceinline__ void pair_tiles_body(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, UniLJ uni, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, int ablate, long long* __restrict__ dbg, TileSub sub_,
                                                   DecideArgs da, const BondRecs bslots,
                                                   double bond_K, double bond_r0, int bond_mode, ActMask bact,
                                                   const CoulArgs<R> ca, const ResArgs<R> ra, const CapArgs<R> cp = CapArgs<R>{},
                                                   double* __restrict__ tout = nullptr) {
  constexpr bool LJONLY = MODE == 1 || MODE == 2, CUBIC = MODE >= 3, COUL = MODE == 4, RES = MODE == 5 || MODE == 7, CAPPED = MODE == 6 || MODE == 7;
#ifndef CHEM_NCH
#define CHEM_NCH 3
#endif
  constexpr int NCH = TPP == 1 ? CHEM_NCH : (TPP == 2 ? 3 : 2);   // chunks (8 slots) each lane preloads before the staging barrier
  long long st0 = 0, st1 = 0, st2 = 0, st3 = 0;
  if (DIAG && dbg) st0 = wall_clock64();
  if (DIAG && ablate == 4) return;   // diagnostic: dispatch cost only
  // guard 3 (no neighbour launch on this step): every workgroup folds the integrate kernel's words and decides, workgroup 0
  // keeps the books and tells the host.  The four loads are issued here and used behind the descriptor's barrier -- one memory
  // latency for both instead of two in a row on every workgroup's critical path.
  unsigned long long g3_w = 0; double g3_acc = 0; int g3_forced = 0, g3_halt = 0;
  static_assert(kFoldSlots == kWave, "guard 3 reads one fold word per lane");
  if (guard == 3) {
    g3_halt = ctl->halt; g3_w = da.fold[da.par * kFoldSlots + lane_id()]; g3_acc = ctl->acc_pp[da.par]; g3_forced = ctl->force_rebuild;
  } else if (guard == 2) {
    double m2;
    if (da.fold) {      // the fold words of all ranks
      const unsigned long long mb = fold_words_max(reinterpret_cast<const unsigned long long*>(da.gathered), da.n * kFoldSlots);
      m2 = sizeof(R) == 4 ? bits_real_f(mb) : bits_real_d(mb);
      if (blockIdx.x == 0 && threadIdx.x < kFoldSlots) da.fold[threadIdx.x] = 0ull;      // (sent already: the exchange is ahead of this launch in the stream)
    } else {
      m2 = da.gathered[0];
      for (int q = 1; q < da.n; ++q) m2 = da.gathered[q] > m2 ? da.gathered[q] : m2;
    }
    const double acc = da.criterion ? sqrt(m2) : ctl->acc_pp[da.par] + sqrt(m2);
    const int forced = ctl->force_rebuild;
    const int need = (acc > half_skin) || forced;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      // (force_rebuild is NOT cleared here: workgroups that start later must read the same value -- the host clears it,
      //  stream-ordered, at the top of the slab rebuild this decision triggers)
      decide_book(ctl, da.par, da.criterion, m2, acc, need, forced ? 1 : 0, da.half_skin_ref);
      da.host_flag[0] = need;
      __threadfence_system();
      da.host_flag[1] = da.ticket;
    }
    if (need) return;
  } else if (guard && ctl->need_rebuild) return;   // speculative launch (decomposed path): the host rebuilds first and launches again
  if (guard != 3 && ctl->halt) return;
  __shared__ TileLDS<R> T;
  __shared__ PairCore<R> spc[kMaxTypes * kMaxTypes];
  CHEM_DYN_LDS(R);
  if (MODE != 2) for (int k = threadIdx.x; k < ntypes * ntypes; k += BS) spc[k] = pcore[k];
  [[maybe_unused]] const R* sfm = nullptr;
  if constexpr (RES) { __shared__ R sfm_[kMaxTypes * kMaxTypes]; res_stage_caps<R>(sfm_, ra.fmax); sfm = sfm_; }      // (the barriers behind the descriptor and the staging cover it)
  [[maybe_unused]] const R* sc2 = nullptr;
  if constexpr (CAPPED) { __shared__ R sc2_[kMaxTypes * kMaxTypes]; cap_stage_radii<R>(sc2_, cp.c2); sc2 = sc2_; }      // (likewise)
  if (guard < 2 && blockIdx.x == 0 && threadIdx.x == 0 && ctl->acc_maxdist > half_skin) ctl->skin_violation = 1;
  const R u_rc2 = sizeof(R) == 4 ? (R)uni.rc2 : (R)uni.drc2, u_lj1 = sizeof(R) == 4 ? (R)uni.lj1 : (R)uni.dlj1,
          u_lj2 = sizeof(R) == 4 ? (R)uni.lj2 : (R)uni.dlj2;
  const int vtile = xcd_remap(blockIdx.x, ntiles);   // ntiles = tiles of THIS launch (all of them, or one of the two subsets below)
  const int tile = vtile < sub_.n1 ? sub_.base1 + vtile : sub_.base2 + (vtile - sub_.n1);
  tile_load_desc<R>(T, desc, tile);
  __syncthreads();
  if (guard == 3) {
    // The host left the launch out on a prediction; if a rebuild is due after all, nothing is counted, the run stops here
    // like behind a full bucket row and the host redoes the step with the launch (nothing but LDS has been written so far).
    if (g3_halt) return;
    const unsigned long long mb = wave_max_u64(g3_w);
    const double m2 = sizeof(R) == 4 ? bits_real_f(mb) : bits_real_d(mb);
    const double acc = g3_acc + sqrt(m2);
    const int need = (acc > half_skin) || g3_forced;
    if (blockIdx.x == 0 && threadIdx.x < kFoldSlots) da.fold[(da.par ^ 1) * kFoldSlots + threadIdx.x] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (need) {
        if (!g3_forced) ctl->force_rebuild = 2;
        ctl->halt_step = da.istep; ctl->halt_par = da.par; ctl->halt = 2;
        if (da.hint) { volatile IdleHint* h = da.hint; h->halted = da.gen; }
      } else {
        decide_book(ctl, da.par, 0, m2, acc, 0, 0, da.half_skin_ref);
        publish_hint(da.hint, da.gen, da.istep, acc, sqrt(m2));
      }
    }
    if (need) return;
  }
  if (DIAG && ablate == 3) return;   // diagnostic: descriptor load only
  if (DIAG && dbg) st1 = wall_clock64();
  const int nhome = T.geom[4], hbase = T.geom[5];
  const int slice = threadIdx.x / TPP, sub = threadIdx.x % TPP;
  constexpr int NSL = BS / TPP;
  const uint4* reg = reinterpret_cast<const uint4*>(nl16 + (size_t)hbase * S16);
  // first pass's list/count loads are issued before the staging barrier so that their latency
  // overlaps the stencil loads
  int p = -1, cnt = 0, hslot = 0, qq = 0;
  uint4 pkv[NCH];
  BondRec bwv = bond_rec_none();
#ifndef CHEM_NT_PRE
#define CHEM_NT_PRE 1
#endif
  // (row order, chem_roworder_host.hpp: position q of the tile's list holds the row of the home named in the upper half of
  //  its count word; the count and the chunks go by position, the particle and its slot by the home)
  auto locate = [&](int q) {
    const int cw = nnh[hbase + q];
    const int qn = row_word_home(cw);
    int sgi = 0;
#pragma unroll
    for (int k = 1; k < NHSEG; ++k) sgi += (qn >= T.hoff[k]) ? 1 : 0;
    const int inrun = qn - T.hoff[sgi];
    p = T.hstart[sgi] + inrun; qq = q;
    const int hr = (sgi / HY + 1) * SY + (sgi % HY + 1);
    hslot = T.rowoff[hr] + T.celloff[hr][1] + inrun;      // the home particle's own slot in the staged tile
    cnt = row_word_count(cw);
    if (bslots) bwv = bslots.rec0[p];   // (inline bonds: first word, issued with the list chunks, consumed after the pair loop)
#pragma unroll
    for (int c = 0; c < NCH; ++c)                           // the tile's region is always allocated: safe before cnt is known
      pkv[c] = (sub + c * TPP) * 8 < S16 ? (CHEM_NT_PRE ? nt_load_u4(&reg[(size_t)(sub + c * TPP) * nhome + q]) : reg[(size_t)(sub + c * TPP) * nhome + q]) : make_uint4(0, 0, 0, 0);
  };
  if (slice < nhome) locate(slice);
  constexpr bool D3 = sizeof(R) == 8;     // fp64: 24-byte slots + type bytes (see tile_fill)
  [[maybe_unused]] R* const sq = reinterpret_cast<R*>(chem_dyn_lds + ((COUL || RES) ? coul_q_offset<R>(CAP) : 0));
  if constexpr (COUL) tile_fill<R, BS, false, D3, true>(T, sx, CAP, x4, 0, ca.tag, ca.qtag, sq);
  else if constexpr (RES) tile_fill<R, BS, false, D3, true, true>(T, sx, CAP, x4, 0, ra.tag, nullptr, sq, ResFill{ra.stamp, ra.alpha, ra.step});
  else if (!DIAG || ablate != 2) tile_fill<R, BS, false, D3>(T, sx, CAP, x4, 0);
  __syncthreads();
  if (DIAG && ablate == 1) return;   // diagnostic: staging only
  if (DIAG && dbg) st2 = wall_clock64();
  double e_lj = 0, e_tab = 0, vir = 0;
  [[maybe_unused]] double e_q = 0, v_q = 0;
  [[maybe_unused]] double tw[6] = {0, 0, 0, 0, 0, 0};
  for (int q0 = 0; q0 < nhome; q0 += NSL) {
    const int q = q0 + slice;
    R fx = 0, fy = 0, fz = 0;
    if (q0 > 0) { p = -1; if (q < nhome) locate(q); }
    if (p >= 0) {
      Vec4<R> xi;
      if constexpr (D3) { xi = lds_gather3d(sx, hslot); xi.w = (R)d3_types<R>(sx, CAP)[hslot]; } else xi = sx[hslot];
      const int pbase = (int)xi.w * ntypes;
      [[maybe_unused]] R kqi = 0; [[maybe_unused]] unsigned int crow = 0;
      if constexpr (COUL) { kqi = ca.k * sq[hslot]; crow = ca.mask[(int)xi.w]; }
      [[maybe_unused]] R lami = 1; [[maybe_unused]] unsigned int rrow = 0;
      if constexpr (RES) { lami = sq[hslot]; rrow = ra.mask[(int)xi.w]; }
      // Uniform-LJ fp32 path: (x, y) of one neighbour live in an aligned register pair (the 16-byte LDS read returns
      // x y z w in four consecutive VGPRs), so the differences, their squares and the force accumulation of the x and y
      // components are PACKED fp32 instructions on that pair -- no register shuffling as when the compiler pairs up two
      // neighbours (its SLP form of this loop spent 27.6 VALU instructions per neighbour, profiles/round3_pmc_sq_counters.txt)
      typedef float f32x2_ __attribute__((ext_vector_type(2)));
      typedef float f32x4_ __attribute__((ext_vector_type(4)));
      f32x2_ fxy = {0.f, 0.f};
      [[maybe_unused]] const f32x2_ xixy = {(float)xi.x, (float)xi.y};
      auto do_chunk = [&](const uint4 pk) {
        const unsigned int wds[4] = {pk.x, pk.y, pk.z, pk.w};
#ifndef CHEM_PK
#define CHEM_PK 1
#endif
        if constexpr (CHEM_PK && MODE == 2 && !ENERGY && sizeof(R) == 4) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            f32x4_ pj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {   // 4 LDS gathers in flight
              const unsigned int sl = (wds[2 * h + (u >> 1)] >> ((u & 1) * 16)) & 0xffff;
              pj[u] = *((const volatile __attribute__((address_space(3))) f32x4_*)sx + sl);
            }
#pragma unroll
            for (int u = 0; u < 4; u += 2) {      // two neighbours: distances per neighbour on its (x, y) pair, the LJ chain packed over the two
              const f32x2_ dxy0 = xixy - pj[u].xy, dxy1 = xixy - pj[u + 1].xy;
              const float dz0 = (float)xi.z - pj[u].z, dz1 = (float)xi.z - pj[u + 1].z;
              const f32x2_ sq0 = dxy0 * dxy0, sq1 = dxy1 * dxy1;
              const f32x2_ r2 = {__builtin_fmaf(dz0, dz0, sq0.x + sq0.y), __builtin_fmaf(dz1, dz1, sq1.x + sq1.y)};
              const f32x2_ r2i = {__builtin_amdgcn_rcpf(r2.x), __builtin_amdgcn_rcpf(r2.y)};
              const f32x2_ r6i = r2i * r2i * r2i;
              const f32x2_ lj1v = {(float)u_lj1, (float)u_lj1}, lj2v = {-(float)u_lj2, -(float)u_lj2};
              f32x2_ ff = r6i * __builtin_elementwise_fma(lj1v, r6i, lj2v) * r2i;
              ff.x = (r2.x <= (float)u_rc2) ? ff.x : 0.f;
              ff.y = (r2.y <= (float)u_rc2) ? ff.y : 0.f;
              const f32x2_ f0 = {ff.x, ff.x}, f1 = {ff.y, ff.y};
              fxy = __builtin_elementwise_fma(f0, dxy0, fxy);
              fxy = __builtin_elementwise_fma(f1, dxy1, fxy);
              fz = (R)__builtin_fmaf(ff.y, dz1, __builtin_fmaf(ff.x, dz0, (float)fz));
            }
          }
          return;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Vec4<R> xs[4];
          [[maybe_unused]] R qs[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {   // 4 LDS gathers in flight
            const unsigned int sl = (wds[2 * h + (u >> 1)] >> ((u & 1) * 16)) & 0xffff;
            if constexpr (D3) { xs[u] = lds_gather3d(sx, sl); if (MODE != 2 || ENERGY) xs[u].w = (R)d3_types<R>(sx, CAP)[sl]; }
            else xs[u] = lds_gather4<R>(sx, sl);
            if constexpr (COUL || RES) qs[u] = sq[sl];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const Vec4<R> xj = xs[u];
            const R dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            const R r2 = dx * dx + dy * dy + dz * dz;
            if (MODE == 2 && !ENERGY) {
              const R r2i = rcp_r(r2), r6i = r2i * r2i * r2i;
              R ff = r6i * (u_lj1 * r6i - u_lj2) * r2i;
              ff = (r2 <= u_rc2) ? ff : (R)0;
              fx += ff * dx; fy += ff * dy; fz += ff * dz;
            } else {
              const int pidx = pbase + (int)xj.w;
              [[maybe_unused]] R c2 = (R)0;
              if constexpr (CAPPED) c2 = sc2[(int)xi.w * kMaxTypes + (int)xj.w];
              if constexpr (TENSOR) {
                R tx = 0, ty = 0, tz = 0;
                if constexpr (RES) {
                  const int tj = (int)xj.w;
                  res_pair<R, ENERGY>([&](R& ax, R& ay, R& az, double& a1, double& a2, double& av) { pair_accum<R, ENERGY, LJONLY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, ax, ay, az, a1, a2, av, c2); },
                                      lami, qs[u], ((rrow >> tj) & 1u) != 0, sfm[(int)xi.w * kMaxTypes + tj], dx, dy, dz, tx, ty, tz, e_lj, e_tab, vir);
                } else
                pair_accum<R, ENERGY, LJONLY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, tx, ty, tz, e_lj, e_tab, vir, c2);
                if constexpr (COUL) coul_term<R, ENERGY>(kqi, qs[u], ((crow >> (int)xj.w) & 1u) != 0, ca.rc2, r2, dx, dy, dz, tx, ty, tz, e_q, v_q);
                fx += tx; fy += ty; fz += tz;
                tensor_add(tw, (double)dx, (double)dy, (double)dz, (double)tx, (double)ty, (double)tz);
              } else {
              if constexpr (RES) {
                const int tj = (int)xj.w;
                res_pair<R, ENERGY>([&](R& ax, R& ay, R& az, double& a1, double& a2, double& av) { pair_accum<R, ENERGY, LJONLY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, ax, ay, az, a1, a2, av, c2); },
                                    lami, qs[u], ((rrow >> tj) & 1u) != 0, sfm[(int)xi.w * kMaxTypes + tj], dx, dy, dz, fx, fy, fz, e_lj, e_tab, vir);
              } else
              pair_accum<R, ENERGY, LJONLY, CUBIC, CAPPED>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, fx, fy, fz, e_lj, e_tab, vir, c2);
              if constexpr (COUL) coul_term<R, ENERGY>(kqi, qs[u], ((crow >> (int)xj.w) & 1u) != 0, ca.rc2, r2, dx, dy, dz, fx, fy, fz, e_q, v_q);
              }
            }
          }
        }
      };
#pragma unroll
      for (int c = 0; c < NCH; ++c) if ((sub + c * TPP) * 8 < cnt) do_chunk(pkv[c]);
      // rows longer than the preloaded chunks (the rule with a list skin: ~52 entries = 6.5 chunks): the load of the chunk
      // after next is issued before a chunk is worked on, so that a lane waits for one L2 round trip per row, not per chunk
      {
        int c = sub + NCH * TPP;
        bool have = c * 8 < cnt;
        uint4 cur = make_uint4(0, 0, 0, 0);
#ifndef CHEM_NT_TAIL
#define CHEM_NT_TAIL 0
#endif
        if (have) cur = CHEM_NT_TAIL ? nt_load_u4(&reg[(size_t)c * nhome + qq]) : reg[(size_t)c * nhome + qq];
        while (have) {
          const int cn = c + TPP;
          const bool hn = cn * 8 < cnt;
          uint4 nx = make_uint4(0, 0, 0, 0);
          if (hn) nx = CHEM_NT_TAIL ? nt_load_u4(&reg[(size_t)cn * nhome + qq]) : reg[(size_t)cn * nhome + qq];
          do_chunk(cur);
          cur = nx; have = hn; c = cn;
        }
      }
      fx += (R)fxy.x; fy += (R)fxy.y;      // (packed x/y accumulators of the uniform-LJ fp32 path; zero otherwise)
      if (!COUL && !RES && !CAPPED && bslots && sub == 0) {
        // Inline harmonic bonds (FixedPairListHarmonic, gromacs_topology.py:949-961; reaction bonds reaction_setup.py:449-467):
        // the LDS slots of the bonded (= excluded) partners are recorded at every rebuild, the geometry comes from the staged
        // image (tile-local coordinates: 2.4e-7 in the fp32 build, exact in fp64) -- no bonded launch, no second pass over f4.
        // bond_mode 1: the list build removed the excluded pairs from the force list (decomposed path) -- add the bonds.
        // bond_mode 2: the list build IGNORED the exclusions (single domain: locating the partners inside the list phase cost
        //   196 us of a 709-us late-stage rebuild, profiles/round3_rebuild_ablation.txt; the rebuild's idle tail records the
        //   slots instead, dev_bond_slots_tile) -- the partners' pair term is in the sums above: take it out again, then add the bonds.  An excluded
        //   pair within the cutoff now was within the list radius at the build, i.e. it IS in the list if its type pair is active.
        const R m2K = (R)(-2.0 * bond_K), r0b = (R)bond_r0;              // (one parameter set: kernel arguments, no table)
        auto bond_quad = [&](const BondRec bq) {
          unsigned int bws[4];
          bond_rec_unpack(bq, bws);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (bws[k] == kBondRecNone) continue;
            const unsigned int sl = bws[k];
            Vec4<R> xj;
            if constexpr (D3) { xj = lds_gather3d(sx, sl); xj.w = (R)d3_types<R>(sx, CAP)[sl]; } else xj = sx[sl];
            const R dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            const R r2 = dx * dx + dy * dy + dz * dz;
            if (bond_mode >= 2) {
              if (MODE == 2 && !ENERGY) {
                if (r2 <= u_rc2 && ((bact.row[(int)xi.w & 15] >> ((int)xj.w & 15)) & 1u)) {
                  const R r2i = rcp_r(r2), r6i = r2i * r2i * r2i;
                  const R ffp = r6i * (u_lj1 * r6i - u_lj2) * r2i;
                  fx -= ffp * dx; fy -= ffp * dy; fz -= ffp * dz;
                }
              } else {
                R tx = 0, ty = 0, tz = 0; double te1 = 0, te2 = 0, tv = 0;
                const int pidx = pbase + (int)xj.w;
                pair_accum<R, ENERGY, LJONLY, CUBIC>(spc[pidx], pext, pidx, tab, r2, dx, dy, dz, tx, ty, tz, te1, te2, tv);
                fx -= tx; fy -= ty; fz -= tz; e_lj -= te1; e_tab -= te2; vir -= tv;
                if constexpr (TENSOR) tensor_add(tw, (double)dx, (double)dy, (double)dz, -(double)tx, -(double)ty, -(double)tz);
              }
            }
            if (!ENERGY) {
              const R r = sqrt_r(r2);
              const R ffb = m2K * (r - r0b) / r;                           // U = K (r - r0)^2
              fx += ffb * dx; fy += ffb * dy; fz += ffb * dz;
            }
          }
        };
        bond_quad(bwv);
        if (bond_rec_full(bwv)) bond_quad(bslots.rec1[p]);   // five to eight bonds: the second word (rare)
      }
    }
    if (TPP > 1) {
#pragma unroll
      for (int o = TPP / 2; o > 0; o >>= 1) { fx += __shfl_xor(fx, o); fy += __shfl_xor(fy, o); fz += __shfl_xor(fz, o); }
    }
    if (p >= 0 && sub == 0) f4[p] = mk4<R>(fx, fy, fz, (R)0);
  }
  if (DIAG && dbg && threadIdx.x == 0) {   // diagnostic instantiation only: per-block phase stamps (100 MHz wall clock)
    st3 = wall_clock64();
    long long* o = dbg + 6 * (size_t)blockIdx.x;
    o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3; o[4] = 0; o[5] = tile;
  }
  if (ENERGY) {
    __shared__ double red[COUL ? 5 : 3][BS / 64];
    for (int o = 32; o > 0; o >>= 1) { e_lj += __shfl_xor(e_lj, o); e_tab += __shfl_xor(e_tab, o); vir += __shfl_xor(vir, o); }
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = e_lj; red[1][threadIdx.x >> 6] = e_tab; red[2][threadIdx.x >> 6] = vir; }
    if constexpr (COUL) {
      for (int o = 32; o > 0; o >>= 1) { e_q += __shfl_xor(e_q, o); v_q += __shfl_xor(v_q, o); }
      if (lane_id() == 0) { red[3][threadIdx.x >> 6] = e_q; red[4][threadIdx.x >> 6] = v_q; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0, b = 0, c = 0;
      for (int k = 0; k < BS / 64; ++k) { a += red[0][k]; b += red[1][k]; c += red[2][k]; }
      eout[3 * blockIdx.x + 0] = 0.5 * a; eout[3 * blockIdx.x + 1] = 0.5 * b; eout[3 * blockIdx.x + 2] = 0.5 * c;
      if constexpr (COUL) {
        double d = 0, e = 0;
        for (int k = 0; k < BS / 64; ++k) { d += red[3][k]; e += red[4][k]; }
        ca.eout[2 * blockIdx.x + 0] = 0.5 * d; ca.eout[2 * blockIdx.x + 1] = 0.5 * e;
      }
    }
  }
  if constexpr (TENSOR) tensor_block_out<BS / 64>(tw, 0.5, tout + 6 * (size_t)blockIdx.x);
}

template <typename R, int TPP, bool ENERGY, int BS, int MODE, bool DIAG = false>
__global__ __launch_bounds__(BS, sizeof(R) == 8 ? 4 : (BS == 1024 ? 2048 : 1536) / 256) void k_pair_tiles(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, UniLJ uni, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, int ablate, long long* __restrict__ dbg, TileSub sub_,
                                                   DecideArgs da = DecideArgs{}, BondRecs bslots = BondRecs{},
                                                   double bond_K = 0.0, double bond_r0 = 0.0, int bond_mode = 0, ActMask bact = ActMask{}) {
  static_assert(MODE < 4, "MODE 4 is k_pair_tiles_q, MODE 5 k_pair_tiles_res, MODE 6 k_pair_tiles_cap, MODE 7 k_pair_tiles_rescap");
  pair_tiles_body<R, TPP, ENERGY, BS, MODE, DIAG>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, uni, eout, half_skin, ctl, guard, ablate, dbg,
                                                  sub_, da, bslots, bond_K, bond_r0, bond_mode, bact, CoulArgs<R>{}, ResArgs<R>{});
}
// MODE 4: one lane per particle, 512 threads; no inline bonds
template <typename R, bool ENERGY>
__global__ __launch_bounds__(512, sizeof(R) == 8 ? 4 : 1536 / 256) void k_pair_tiles_q(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, TileSub sub_, DecideArgs da, CoulArgs<R> ca) {
  pair_tiles_body<R, 1, ENERGY, 512, 4, false>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, UniLJ{}, eout, half_skin, ctl, guard, 0, nullptr,
                                               sub_, da, BondRecs{}, 0.0, 0.0, 0, ActMask{}, ca, ResArgs<R>{});
}
// MODE 5: one lane per particle, 512 threads; no inline bonds
template <typename R, bool ENERGY>
__global__ __launch_bounds__(512, sizeof(R) == 8 ? 4 : 1536 / 256) void k_pair_tiles_res(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, TileSub sub_, DecideArgs da, ResArgs<R> ra) {
  pair_tiles_body<R, 1, ENERGY, 512, 5, false>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, UniLJ{}, eout, half_skin, ctl, guard, 0, nullptr,
                                               sub_, da, BondRecs{}, 0.0, 0.0, 0, ActMask{}, CoulArgs<R>{}, ra);
}
// MODE 6: one lane per particle, 512 threads; no inline bonds
template <typename R, bool ENERGY>
__global__ __launch_bounds__(512, sizeof(R) == 8 ? 4 : 1536 / 256) void k_pair_tiles_cap(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, TileSub sub_, DecideArgs da, CapArgs<R> cp) {
  pair_tiles_body<R, 1, ENERGY, 512, 6, false>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, UniLJ{}, eout, half_skin, ctl, guard, 0, nullptr,
                                               sub_, da, BondRecs{}, 0.0, 0.0, 0, ActMask{}, CoulArgs<R>{}, ResArgs<R>{}, cp);
}
// MODE 7: one lane per particle, 512 threads; no inline bonds
template <typename R, bool ENERGY>
__global__ __launch_bounds__(512, sizeof(R) == 8 ? 4 : 1536 / 256) void k_pair_tiles_rescap(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                   const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                   const int* __restrict__ nnh, int S16,
                                                   const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                   int ntypes, const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                   double half_skin, DevCtl* ctl, int guard, TileSub sub_, DecideArgs da, ResArgs<R> ra, CapArgs<R> cp) {
  pair_tiles_body<R, 1, ENERGY, 512, 7, false>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, UniLJ{}, eout, half_skin, ctl, guard, 0, nullptr,
                                               sub_, da, BondRecs{}, 0.0, 0.0, 0, ActMask{}, CoulArgs<R>{}, ra, cp);
}

// =======================================================================================
// K4-K6  bonded forces (FixedPairList/TripleList/QuadrupleList interactions,
//     gromacs_topology.py:949-961,1086-1096,1206-1224).  Per-particle CSR (by tag): every
//     member of a tuple evaluates the term and keeps its own force -> no atomics,
//     deterministic.  Geometry in fp64 in both precision modes.
// =======================================================================================

__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot3(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross3(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// a b - c d with the rounding error of c d recovered by fused multiply-adds (Kahan): a cross product of nearly parallel vectors
// keeps its relative accuracy (bonded_term EXACT)
__device__ __forceinline__ double diff_of_products(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  const double w = c * d;
  const double e = __builtin_fma(-c, d, w), f = __builtin_fma(a, b, -w);
  return f + e;
}
__device__ __forceinline__ D3 cross3_exact(D3 a, D3 b) {
  return {diff_of_products(a.y, b.z, a.z, b.y), diff_of_products(a.z, b.x, a.x, b.z), diff_of_products(a.x, b.y, a.y, b.x)};
}
struct BoxD { double L[3], invL[3]; double qs[3], qh[3]; };   // qs, qh: fixed-point decoding of the fp32 build's positions (Box<R>)
__device__ __forceinline__ D3 minimgD(const BoxD& b, D3 d) {
  return {d.x - b.L[0] * rint(d.x * b.invL[0]), d.y - b.L[1] * rint(d.y * b.invL[1]), d.z - b.L[2] * rint(d.z * b.invL[2])};
}
// |d|^2 exactly as the CPU oracle rounds it: three products, two sums, NO fused multiply-add.  (__dmul_rn / __dadd_rn are plain
// operators in the HIP headers and -ffp-contract=fast fused them; invisible as long as the test positions were fp32 values,
// whose products are exact in fp64.)
__device__ __forceinline__ double dist2_unfused(const D3& d) {
#pragma clang fp contract(off)
  const double xx = d.x * d.x, yy = d.y * d.y, zz = d.z * d.z;
  return (xx + yy) + zz;
}
template <typename R> __device__ __forceinline__ D3 posD(const Vec4<R>& v, const BoxD& b) { return pos_real(v, b.qs, b.qh); }   // exact in both builds

// bond tables (chem_table_create[_interp]): rows = (e, f) pairs of all tables back to back,
// info[h] = (first row, +-rows of the grid, r0, 1/dr); the sign of the second entry is the interpolation kind:
//   > 0  linear: one pair per grid row;
//   < 0  piecewise cubic (Akima or natural spline, fitted on the host: chem_tab_host.hpp): four pairs per interval,
//        (e c0, f c0) .. (e c3, f c3), rows - 1 intervals.
// (the kind as a field of its own cost k_bonded_work a register)
struct BTab { const double2* rows; const double4* info; };
// table h at x (a distance, or an angle in radians): u = e(x), fv = f(x); beyond the grid the end rows' values hold
__device__ __forceinline__ void btab_lookup(const BTab& bt, const int h, const double x, double& u, double& fv) {
  const double4 ti = bt.info[h];
  const double2* row = bt.rows + (size_t)ti.x;
  const int nr = (int)ti.y, nrow = nr < 0 ? -nr : nr;
  const double t = (x - ti.z) * ti.w;
  if (nr > 0) {
    if (t <= 0) { u = row[0].x; fv = row[0].y; }
    else if (t >= (double)(nrow - 1)) { u = row[nrow - 1].x; fv = row[nrow - 1].y; }
    else { const int k = (int)t; const double w = t - (double)k; const double2 a = row[k], b = row[k + 1]; u = a.x + w * (b.x - a.x); fv = a.y + w * (b.y - a.y); }
  } else {
    const double tc = t > 0 ? (t < (double)(nrow - 1) ? t : (double)(nrow - 1)) : 0.0;      // (a NaN ends at 0)
    int k = (int)tc;
    if (k > nrow - 2) k = nrow - 2;
    const double w = tc - (double)k;
    const double2 c0 = row[4 * k], c1 = row[4 * k + 1], c2 = row[4 * k + 2], c3 = row[4 * k + 3];
    u = c0.x + w * (c1.x + w * (c2.x + w * c3.x));
    fv = c0.y + w * (c1.y + w * (c2.y + w * c3.y));
  }
}

// one bonded term seen from member `me` of the tuple (j0..j3 = particle indices of the tuple in order)
// BONDS_ONLY: the caller guarantees arity 2 and an analytic kind (harmonic, FENE, FENE+LJ, LJ pair) -- the angle, dihedral
// and table code is not compiled in, which is what brings the per-step kernel from 209 to a few dozen registers
// HYB: the term (force and energy) is scaled by `lam` (hybrid lists); a triple or quadruple whose lam is exactly 0 is left out
// (its full term need not be finite); not compiled into the other instantiations
// COUL: the 1-4 Coulomb kind (CHEM_POT_COULOMB_BOND) with the two members' charges q0, q1; not compiled into the others either
// EXACT (k_bonded_virial_tensor alone): the bending term in a form that keeps its digits next to a straight or folded angle
// ("Conditioning of the bending term"): r1 x r2 by compensated products, theta and sin(theta) from atan2(|r1 x r2|,
// r1 . r2), the two forces as (r1 x r2) x r1 and r2 x (r1 x r2) instead of differences of nearly equal vectors times dU / sin.
// The same law; at 1e-5 off folded with theta0 = pi the plain form is off by 1e-10 of the list's d (x) F, which an observable
// compared at that level cannot afford.  Not compiled into the other instantiations.
template <typename R, bool ENERGY, bool BONDS_ONLY = false, bool HYB = false, bool COUL = false, bool EXACT = false>
__device__ __forceinline__ void bonded_term(const BondedParam& bp, const int me, const int j0, const int j1, const int j2, const int j3,
                                            const Vec4<R>* __restrict__ x4, const BoxD& box, D3& f, double* __restrict__ elist, DevCtl* ctl, const BTab& bt,
                                            const double lam = 1.0, const double q0 = 0.0, const double q1 = 0.0) {
    const double* p = bp.p;
    double u = 0;
    if (BONDS_ONLY || bp.arity == 2) {
      // tuple (t0,t1); r_ij = x_t0 - x_t1
      if ((j0 | j1) < 0) { ctl->bonded_missing = 1; return; }
      const D3 x0 = posD<R>(x4[j0], box), x1 = posD<R>(x4[j1], box);
      const D3 d = minimgD(box, x0 - x1);
      const double r = sqrt(dot3(d, d));
      double ff = 0;
      if (bp.kind == CHEM_POT_HARMONIC) { const double dr = r - p[1]; u = p[0] * dr * dr; ff = -2.0 * p[0] * dr / r; }
      else if (bp.kind == CHEM_POT_FENE) { const double dr = r - p[1], q = dr / p[2], den = 1.0 - q * q; u = -0.5 * p[0] * p[2] * p[2] * log(den); ff = -p[0] * dr / den / r; }
      else if (bp.kind == CHEM_POT_FENE_LJ) {   // FENELennardJones(K, r0, rMax, sigma, epsilon)
        const double dr = r - p[1], q = dr / p[2], den = 1.0 - q * q;
        const double s2 = p[3] * p[3] / (r * r), s6 = s2 * s2 * s2;
        u = -0.5 * p[0] * p[2] * p[2] * log(den) + 4.0 * p[4] * (s6 * s6 - s6);
        ff = -p[0] * dr / den / r + 24.0 * p[4] * (2.0 * s6 * s6 - s6) / (r * r);
      }
      else if (bp.kind == CHEM_POT_LJ_BOND) {   // FixedPairListLennardJones(epsilon, sigma, cutoff): 1-4 pairs
        if (r <= p[2]) {
          const double s2 = p[1] * p[1] / (r * r), s6 = s2 * s2 * s2;
          // energy shifted to zero at the cutoff: espressopp's LennardJones defaults to shift = 'auto' (SURVEY App. C), also on the 1-4 lists
          const double c2 = p[1] * p[1] / (p[2] * p[2]), c6 = p[2] < 1e29 ? c2 * c2 * c2 : 0.0;
          u = 4.0 * p[0] * ((s6 * s6 - s6) - (c6 * c6 - c6));
          ff = 24.0 * p[0] * (2.0 * s6 * s6 - s6) / (r * r);
        }
      }
      else if (COUL && bp.kind == CHEM_POT_COULOMB_BOND) {   // FixedPairListCoulombTruncated(prefactor, cutoff): 1-4 pairs, no shift
        if (r <= p[1]) { u = p[0] * (q0 * q1) / r; ff = u / (r * r); }
      }
      else if (!BONDS_ONLY && bp.kind == CHEM_POT_TABULATED) {   // Tabulated: e(r), f(r) from table p[0]
        double fv;
        btab_lookup(bt, (int)p[0], r, u, fv);
        ff = fv / r;
      }
      if (HYB) { ff *= lam; u *= lam; }
      const double sgn = me == 0 ? 1.0 : -1.0;
      f = f + (sgn * ff) * d;
    } else if (BONDS_ONLY) {
    } else if (bp.arity == 3) {
      if ((j0 | j1 | j2) < 0) { ctl->bonded_missing = 1; return; }
      if (HYB && lam == 0.0) return;
      const D3 x0 = posD<R>(x4[j0], box), x1 = posD<R>(x4[j1], box), x2 = posD<R>(x4[j2], box);
      const D3 r1 = minimgD(box, x0 - x1), r2 = minimgD(box, x2 - x1);
      const double n1 = sqrt(dot3(r1, r1)), n2 = sqrt(dot3(r2, r2));
      double c = dot3(r1, r2) / (n1 * n2);
      c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
      double th = acos(c);
      double s = sqrt(1.0 - c * c);
      [[maybe_unused]] D3 x12 = {0, 0, 0}; [[maybe_unused]] double sn = 0;
      if constexpr (EXACT) { x12 = cross3_exact(r1, r2); sn = sqrt(dot3(x12, x12)); th = atan2(sn, dot3(r1, r2)); s = sn / (n1 * n2); }
      [[maybe_unused]] const bool perp = EXACT && s >= 1e-9;
      if (s < 1e-9) s = 1e-9;
      double dU = 0;
      if (bp.kind == CHEM_POT_ANG_HARMONIC) { const double d = th - p[1]; u = p[0] * d * d; dU = 2.0 * p[0] * d; }
      else if (bp.kind == CHEM_POT_ANG_COSINE) { u = p[0] * (1.0 + cos(th - p[1])); dU = -p[0] * sin(th - p[1]); }
      else if (bp.kind == CHEM_POT_ANG_TABULATED) {   // TabulatedAngular: U(theta), -dU/dtheta on a uniform grid in radians
        double fv;
        btab_lookup(bt, (int)p[0], th, u, fv);
        dU = -fv;
      }
      if (HYB) { dU *= lam; u *= lam; }
      const double a = dU / s;
      D3 fi = a * ((1.0 / (n1 * n2)) * r2 - (c / (n1 * n1)) * r1);
      D3 fk = a * ((1.0 / (n1 * n2)) * r1 - (c / (n2 * n2)) * r2);
      // EXACT: the same two vectors without the difference of nearly equal ones: n1^2 r2 - (r1 . r2) r1 = (r1 x r2) x r1
      if constexpr (EXACT) if (perp) { fi = (dU / (sn * n1 * n1)) * cross3(x12, r1); fk = (dU / (sn * n2 * n2)) * cross3(r2, x12); }
      if (me == 0) f = f + fi; else if (me == 2) f = f + fk; else f = f - (fi + fk);
    } else {
      if ((j0 | j1 | j2 | j3) < 0) { ctl->bonded_missing = 1; return; }
      if (HYB && lam == 0.0) return;
      const D3 x0 = posD<R>(x4[j0], box), x1 = posD<R>(x4[j1], box), x2 = posD<R>(x4[j2], box), x3 = posD<R>(x4[j3], box);
      const D3 b1 = minimgD(box, x1 - x0), b2 = minimgD(box, x2 - x1), b3 = minimgD(box, x3 - x2);
      const D3 m = cross3(b1, b2), nn = cross3(b2, b3);
      const double m2 = dot3(m, m), n2 = dot3(nn, nn), lb2 = dot3(b2, b2), lb = sqrt(lb2);
      if (m2 < 1e-30 || n2 < 1e-30) return;
      const double phi = atan2(lb * dot3(b1, nn), dot3(m, nn));
      double dU = 0;
      if (bp.kind == CHEM_POT_DIH_NCOS) { u = p[0] * (1.0 + cos(p[2] * phi - p[1])); dU = -p[0] * p[2] * sin(p[2] * phi - p[1]); }
      else if (bp.kind == CHEM_POT_DIH_RB) {
        const double psi = phi - M_PI, cp = cos(psi), sp = sin(psi);
        double pw = 1.0, dsum = 0;
        for (int k = 0; k < 6; ++k) { u += p[k] * pw; if (k < 5) dsum += (k + 1) * p[k + 1] * pw; pw *= cp; }
        dU = -sp * dsum;
      }
      else if (bp.kind == CHEM_POT_DIH_HARMONIC) {   // DihedralHarmonic(K, phi0): U = K/2 (phi - phi0)^2, difference wrapped
        double d = phi - p[1];
        d -= 2.0 * M_PI * rint(d / (2.0 * M_PI));
        u = 0.5 * p[0] * d * d; dU = p[0] * d;
      }
      else if (bp.kind == CHEM_POT_DIH_TABULATED) {   // TabulatedDihedral: U(phi), -dU/dphi on a uniform grid over [-pi, pi]
        double fv;
        btab_lookup(bt, (int)p[0], phi, u, fv);
        dU = -fv;
      }
      if (HYB) { dU *= lam; u *= lam; }
      const D3 g1 = (-lb / m2) * m, g4 = (lb / n2) * nn;
      const double s12 = dot3(b1, b2) / lb2, s32 = dot3(b3, b2) / lb2;
      D3 g;
      if (me == 0) g = g1;
      else if (me == 3) g = g4;
      else if (me == 1) g = (-1.0 - s12) * g1 + s32 * g4;
      else g = (-1.0 - s32) * g4 + s12 * g1;
      f = f - dU * g;
    }
    if (ENERGY && me == 0) *elist += u;      // (the caller's own word: the entry's energy, summed per list by k_list_sums)
}

// The entry points of the bonded forces.  Two launch shapes -- one thread per particle walking its rows of the per-tag CSR
// (k_bonded*: the launch without a work list, and observe()), one thread per owner of the work list (k_bonded_work*: every
// step) -- and one body each, bonded_particle_body and bonded_work_body, which hold the entry walk.  HYB compiles in the lambda
// of a hybrid entry (hybrid_lambda: 1 for entries of lists that are not hybrid; a pair keeps ~birth in its own t2, a triple
// or quadruple in t2 of its second entry), COUL the two charges of a 1-4 Coulomb
// entry (CHEM_POT_COULOMB_BOND; type R, the product is formed in fp64) and with them the matching code of bonded_term; `hy`,
// `qtag` and the work list's `tag` are read under those flags only.  A context with both kinds of list runs the COUL family,
// which carries the lambda code along, so there is no fourth.  The families stay separate kernels, chosen on the host
// (bonded_kind, chem_launch_host.hpp), and not one kernel with flags: the plain kernels run every step of every workload
// and keep the registers and the argument list they were measured with.
template <typename R, bool ENERGY, bool HYB, bool COUL>
__device__ __forceinline__ void bonded_particle_body(int i0, int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                     const int* __restrict__ tag, const int* __restrict__ rtag,
                                                     const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                     const BondedParam* __restrict__ bpar, const BoxD& box, double* __restrict__ elist, DevCtl* ctl, const BTab& bt,
                                                     [[maybe_unused]] const HybridArgs& hy, [[maybe_unused]] const R* __restrict__ qtag) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= i0 + n) return;
  const int tg = tag[i];
  const int e0 = bstart[tg], e1 = bstart[tg + 1];
  if (e0 == e1) return;
  D3 f = {0, 0, 0};
  for (int e = e0; e < e1; ++e) {
    const BondedEntry be = bent[e];
    const int slot = bonded_slot(be.meta), me = bonded_member(be.meta);
    const BondedParam& bp = bpar[slot];
    const int ar = bp.arity;
    const int j0 = rtag[be.t0], j1 = rtag[be.t1], j2 = ar > 2 ? rtag[be.t2] : 0;
    int j3 = 0;
    // ENERGY: elist holds one word per entry of bent; member 0 leaves the entry's energy there (no atomics: the sums per list
    // are k_list_sums', in an order that depends on the entry table alone -- the same bits for the same state)
    [[maybe_unused]] const int es = e;
    [[maybe_unused]] double ue = 0.0;
    double* const ep = ENERGY ? &ue : elist;
    [[maybe_unused]] int tb = be.t2;      // HYB: the word that holds ~birth
    if constexpr (HYB) {
      if (ar == 4) { const BondedEntry b2 = bent[e + 1]; j3 = rtag[b2.t0]; tb = b2.t2; ++e; }
      else if (hybrid_wide_triple(bp)) { tb = bent[e + 1].t2; ++e; }
    } else {
      if (ar == 4) { j3 = rtag[bent[e + 1].t0]; ++e; }   // quadruples occupy two consecutive entries: (t0,t1,t2,meta),(t3,-,-,-)
    }
    if constexpr (COUL) {
      double q0 = 0, q1 = 0;
      if (bp.kind == CHEM_POT_COULOMB_BOND) { q0 = (double)qtag[be.t0]; q1 = (double)qtag[be.t1]; }
      bonded_term<R, ENERGY, false, true, true>(bp, me, j0, j1, j2, j3, x4, box, f, ep, ctl, bt, hybrid_lambda(hy, bp, slot, tb), q0, q1);
    } else if constexpr (HYB) {
      bonded_term<R, ENERGY, false, true>(bp, me, j0, j1, j2, j3, x4, box, f, ep, ctl, bt, hybrid_lambda(hy, bp, slot, tb));
    } else {
      bonded_term<R, ENERGY>(bp, me, j0, j1, j2, j3, x4, box, f, ep, ctl, bt);
    }
    if constexpr (ENERGY) { if (me == 0) elist[es] = ue; }
  }
  Vec4<R> fo = f4[i];
  fo.x += (R)f.x; fo.y += (R)f.y; fo.z += (R)f.z;
  f4[i] = fo;
}
template <typename R, bool ENERGY>
__global__ __launch_bounds__(256) void k_bonded(int i0, int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                const int* __restrict__ tag, const int* __restrict__ rtag,
                                                const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                const BondedParam* __restrict__ bpar, BoxD box, double* __restrict__ elist, DevCtl* ctl, BTab bt) {
  bonded_particle_body<R, ENERGY, false, false>(i0, n, x4, f4, tag, rtag, bstart, bent, bpar, box, elist, ctl, bt, HybridArgs{}, nullptr);
}
// at least one hybrid list in the context (CtxT::has_hybrid)
template <typename R, bool ENERGY>
__global__ __launch_bounds__(256) void k_bonded_hyb(int i0, int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                    const int* __restrict__ tag, const int* __restrict__ rtag,
                                                    const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                    const BondedParam* __restrict__ bpar, BoxD box, double* __restrict__ elist, DevCtl* ctl, BTab bt,
                                                    HybridArgs hy) {
  bonded_particle_body<R, ENERGY, true, false>(i0, n, x4, f4, tag, rtag, bstart, bent, bpar, box, elist, ctl, bt, hy, nullptr);
}
// at least one 1-4 Coulomb list in the context (CtxT::has_coul14): the two members of a Coulomb entry read their charges by tag
template <typename R, bool ENERGY>
__global__ __launch_bounds__(256) void k_bonded_q(int i0, int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                  const int* __restrict__ tag, const int* __restrict__ rtag,
                                                  const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                  const BondedParam* __restrict__ bpar, BoxD box, double* __restrict__ elist, DevCtl* ctl, BTab bt,
                                                  HybridArgs hy, const R* __restrict__ qtag) {
  bonded_particle_body<R, ENERGY, true, true>(i0, n, x4, f4, tag, rtag, bstart, bent, bpar, box, elist, ctl, bt, hy, qtag);
}

// exclusive scan over the block (BS threads, BS/64 <= 16 waves); returns the exclusive prefix of v,
// *total = block sum.  Two barriers; safe to call back to back.
template <int BS>
__device__ __forceinline__ int block_scan_excl(int v, int* total) {
  __shared__ int ws[16];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  __syncthreads();
  if (lane == 63) ws[w] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < BS / 64; ++k) { if (k < w) off += ws[k]; tot += ws[k]; }
  *total = tot;
  return off + incl - v;
}

// ---- row order of ONE tile's force list (option row_order; the rule and its reasons: chem_roworder_host.hpp).  The sweep has
// written the tile's rows and counts into the workgroup's staging region (st16 / stcnt, the tile's own layout: chunk c of home
// i at (c nhome + i) 8); here the rows are ranked by (chunks, natural index) -- a counting sort: per wave-pass of 64 homes and
// class the ballot gives the count and every lane's place among its equals, an exclusive scan over (class, wave-pass) the
// rest -- and copied to their positions in nl16, with their count words (entries, home).  Entry for entry the rows of the sweep.  `wc`: LDS scratch
// of kRowClasses * (kRowStageMax / 64) words (the sweep's image: free behind the barrier).  P: rows per pass of the force kernel.
template <int BS>
__device__ __forceinline__ void dev_row_order(const int nhome, const int hbase, const int S16, const int P, const unsigned short* st16, int* stcnt,
                                              unsigned short* nl16, int* nnh, int* wc) {
  const int t = threadIdx.x, lane = lane_id();
  const int NC = S16 / 8 + 1, NWP = (nhome + 63) >> 6;      // classes (cnt <= S16), wave-passes
  __syncthreads();      // the sweep is over: its rows and counts are visible to the workgroup, its image is free
  for (int i0 = (t & ~63); i0 < nhome; i0 += BS) {      // (wave-uniform)
    const int i = i0 + lane;
    const int cnt = i < nhome ? row_word_count(stcnt[i]) : 0;
    const int k = i < nhome ? row_chunks(cnt) : -1;
    int pre = 0;
    for (int c = 0; c < NC; ++c) {
      const unsigned long long m = __ballot(k == c);
      if (k == c) pre = __popcll(m & lanemask_lt());
      if (lane == 0) wc[c * NWP + (i0 >> 6)] = __popcll(m);
    }
    if (i < nhome) stcnt[i] = row_word(cnt, pre);      // (own word: the place among the equals of the wave-pass takes the home's half)
  }
  __syncthreads();
  {
    const int nwc = NC * NWP;
    int carry = 0;
    for (int base = 0; base < nwc; base += BS) {
      const int k = base + t;
      const int v = k < nwc ? wc[k] : 0;
      int tot;
      const int ex = block_scan_excl<BS>(v, &tot);
      if (k < nwc) wc[k] = carry + ex;
      carry += tot;
    }
    __syncthreads();
  }
  uint4* const reg = reinterpret_cast<uint4*>(nl16 + (size_t)hbase * S16);
  for (int i = t; i < nhome; i += BS) {
    const int v = stcnt[i], cnt = row_word_count(v), k = row_chunks(cnt);
    const int pos = row_position(wc[k * NWP + (i >> 6)] + row_word_home(v), nhome, P);
    nnh[hbase + pos] = row_word(cnt, i);
    const uint4* src = reinterpret_cast<const uint4*>(st16) + i;
    // (one chunk at a time: four in flight cost the kernel 68 bytes of scratch per lane more, a real call 52)
    for (int c = 0; c < k; ++c) reg[(size_t)c * nhome + pos] = src[(size_t)c * nhome];
  }
}

// ---- bonded work list: rebuilt together with the Verlet list (the particle order only changes
// there).  bwork = compact list of the particles that own bonded entries (i, e0, e1), bj = the
// entries' partner tags already resolved to particle indices.  The per-step kernel runs over the
// owners only, with full waves (the fp64 term code is long: a wave with one bonded lane costs as
// much as a full one), and has two dependent loads in front of the arithmetic instead of five.
// one chunk of BS particles starting at ib (block-uniform; ends with a workgroup barrier)
template <int BS>
// over_excl != nullptr (inline bonds): only the owners with MORE than kBondSlots exclusions enter the work list -- the force kernel
// evaluates the bonds of everybody else from its staged image (excl_start rows: the same criterion the list build applies)
__device__ __forceinline__ void dev_bonded_prep_chunk(int ib, int iend, const int* tag, const int* rtag, const int* bstart, const BondedEntry* bent,
                                                      int4* bwork, int4* bj, DevCtl* ctl, const int* over_excl = nullptr) {
  __shared__ int s_base, s_ebase;
  {
    const int i = ib + threadIdx.x;
    int e0 = 0, e1 = 0;
    if (i < iend) {
      const int tg = tag[i]; e0 = bstart[tg]; e1 = bstart[tg + 1];
      if (over_excl && over_excl[tg + 1] - over_excl[tg] <= kBondSlots) e1 = e0;
    }
    const int has = e1 > e0 ? 1 : 0;
    int tot, etot;
    const int rank = block_scan_excl<BS>(has, &tot);       // one global atomic per block and pass, not per wave:
    const int erank = block_scan_excl<BS>(e1 - e0, &etot); // (same-address atomics cost ~12 ns each)
    if (threadIdx.x == 0) {
      const unsigned long long old = tot ? atomicAdd(&ctl->bw64, ((unsigned long long)etot << 32) | (unsigned long long)tot) : 0ull;
      s_base = (int)(old & 0xffffffffull); s_ebase = (int)(old >> 32);
    }
    __syncthreads();
    // the entries of an owner follow each other IN WORK-LIST ORDER (the per-tag CSR is in tag order, i.e. scattered for
    // neighbouring particles): the per-step kernel reads one coalesced 16-byte record per entry -- partner indices and
    // the parameter slot / own position -- and nothing else
    const int eo = s_ebase + erank;
    if (has) bwork[s_base + rank] = make_int4(i, eo, e1 - e0, 0);
    // (t2 < 0: the birth step of a hybrid pair, no tag -- handed on as it is)
    for (int e = e0; e < e1; ++e) { const BondedEntry be = bent[e]; bj[eo + (e - e0)] = make_int4(rtag[be.t0], rtag[be.t1], be.t2 < 0 ? be.t2 : rtag[be.t2], be.meta); }
    __syncthreads();
  }
}
template <int BS>
__device__ __forceinline__ void dev_bonded_prep(int i0, int n, const int* tag, const int* rtag, const int* bstart, const BondedEntry* bent,
                                                int4* bwork, int4* bj, DevCtl* ctl, const int* over_excl = nullptr) {
  for (int ib = i0 + blockIdx.x * BS; ib < i0 + n; ib += gridDim.x * BS)    // block-uniform bound (block scan inside)
    dev_bonded_prep_chunk<BS>(ib, i0 + n, tag, rtag, bstart, bent, bwork, bj, ctl, over_excl);
}

__global__ __launch_bounds__(256) void k_bonded_prep(int i0, int n, const int* __restrict__ tag, const int* __restrict__ rtag, const int* __restrict__ bstart,
                                                     const BondedEntry* __restrict__ bent, int4* __restrict__ bwork, int4* __restrict__ bj, DevCtl* ctl,
                                                     const int* __restrict__ over_excl) {
  dev_bonded_prep<256>(i0, n, tag, rtag, bstart, bent, bwork, bj, ctl, over_excl);
}

// one owner of the work list per thread (HYB, COUL: see bonded_particle_body).  jj.z of a hybrid pair, and of the second
// record of a hybrid triple or quadruple, is ~birth step, handed on by the work-list build.  The records carry particle indices, so a charge is qtag[tag[j]] -- ghosts included, as in
// CoulArgs -- and is read at every evaluation: nothing in a record can go stale when a charge changes between two list builds.
template <typename R, bool BONDS_ONLY, bool HYB, bool COUL>
__device__ __forceinline__ void bonded_work_body(const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4, const int4* __restrict__ bwork, const int4* __restrict__ bj,
                                                 const BondedParam* __restrict__ bpar, const BoxD& box, DevCtl* ctl, int guard, const BTab& bt,
                                                 [[maybe_unused]] const HybridArgs& hy, [[maybe_unused]] const R* __restrict__ qtag,
                                                 [[maybe_unused]] const int* __restrict__ tag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int)(ctl->bw64 & 0xffffffffull) || (guard && ctl->need_rebuild) || ctl->halt) return;
  const int4 wk = bwork[k];
  D3 f = {0, 0, 0};
  for (int e = wk.y; e < wk.y + wk.z; ++e) {
    const int4 jj = bj[e];
    const int slot = bonded_slot(jj.w), me = bonded_member(jj.w);
    const BondedParam& bp = bpar[slot];
    int j3 = 0;
    [[maybe_unused]] int tb = jj.z;      // HYB: the word that holds ~birth
    if constexpr (HYB && !BONDS_ONLY) {
      if (bp.arity == 4) { const int4 j2nd = bj[e + 1]; j3 = j2nd.x; tb = j2nd.z; ++e; }
      else if (hybrid_wide_triple(bp)) { tb = bj[e + 1].z; ++e; }
    } else {
      if (!BONDS_ONLY && bp.arity == 4) { j3 = bj[e + 1].x; ++e; }
    }
    const int j2 = (!BONDS_ONLY && bp.arity > 2) ? jj.z : 0;
    if constexpr (HYB || COUL) {
      const double lam = hybrid_lambda(hy, bp, slot, tb);
      if constexpr (COUL) {
        double q0 = 0, q1 = 0;
        if (bp.kind == CHEM_POT_COULOMB_BOND && (jj.x | jj.y) >= 0) { q0 = (double)qtag[tag[jj.x]]; q1 = (double)qtag[tag[jj.y]]; }   // (a missing partner: bonded_term reports it)
        bonded_term<R, false, BONDS_ONLY, true, true>(bp, me, jj.x, jj.y, j2, j3, x4, box, f, nullptr, ctl, bt, lam, q0, q1);
      } else {
        bonded_term<R, false, BONDS_ONLY, true>(bp, me, jj.x, jj.y, j2, j3, x4, box, f, nullptr, ctl, bt, lam);
      }
    } else {
      bonded_term<R, false, BONDS_ONLY>(bp, me, jj.x, jj.y, j2, j3, x4, box, f, nullptr, ctl, bt);
    }
  }
  Vec4<R> fo = f4[wk.x];
  fo.x += (R)f.x; fo.y += (R)f.y; fo.z += (R)f.z;
  f4[wk.x] = fo;
}
// (`bent` is not read: the records of bj hold all of an entry.  It stays in the launch signature.)
template <typename R, bool BONDS_ONLY = false>
__global__ __launch_bounds__(256) void k_bonded_work(const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4, const int4* __restrict__ bwork, const int4* __restrict__ bj,
                                                     const BondedEntry* __restrict__ bent, const BondedParam* __restrict__ bpar, BoxD box, DevCtl* ctl, int guard, BTab bt) {
  bonded_work_body<R, BONDS_ONLY, false, false>(x4, f4, bwork, bj, bpar, box, ctl, guard, bt, HybridArgs{}, nullptr, nullptr);
}
template <typename R, bool BONDS_ONLY = false>
__global__ __launch_bounds__(256) void k_bonded_work_hyb(const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4, const int4* __restrict__ bwork, const int4* __restrict__ bj,
                                                         const BondedEntry* __restrict__ bent, const BondedParam* __restrict__ bpar, BoxD box, DevCtl* ctl, int guard, BTab bt,
                                                         HybridArgs hy) {
  bonded_work_body<R, BONDS_ONLY, true, false>(x4, f4, bwork, bj, bpar, box, ctl, guard, bt, hy, nullptr, nullptr);
}
template <typename R, bool BONDS_ONLY = false>
__global__ __launch_bounds__(256) void k_bonded_work_q(const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4, const int4* __restrict__ bwork, const int4* __restrict__ bj,
                                                       const BondedEntry* __restrict__ bent, const BondedParam* __restrict__ bpar, BoxD box, DevCtl* ctl, int guard, BTab bt,
                                                       HybridArgs hy, const R* __restrict__ qtag, const int* __restrict__ tag) {
  bonded_work_body<R, BONDS_ONLY, true, true>(x4, f4, bwork, bj, bpar, box, ctl, guard, bt, hy, qtag, tag);
}

// =======================================================================================
// Fused rebuild: decision + binning + cell scan + placement + canonical sort + copy-back + tile
// descriptors + list build in ONE persistent launch with grid barriers.
// Why: on this part a dependent kernel-to-kernel hand-over costs ~4.6 us, and the separate chain is
// 9 launches that all early-exit on ~7 of 8 steps -- ~40 us of a 160 us step spent launching
// nothing.  Here the idle path is one launch whose workgroups each fold the step's displacement
// maxima themselves (identical inputs, identical arithmetic => identical decision, no barrier
// needed to agree) and exit.
// The grid is sized by the host to be fully co-resident (occupancy query x CU count, exclusive
// device); a barrier that is not released within ~1 s sets ctl->barrier_timeout and every
// workgroup leaves (the host reports a fatal error) instead of spinning forever.
// =======================================================================================
struct GridBar {
  unsigned int grp[8][32];     // arrivals per XCD group (128-byte spacing)
  unsigned int top[32];        // groups arrived
  unsigned int gen[32];        // generation (release flag)
  unsigned int tq[8][32];      // tile queue heads, one per XCD
  unsigned int prepq[32];      // head of the bonded-work-list chunk queue
  unsigned int bondq[32];      // head of the queue of tiles whose bonded partners' slots are to be recorded (bond pass)
  long long stamp[16];         // wall_clock64 of workgroup 0 at the phase boundaries of the last rebuild (diagnostics)
};

__device__ __forceinline__ bool grid_barrier(GridBar* gb, DevCtl* ctl) {
  __shared__ int ok_s;
  // Every wave waits until its own stores are acknowledged by the L2; ONE thread of the workgroup
  // then executes the device-scope release (L2 write-back, needed across XCDs) and, after the wait,
  // the acquire (L1/L2 invalidate).  Both act on the caches, not on the issuing wave, so one per
  // workgroup is enough -- fences from all 6144 waves made a barrier cost ~160 us.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    int ok = 1;
    const unsigned int g = blockIdx.x & 7u;
    const unsigned int ngrp = gridDim.x < 8u ? gridDim.x : 8u;
    const unsigned int gsize = (gridDim.x - g + 7u) >> 3;
    const unsigned int gen = __hip_atomic_load(&gb->gen[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (atomicAdd(&gb->grp[g][0], 1u) == gsize - 1u) {
      __hip_atomic_store(&gb->grp[g][0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (atomicAdd(&gb->top[0], 1u) == ngrp - 1u) {
        __hip_atomic_store(&gb->top[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&gb->gen[0], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    unsigned int spins = 0;
    while (__hip_atomic_load(&gb->gen[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > (1u << 20)) { ctl->barrier_timeout = 1; ok = 0; break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // drop stale lines before anyone reads what other XCDs wrote
    ok_s = ok;
  }
  __syncthreads();
  return ok_s != 0;
}

template <typename R> struct FusedArgs {
  int n, ncell, ntiles, CAP, S, has_excl, criterion, par, seg_shift, tseg_shift, nblk, want32, ntypes, ablate, coop;      // (coop: option coop_overflow, see dev_nlist_tile_f32)
  double half_skin; R rl2;
  long long istep;                     // step this launch belongs to (recorded in ctl->halt_step when the launch has to stop the run)
  double half_skin_ref; R rl2_rows;    // the workload's skin: reference rebuild count, radius of the int32 Verlet rows (rl2 / half_skin: list skin)
  Vec4<R> *x4, *v4, *x4o, *v4o, *x0;
  int *tag, *tago, *rtag; int4 *img4, *img4o;
  int *cell_cnt, *cell_of, *slot_of, *cell_start, *cell_loc, *btot, *perm, *tn, *tloc, *tbtot, *cell_sub, *cell_n, *bucket; int bcap;
  TileLDS<R>* desc; const int *excl_start, *excl_list;
  int* tile_ord;         // the same order as a list (inverse of tile_pos): the tile queues of the list phase hand out the large tiles first.
                         // Both arrays are double-buffered ([parity of the rebuild count][ntiles]): workgroups 0..7 rewrite the other
                         // half from THIS rebuild's home counts (gelation makes the tiles unequal), the next rebuild uses it
  int* tile_pos;         // where the descriptor of tile t goes: inside every XCD's range the full-size tiles first, the short edge
                         // tiles last, so that the one-shot force launch (workgroup v reads desc[xcd_remap(v)]) ends on short blocks
  unsigned short* nl16; int *nnh, *nlist, *nn;
  // row order (dev_row_order; stage16 == nullptr: off, the natural order): staging region of every workgroup, rows of
  // stage_cap homes and their count words; rows per pass of the force kernel
  unsigned short* stage16; int* stage_cnt; int stage_cap, row_P;
  unsigned long long* blockmax; DevCtl* ctl; GridBar* gb;
  const int* bstart; const BondedEntry* bent; int4 *bwork, *bj; int nbent;
  BondRecs bslots;       // inline bonds (rec0 non-null: the bonded partners' LDS slots are recorded, one BondRec per particle in each array)
  int bond_pass;         // 1: the list build ignores the exclusions (= bonds); workgroups that have run out of tiles record the partner
                         //    slots (dev_bond_slots_tile) and every force launch takes the partners' pair term out again (k_pair_tiles bond_mode 2);
                         //    2: as 1, but k_bond_slots behind this launch records the slots (option bond_slots_kernel);
                         //    0: the list build removes the excluded pairs and records their slots
  Box<R> box; ActMask act;
  long long* wgst;   // diagnostics (option debug_stamps=2): 8 wall-clock stamps per workgroup of the last rebuilding launch
  // accumulated criterion: the step's maxima as k_integrate folded them, both parities ([par] read, [par ^ 1] cleared for the next
  // step's integrate) -- 64 reads per workgroup where the block maxima are 1954 at a million particles; nullptr: blockmax
  unsigned long long* fold;
  IdleHint* hint; int gen;      // pinned host words the bookkeeping thread publishes (step, accumulated distance, displacement) to; may be nullptr
};

// segment offsets: s_off[k] = base + sum of tot[0..k), s_off[nseg] = grand total (nseg <= 1024)
template <int BS>
__device__ __forceinline__ void seg_offsets(const int* tot, int nseg, int* s_off) {
  int carry = 0;
  for (int base = 0; base < nseg; base += BS) {
    const int k = base + (int)threadIdx.x;
    const int v = k < nseg ? tot[k] : 0;
    int t;
    const int ex = block_scan_excl<BS>(v, &t);
    if (k < nseg) s_off[k] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) s_off[nseg] = carry;
  __syncthreads();
}

// block-parallel local scans: segment `seg` = 2^shift consecutive items; loc[] = exclusive prefix inside
// the segment, tot[seg] = segment sum.  zero != 0: the counts are cleared for the next rebuild.
template <int BS>
__device__ __forceinline__ void seg_scan(int* cnt, int nitem, int shift, int* loc, int* tot, bool zero, int* cnt_copy = nullptr) {
  const int per = 1 << shift, nseg = (nitem + per - 1) >> shift;
  for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
    const int lo = seg << shift, hi = min(nitem, lo + per);
    int carry = 0;
    for (int base = lo; base < hi; base += BS) {
      const int k = base + (int)threadIdx.x;
      int v = 0;
      if (k < hi) { v = cnt[k]; if (zero) cnt[k] = 0; if (cnt_copy) cnt_copy[k] = v; }
      int t;
      const int ex = block_scan_excl<BS>(v, &t);
      if (k < hi) loc[k] = carry + ex;
      carry += t;
    }
    if (threadIdx.x == 0) tot[seg] = carry;
  }
}

#ifndef CHEM_FUSED_WAVES
#define CHEM_FUSED_WAVES 4
#endif
// DIAG = true: diagnostic instantiation (option debug_stamps) with the per-workgroup phase stamps and the ablation switch of
// the list build, also used when the int32 Verlet rows are wanted (chem_get_verlet_pairs); the production instantiation carries none of it (their uniform branches in the peel loop cost 7 % of the
// launch: 386 -> 360 us)
template <typename R, int BS, bool DIAG = false>
__global__ __launch_bounds__(BS, CHEM_FUSED_WAVES) void k_rebuild_fused(const FusedArgs<R> a) {
  __shared__ TileLDS<R> T;
  __shared__ int s_off[1025];
  __shared__ unsigned long long s_m[BS / 64];
  __shared__ int s_tile;
  CHEM_DYN_LDS(R);
  const int t = threadIdx.x, b = blockIdx.x, NB = gridDim.x, lane = lane_id(), w = t >> 6;
  DevCtl* const ctl = a.ctl;

  if (ctl->halt) return;   // a previous launch of this run stopped it (set one launch ago at the earliest: every workgroup sees it)
  // ---- P0: decision, computed redundantly by every workgroup ----
  unsigned long long m = 0;
  if (a.fold) {
    m = fold_words_max(a.fold + a.par * kFoldSlots, kFoldSlots);
    if (b == 0 && t < kFoldSlots) a.fold[(a.par ^ 1) * kFoldSlots + t] = 0ull;
  } else {
    for (int k = t; k < a.nblk; k += BS) { const unsigned long long v = a.blockmax[k]; m = v > m ? v : m; }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(m, o); m = v > m ? v : m; }
    if (lane == 0) s_m[w] = m;
    __syncthreads();
    m = s_m[0];
#pragma unroll
    for (int k = 1; k < BS / 64; ++k) m = s_m[k] > m ? s_m[k] : m;
  }
  const double m2 = sizeof(R) == 4 ? bits_real_f(m) : bits_real_d(m);
  double acc = a.criterion ? sqrt(m2) : ctl->acc_pp[a.par] + sqrt(m2);
  const int forced = ctl->force_rebuild;
  const int need = (acc > a.half_skin) || forced;
  if (!need) {
    if (b == 0 && t == 0) { decide_book(ctl, a.par, a.criterion, m2, acc, 0, 0, a.half_skin_ref); publish_hint(a.hint, a.gen, a.istep, acc, sqrt(m2)); }
    return;
  }

  // ---- P1: bin.  Members go straight into the bucket row of their cell; per-segment particle totals are
  //          accumulated beside the cell counts, so that no scan phase is needed afterwards ----
  if (b == 0 && t == 0) a.gb->stamp[0] = wall_clock64();
  long long* const wst = (DIAG && a.wgst) ? a.wgst + 8 * (size_t)b : nullptr;
  const int ablate = DIAG ? a.ablate : 0;
#define WGST(K) do { if (wst && t == 0) wst[K] = wall_clock64(); } while (0)
  WGST(0);
  if (b == 0 && t < 8) a.gb->tq[t][0] = 0u;
  if (b == 0 && t == 8) { ctl->bw64 = 0ull; a.gb->prepq[0] = 0u; a.gb->bondq[0] = 0u; }
  { MigBuf<R> none{}; dev_bin<R>(0, a.n, a.x4, a.v4, a.tag, a.img4, a.box, a.cell_cnt, a.cell_of, a.slot_of, none, none, ctl, a.bucket, a.bcap, a.btot, a.seg_shift); }
  WGST(1);
  if (!grid_barrier(a.gb, ctl)) return; WGST(2); if (b == 0 && t == 0) { const long long st = wall_clock64(); a.gb->stamp[1] = st; a.gb->stamp[2] = st; a.gb->stamp[3] = st; }
  if (ctl->bucket_overflow) {
    // a cell is fuller than a bucket row: nothing but the counters has been touched yet -- clear them and leave; the
    // host redoes this rebuild with the unfused chain (force_rebuild stays set)
    for (int k = b * BS + t; k < a.ncell; k += NB * BS) a.cell_cnt[k] = 0;
    if (b == 0) for (int k = t; k < 1024; k += BS) a.btot[k] = 0;
    //  (a regular decision stays one for the reference rule when the host redoes it: DevCtl::force_rebuild)
    if (b == 0 && t == 0) { ctl->need_rebuild = 1; ctl->force_rebuild = forced ? forced : 2; ctl->halt_step = a.istep; ctl->halt_par = a.par; ctl->halt = 1; if (a.hint) { volatile IdleHint* h = a.hint; h->halted = a.gen; } }
    return;
  }
  // every workgroup has taken its decision: the control block may change now
  if (b == 0 && t == 0) {
    ctl->force_rebuild = 0;
    decide_book(ctl, a.par, a.criterion, m2, acc, 1, forced, a.half_skin_ref);
    publish_hint(a.hint, a.gen, a.istep, 0.0, sqrt(m2));
  }

  // ---- P4: cell_start, canonical order inside every cell + gather + tag -> index map; home count of every tile ----
  {
    const int nseg = (a.ncell + (1 << a.seg_shift) - 1) >> a.seg_shift;
    seg_offsets<BS>(a.btot, nseg, s_off);
    if (b == 0 && t == 0) a.cell_start[a.ncell] = s_off[nseg];
    dev_sort_gather_bucket<R>(a.ncell, a.cell_cnt, s_off, a.seg_shift, a.bucket, a.bcap, a.cell_start, a.x4, a.v4, a.tag, a.img4,
                              a.x4o, a.v4o, a.tago, a.img4o, a.rtag, a.box, a.cell_sub);
    const int nx = a.box.nc[0], ny = a.box.nc[1], nz = a.box.nc[2];
    const int ntx = tile_ntx(nx, a.box.xs_nb, a.box.xs_w), nty = (ny + HY - 1) / HY;
    for (int tile = b * BS + t; tile < a.ntiles; tile += NB * BS) {
      const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
      int cx0, hx;
      tile_xrange(tx, nx, a.box.xs_nb, a.box.xs_w, cx0, hx);
      const int cy0 = ty * HY, cz0 = tz * HZ;
      const int hy = min(HY, ny - cy0), hz = min(HZ, nz - cz0);
      int nh = 0;
      for (int hzi = 0; hzi < hz; ++hzi) for (int hyi = 0; hyi < hy; ++hyi) {
        const int c0 = ((cz0 + hzi) * ny + (cy0 + hyi)) * nx + cx0;
        for (int k = 0; k < hx; ++k) nh += a.cell_cnt[c0 + k];
      }
      a.tn[tile] = nh;
    }
  }
  WGST(3);
  if (!grid_barrier(a.gb, ctl)) return; WGST(4); if (b == 0 && t == 0) { const long long st = wall_clock64(); a.gb->stamp[4] = st; a.gb->stamp[5] = st; }

  // ---- P6: tile descriptors + list build.  Tiles are handed out dynamically, each XCD first drains its own contiguous
  //          range of tiles (L2 locality, see xcd_remap) and then helps the others.  The counts of this rebuild are
  //          cleared for the next one; the sorted arrays (x4o/v4o/tago/img4o) are read in place and copied back into
  //          the live arrays by workgroups that have run out of tiles ----
  {
    for (int k = b * BS + t; k < a.ncell; k += NB * BS) a.cell_cnt[k] = 0;
    if (b == 0) for (int k = t; k < 1024; k += BS) a.btot[k] = 0;
    // base of every tile's region in the transposed list = exclusive prefix of the home counts: segment totals of
    // 2^tseg_shift tiles are summed by every workgroup for itself (a few KB of reads), the rest at claim time
    const int tper = 1 << a.tseg_shift, ntseg = (a.ntiles + tper - 1) >> a.tseg_shift;
    {
      int carry = 0;
      for (int base = 0; base < ntseg; base += BS) {
        const int k = base + t;
        int v = 0;
        if (k < ntseg) for (int j = k << a.tseg_shift; j < min(a.ntiles, (k + 1) << a.tseg_shift); ++j) v += a.tn[j];
        int tot;
        const int ex = block_scan_excl<BS>(v, &tot);
        if (k < ntseg) s_off[k] = carry + ex;
        carry += tot;
      }
      __syncthreads();
    }
    const int q = a.ntiles >> 3, r = a.ntiles & 7, myx = b & 7;
    const int lpar = a.tile_ord ? (ctl->rebuild_count & 1) : 0;      // (incremented behind the first barrier: the same for everybody here)
    const int* const ord_r = a.tile_ord ? a.tile_ord + (size_t)lpar * a.ntiles : nullptr;
    const int* const pos_r = a.tile_pos ? a.tile_pos + (size_t)lpar * a.ntiles : nullptr;
    int ndone = 0;
    WGST(5);
    // thread 0 claims a tile: own XCD's queue first, then the others'
    auto claim = [&]() {
      int tile = -1;
      for (int d = 0; d < 8 && tile < 0; ++d) {
        const int x = (myx + d) & 7;
        const int cntx = q + (x < r ? 1 : 0);
        if (__hip_atomic_load(&a.gb->tq[x][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned int)cntx) continue;
        const int k = (int)atomicAdd(&a.gb->tq[x][0], 1u);
        if (k < cntx) { tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k; if (ord_r) tile = ord_r[tile]; }
      }
      return tile;
    };
    for (;;) {
      __syncthreads();
      if (t == 0) s_tile = claim();    // (claiming ahead of time, beside the previous tile's work, hides this round trip but
      __syncthreads();                 //  unbalances the tail of the phase: measured 307 -> 367 us)
      const int tile = s_tile;
      if (tile < 0) break;
      ++ndone;
      // base of the tile's list region = prefix of its segment + the home counts of the tiles in front of it inside the
      // segment: loaded here by the last wave, reduced after the tables (their latency overlaps)
      int hb_part = 0;
      if (w == BS / 64 - 1) {
        for (int j = ((tile >> a.tseg_shift) << a.tseg_shift) + lane; j < tile; j += 64) hb_part += a.tn[j];
      }
      const bool f32list = sizeof(R) == 4 || !(DIAG && a.want32);   // fp64: the exact list build only where the int32 rows are wanted
      if (f32list) list_stage_clear<BS>(chem_dyn_lds, list_lds_layout(a.CAP, a.ntypes), a.ntypes);   // (tile_tables synchronises)
      tile_tables<R>(T, a.CAP, tile, a.cell_start, a.box, ctl, a.cell_sub);      // ends with a workgroup barrier
      if (w == BS / 64 - 1) {
        for (int o = 32; o > 0; o >>= 1) hb_part += __shfl_xor(hb_part, o);
        if (lane == 0) T.geom[5] = s_off[tile >> a.tseg_shift] + hb_part;
      }
      __syncthreads();
      {   // the descriptor every force launch until the next rebuild reads
        const int* src = reinterpret_cast<const int*>(&T);
        int* dst = reinterpret_cast<int*>(&a.desc[pos_r ? pos_r[tile] : tile]);
        for (int k = t; k < (int)(sizeof(TileLDS<R>) / 4); k += BS) dst[k] = src[k];
      }
      const bool ordered = a.stage16 && T.geom[4] <= a.stage_cap && !(f32list && ablate == 1);
      const int sbase = ordered ? b * a.stage_cap : -1;      // row base of this workgroup's staging region
      if (f32list) {
        const ListLDS L = list_lds_layout(a.CAP, a.ntypes);
        list_stage_f32<R, BS>(T, chem_dyn_lds, L, a.CAP, a.x4o, a.act, a.ntypes);
        __syncthreads();
        if (ablate == 1) { for (int q = t; q < T.geom[4]; q += BS) a.nnh[T.geom[5] + q] = row_word(0, q); }
        else
        dev_nlist_tile_f32<R, BS>(T, chem_dyn_lds, L, a.tago, (float)a.rl2, a.excl_start, a.excl_list, a.bond_pass ? 0 : a.has_excl, ordered ? a.stage16 : a.nl16, a.S,
                               ordered ? a.stage_cnt : a.nnh, (DIAG && a.want32) ? a.nlist : (int*)nullptr, a.S, a.nn, ctl, &a.box, a.rtag, a.x4o, ablate, (float)a.rl2_rows,
                               a.bond_pass ? BondRecs{} : a.bslots, nullptr, 0, 0x7fffffff, a.coop, sbase);
      } else {
        tile_fill<R, BS, true>(T, sx, a.CAP, a.x4o, 1);
        __syncthreads();
        dev_nlist_tile<R, BS>(T, sx, a.tago, a.rl2, a.excl_start, a.excl_list, a.has_excl, a.act, ordered ? a.stage16 : a.nl16, a.S, ordered ? a.stage_cnt : a.nnh,
                              a.want32 ? a.nlist : (int*)nullptr, a.S, a.nn, ctl, &a.box, a.rtag, a.x4o, a.rl2_rows, sbase);
      }
      // row order: the sweep went into this workgroup's staging region, the rows reach their places now.  A tile beyond the
      // staging region (or a diagnostic build without rows) has been written in place, in the natural order.
      if (ordered) dev_row_order<BS>(T.geom[4], T.geom[5], a.S, a.row_P, a.stage16 + (size_t)sbase * a.S, a.stage_cnt + sbase, a.nl16, a.nnh,
                                     reinterpret_cast<int*>(chem_dyn_lds));
    }
    WGST(6);
    if (wst && t == 0) wst[7] = ndone;
    // order of the NEXT rebuild (and of the force launches behind it): wave 0 of workgroup x < 8 sorts the tiles of XCD
    // range x by home count, largest first -- eight classes relative to the mean, stable inside a class (ballot prefix)
    if (a.tile_ord && b < 8 && w == 0) {
      const int cntx = q + (b < r ? 1 : 0), off = b < r ? b * (q + 1) : r * (q + 1) + (b - r) * q;
      int* const ord_w = a.tile_ord + (size_t)(lpar ^ 1) * a.ntiles;
      int* const pos_w = a.tile_pos + (size_t)(lpar ^ 1) * a.ntiles;
      const int mean4 = (int)(((long long)a.n * 4 + a.ntiles - 1) / a.ntiles);      // class = 4 tn / mean, clamped: 7 classes above 7/4 of the mean ... 0
      auto cls_of = [&](int tile) { const int c = a.tn[tile] * 16 / (mean4 > 0 ? mean4 : 1); return 7 - (c > 7 ? 7 : c); };   // 0 = largest
      int tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int k0 = 0; k0 < cntx; k0 += 64) {
        const int k = k0 + lane, c = k < cntx ? cls_of(off + k) : -1;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) tot[cc] += __popcll(__ballot(c == cc));
      }
      int base[8]; { int acc_ = 0;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) { base[cc] = acc_; acc_ += tot[cc]; } }
      for (int k0 = 0; k0 < cntx; k0 += 64) {
        const int k = k0 + lane, c = k < cntx ? cls_of(off + k) : -1;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
          const unsigned long long m = __ballot(c == cc);
          if (c == cc) { const int p_ = off + base[cc] + __popcll(m & lanemask_lt()); ord_w[p_] = off + k; pos_w[off + k] = p_; }
          base[cc] += __popcll(m);
        }
      }
    }
    // bond pass: the list build ignored the exclusions, the bonded partners' slots of every home particle are recorded here for
    // the force launches up to the next rebuild (nothing in this launch reads them).  One tile per item, claimed like the chunks
    // of the work list below by workgroups that have run out of tiles; everything an item reads -- rtag, the sorted copies,
    // cell_start / cell_sub, the exclusion rows -- is complete since the last barrier, so nobody waits for anybody.
    if (a.bond_pass == 1 && a.bslots) {
      for (;;) {
        __syncthreads();
        if (t == 0) s_tile = (int)atomicAdd(&a.gb->bondq[0], 1u);
        __syncthreads();
        const int tile = s_tile;
        if (tile >= a.ntiles) break;
        tile_tables<R>(T, a.CAP, tile, a.cell_start, a.box, ctl, a.cell_sub);      // ends with a workgroup barrier
        dev_bond_slots_tile<R>(T, a.tago, a.excl_start, a.excl_list, a.rtag, nullptr, 0, 0x7fffffff, a.x4o, a.box, a.bslots, ctl);
      }
    }
    // bonded work list (nothing in this launch reads it): chunks of BS particles from a queue, taken by workgroups that
    // have run out of tiles -- as a fixed share in front of the tiles it was 25 us on every workgroup's critical path,
    // here it fills the idle tail of the phase (rtag is complete since the last barrier)
    if (a.nbent > 0) {
      for (;;) {
        __syncthreads();
        if (t == 0) s_tile = (int)atomicAdd(&a.gb->prepq[0], 1u);
        __syncthreads();
        const int ib = s_tile * BS;
        if (ib >= a.n) break;
        dev_bonded_prep_chunk<BS>(ib, a.n, a.tago, a.rtag, a.bstart, a.bent, a.bwork, a.bj, ctl, a.bslots ? a.excl_start : (const int*)nullptr);
      }
    }
    // copy-back (+ reference positions): every workgroup moves its share once it has no tile left
    for (int k = b * BS + t; k < a.n; k += NB * BS) {
      const Vec4<R> xk = a.x4o[k];
      a.x4[k] = xk; if (a.x0) a.x0[k] = xk;
      a.v4[k] = a.v4o[k]; a.img4[k] = a.img4o[k]; a.tag[k] = a.tago[k];
    }
  }
  // Lists this launch could not build -- a stencil beyond the LDS tile capacity, a row beyond its stride -- stop the run like a
  // full bucket row does (the particles are sorted and consistent, the forces of this step never evaluated): the host grows
  // the capacity at its next synchronisation and re-enters at this step (chem_api.hip: halted(), rebuild_now()).
  if (t == 0) {
    const volatile DevCtl* vc = ctl;
    if (vc->stage_overflow | vc->nl_overflow) { ctl->halt_step = a.istep; ctl->halt_par = a.par; ctl->halt = 3; if (b == 0 && a.hint) { volatile IdleHint* h = a.hint; h->halted = a.gen; } }
  }
  if (b == 0 && t == 0) a.gb->stamp[6] = wall_clock64();
  if (wst) { __syncthreads(); if (t == 0) wst[7] |= (long long)(wall_clock64() - wst[0]) << 16; }
#undef WGST
}

// =======================================================================================
// K11 observables (analysis.Temperature/KineticEnergy, start_simulation.py:453-493)
// =======================================================================================
template <typename R>
__global__ __launch_bounds__(256) void k_kinetic(int i0, int n, const Vec4<R>* __restrict__ v4, double* __restrict__ out) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  double ek = 0, px = 0, py = 0, pz = 0;
  if (i < i0 + n) {
    const Vec4<R> v = v4[i];
    const double m = (double)v.w, vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
    ek = 0.5 * m * (vx * vx + vy * vy + vz * vz); px = m * vx; py = m * vy; pz = m * vz;
  }
  __shared__ double red[4][4];
  for (int o = 32; o > 0; o >>= 1) { ek += __shfl_xor(ek, o); px += __shfl_xor(px, o); py += __shfl_xor(py, o); pz += __shfl_xor(pz, o); }
  if (lane_id() == 0) { int w = threadIdx.x >> 6; red[0][w] = ek; red[1][w] = px; red[2][w] = py; red[3][w] = pz; }
  __syncthreads();
  if (threadIdx.x < 4) {
    double s = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += red[threadIdx.x][k];
    out[4 * blockIdx.x + threadIdx.x] = s;
  }
}

// ---- velocity-rescaling thermostats (Berendsen, Isokinetic; start_simulation.py:341-348) --------
// k_kinetic leaves per-block (Ekin, p) partials; one block folds them into the scale factor, a
// streaming kernel applies it.  Decomposed path: the fold writes the local Ekin, the ranks sum it
// (transport all-reduce), k_rescale_lambda is launched with nblk = 0 and reads the sum.
__global__ __launch_bounds__(256) void k_rescale_lambda(const double* __restrict__ part, int nblk, double* __restrict__ ekin_io, double* __restrict__ lam_out,
                                                        int kind, double kT, double pref /* dt/tau */, double ntot, uint64_t svr_seed, uint64_t step) {
  __shared__ double red[4];
  double ek = 0;
  for (int k = threadIdx.x; k < nblk; k += blockDim.x) ek += part[4 * k];
  for (int o = 32; o > 0; o >>= 1) ek += __shfl_xor(ek, o);
  if (lane_id() == 0) red[threadIdx.x >> 6] = ek;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (nblk > 0) { ek = red[0] + red[1] + red[2] + red[3]; *ekin_io = ek; }
    else ek = *ekin_io;
    if (lam_out) {
      const double kTnow = 2.0 * ek / (3.0 * ntot);
      // kind 3: StochasticVelocityRescaling (one scalar draw per step, include/chem_philox.h; taut = tau/dt = 1/pref)
      *lam_out = kind == 1 ? sqrt(1.0 + pref * (kT / kTnow - 1.0)) : kind == 2 ? sqrt(kT / kTnow)
               : chem_philox::svr_lambda(svr_seed, step, ek, 1.5 * ntot * kT, (int64_t)(3.0 * ntot), 1.0 / pref);
    }
  }
}
template <typename R>
__global__ __launch_bounds__(256) void k_scale_v(int i0, int n, Vec4<R>* __restrict__ v4, const double* __restrict__ lam, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;   // (a stopped run must not keep rescaling its frozen velocities)
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= i0 + n) return;
  const R s = (R)*lam;
  Vec4<R> v = v4[i];
  v.x *= s; v.y *= s; v.z *= s;
  v4[i] = v;
}

// =======================================================================================
// K12 pressure and Berendsen barostat (analysis.Pressure, integrator.BerendsenBarostat; chem_baro_host.hpp)
// =======================================================================================
// sum of `nblk` values part[stride * k + off] by one block of 256, in an order that depends on nothing but nblk
__device__ __forceinline__ double baro_block_sum(const double* __restrict__ part, int nblk, int stride, int off, double* red) {
  double s = 0;
  for (int k = threadIdx.x; k < nblk; k += blockDim.x) s += part[(size_t)stride * k + off];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// Bonded virial: walks the bstart / bent / bpar entries of k_bonded<R, true>.  Member 0 of a pair entry contributes r_ij . F_ij
// once (as the energy does), so the sum is right on slabs, where the partner may be a ghost.  The force law is bonded_term's
// own (hybrid lambda and 1-4 Coulomb charges included: qtag is read for Coulomb entries only, hy.par for hybrid slots only).
// Triples and quadruples depend on angles alone: their virial vanishes identically, whatever their lambda, and is left at zero.
// vlist[e] = the share of entry e of bent (one word per entry, summed per list by k_list_sums; nullptr: not wanted); part[block] =
// the block's sum over all lists, reduced in a fixed order (what the barostat reads).  Both: the same bits for the same state.
template <typename R>
__global__ __launch_bounds__(256) void k_bonded_virial(int i0, int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag, const int* __restrict__ rtag,
                                                       const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                       const BondedParam* __restrict__ bpar, BoxD box, double* __restrict__ vlist, double* __restrict__ part,
                                                       DevCtl* ctl, BTab bt, HybridArgs hy, const R* __restrict__ qtag) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  double w = 0;
  if (i < i0 + n) {
    const int tg = tag[i];
    const int e0 = bstart[tg], e1 = bstart[tg + 1];
    for (int e = e0; e < e1; ++e) {
      const BondedEntry be = bent[e];
      const int slot = bonded_slot(be.meta), me = bonded_member(be.meta);
      const BondedParam& bp = bpar[slot];
      if (bp.arity == 4 || hybrid_wide_triple(bp)) ++e;      // (quadruples and hybrid triples occupy two consecutive entries)
      if (bp.arity != 2 || me != 0) continue;
      const int j0 = rtag[be.t0], j1 = rtag[be.t1];
      if ((j0 | j1) < 0) { ctl->bonded_missing = 1; continue; }
      double q0 = 0, q1 = 0;
      if (bp.kind == CHEM_POT_COULOMB_BOND) { q0 = (double)qtag[be.t0]; q1 = (double)qtag[be.t1]; }
      D3 f = {0, 0, 0};
      bonded_term<R, false, false, true, true>(bp, 0, j0, j1, 0, 0, x4, box, f, nullptr, ctl, bt, hybrid_lambda(hy, bp, slot, be.t2), q0, q1);
      const D3 d = minimgD(box, posD<R>(x4[j0], box) - posD<R>(x4[j1], box));
      const double t = dot3(d, f);
      if (vlist) vlist[e] = t;      // (the per-step launch of the barostat reads part[] alone)
      w += t;
    }
  }
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
  if (lane_id() == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// One block folds the partials of the step -- k_kinetic (Ekin at [4k]), the energy instantiation of the pair kernel (r.F at
// [3k + 2]; Coulomb term at [2k + 1]) and k_bonded_virial -- into P and mu.  out: [0] P, [1] mu, [2] mu^3, [3] sum m v^2,
// [4] non-bonded virial, [5] bonded virial.  mu = 1 where mu^3 <= 0: the host reads [2] and stops the run.
__global__ __launch_bounds__(256) void k_baro_mu(const double* __restrict__ ekpart, int nk, const double* __restrict__ epart, int ne, const double* __restrict__ qpart, int nq,
                                                 const double* __restrict__ bpart, int nbv, double volume, double dt, double tau, double p0, double* __restrict__ out) {
  __shared__ double red[4];
  const double ek = baro_block_sum(ekpart, nk, 4, 0, red);
  const double wnb = baro_block_sum(epart, ne, 3, 2, red) + baro_block_sum(qpart, nq, 2, 1, red);
  const double wb = baro_block_sum(bpart, nbv, 1, 0, red);
  if (threadIdx.x == 0) {
    const double mv2 = 2.0 * ek;
    const double p = baro_pressure(mv2, wnb + wb, volume);
    const double mu3 = baro_mu3(dt, tau, p0, p);
    out[0] = p; out[1] = baro_mu3_ok(mu3) ? baro_mu(mu3) : 1.0; out[2] = mu3; out[3] = mv2; out[4] = wnb; out[5] = wb;
  }
}
// The Langevin piston's kick (chem_barostat_langevin; the rules: chem_baro_host.hpp): one block folds the same partials as
// k_baro_mu into P, draws the step's uniform, moves the piston momentum kept in device memory (*pe) and computes the factors of
// the next step.  out: [0] P, [1] pe (new), [2] eps_dot, [3] sv, [4] mu, [5] sum m v^2, [6] non-bonded virial, [7] bonded virial.
// Where the new state is not acceptable (piston_ok) sv = mu = 1 are written and *pe keeps the value that says why: the host
// reads [1] and stops the run.
__global__ __launch_bounds__(256) void k_baro_piston(const double* __restrict__ ekpart, int nk, const double* __restrict__ epart, int ne, const double* __restrict__ qpart, int nq,
                                                     const double* __restrict__ bpart, int nbv, double volume, double dt, double p0, double w, double gamma_p, double kT,
                                                     double nf, uint64_t seed, uint64_t step, double* __restrict__ pe, double* __restrict__ out) {
  __shared__ double red[4];
  const double ek = baro_block_sum(ekpart, nk, 4, 0, red);
  const double wnb = baro_block_sum(epart, ne, 3, 2, red) + baro_block_sum(qpart, nq, 2, 1, red);
  const double wb = baro_block_sum(bpart, nbv, 1, 0, red);
  if (threadIdx.x == 0) {
    const double mv2 = 2.0 * ek;
    const double p = baro_pressure(mv2, wnb + wb, volume);
    uint32_t r[4];
    chem_philox::barostat_draw(seed, step, r);
    const double pe0 = *pe;
    const double pen = pe0 + dt * piston_force(volume, p, p0, nf, mv2, gamma_p, pe0, w, kT, dt, chem_philox::u01(r[0]));
    const double sv = piston_sv(pen, w, nf, dt), mu = piston_mu(pen, w, dt);
    const bool ok = piston_ok(pen, mu, sv);
    *pe = pen;
    out[0] = p; out[1] = pen; out[2] = pen / w; out[3] = ok ? sv : 1.0; out[4] = ok ? mu : 1.0; out[5] = mv2; out[6] = wnb; out[7] = wb;
  }
}
// After a scaling the tile descriptors of the last list build keep their lengths in the old unit: periodic shifts, the
// reference point and the cell edges of the staged coordinates, the fixed-point scale.  This kernel computes the tables of every
// tile again from the unchanged cell_start and the NEW box (tile_tables, the routine of the list build) and copies those
// fields alone into the descriptor in force -- the slot tables, the home runs and the list base (geom[5]) stay what the list
// was built with.  pos: the descriptor's place where the fused rebuild stores them in launch order (nullptr: by tile).
template <typename R>
__global__ __launch_bounds__(128) void k_baro_tile_desc(int ntiles, int CAP, const int* __restrict__ cell_start, Box<R> box,
                                                        TileLDS<R>* __restrict__ desc, DevCtl* ctl, const int* __restrict__ cell_sub,
                                                        const int* __restrict__ pos) {
  if (ctl->halt) return;
  __shared__ TileLDS<R> T;
  constexpr int a0 = (int)(offsetof(TileLDS<R>, cellshx) / 4), a1 = (int)(offsetof(TileLDS<R>, hstart) / 4);
  constexpr int b0 = (int)(offsetof(TileLDS<R>, org) / 4), b1 = (int)(sizeof(TileLDS<R>) / 4);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
    tile_tables<R>(T, CAP, tile, cell_start, box, ctl, cell_sub);
    const int* src = reinterpret_cast<const int*>(&T);
    int* dst = reinterpret_cast<int*>(&desc[pos ? pos[tile] : tile]);
    for (int k = a0 + (int)threadIdx.x; k < a1; k += blockDim.x) dst[k] = src[k];
    for (int k = b0 + (int)threadIdx.x; k < b1; k += blockDim.x) dst[k] = src[k];
  }
}
// x <- mu x about the origin.  Only the fp64 build keeps lengths in its position words; the fp32 build's are box fractions and
// follow the box lengths the host hands to the next launches.
__global__ __launch_bounds__(256) void k_baro_scale_x(int n, double4* __restrict__ x4, const double* __restrict__ mu, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = *mu;
  double4 x = x4[i];
  x.x *= s; x.y *= s; x.z *= s;
  x4[i] = x;
}

// =======================================================================================
// K13 pressure tensor (analysis.PressureTensor; rule set in include/chem_mi355.h "pressure tensor"; the kernel of a context:
//     chem_tensor_host.hpp).  Six components in the order xx, yy, zz, xy, xz, yz.  Launched by chem_get_pressure_tensor alone.
// =======================================================================================
// K_ab = sum m v_a v_b: out[6 * block + c]
template <typename R>
__global__ __launch_bounds__(256) void k_kinetic_tensor(int i0, int n, const Vec4<R>* __restrict__ v4, double* __restrict__ out) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  double tw[6] = {0, 0, 0, 0, 0, 0};
  if (i < i0 + n) {
    const Vec4<R> v = v4[i];
    const double m = (double)v.w, vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
    tensor_add(tw, vx, vy, vz, m * vx, m * vy, m * vz);
  }
  tensor_block_out<4>(tw, 1.0, out + 6 * (size_t)blockIdx.x);
}
// Bonded part: the walk of k_bonded_virial over every arity, the entry counted at member 0.  Pairs: d_ij (x) F_i.  Triples
// (i, j, k), centre j: d_ij (x) F_i + d_kj (x) F_k.  Quadruples (i, j, k, l): d_ij (x) F_i + d_kj (x) F_k + (d_kj + d_lk) (x) F_l.
// The forces are bonded_term's, one call per member, in its EXACT instantiation; the d are the minimum-image differences it forms.
// vlist[6 * e + c] = the share of entry e of bent (six words per entry, summed per list by k_list_sums; nothing reads a sum over
// the lists, so no block partials).
template <typename R>
__global__ __launch_bounds__(256) void k_bonded_virial_tensor(int i0, int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag, const int* __restrict__ rtag,
                                                              const int* __restrict__ bstart, const BondedEntry* __restrict__ bent,
                                                              const BondedParam* __restrict__ bpar, BoxD box, double* __restrict__ vlist,
                                                              DevCtl* ctl, BTab bt, HybridArgs hy, const R* __restrict__ qtag) {
  const int i = i0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < i0 + n) {
    const int tg = tag[i];
    const int e0 = bstart[tg], e1 = bstart[tg + 1];
    for (int e = e0; e < e1; ++e) {
      const BondedEntry be = bent[e];
      const int slot = bonded_slot(be.meta), me = bonded_member(be.meta);
      const BondedParam& bp = bpar[slot];
      const int ar = bp.arity;
      int j3 = 0;
      const int es = e;
      int tb = be.t2;      // the word that holds ~birth of a hybrid entry
      if (ar == 4) { const BondedEntry b2 = bent[e + 1]; j3 = rtag[b2.t0]; tb = b2.t2; ++e; }      // (quadruples occupy two consecutive entries,
      else if (hybrid_wide_triple(bp)) { tb = bent[e + 1].t2; ++e; }                             //  hybrid triples too)
      if (me != 0) continue;
      const int j0 = rtag[be.t0], j1 = rtag[be.t1], j2 = ar > 2 ? rtag[be.t2] : 0;
      if ((j0 | j1 | j2 | j3) < 0) { ctl->bonded_missing = 1; continue; }
      double q0 = 0, q1 = 0;
      if (bp.kind == CHEM_POT_COULOMB_BOND) { q0 = (double)qtag[be.t0]; q1 = (double)qtag[be.t1]; }
      const double lam = hybrid_lambda(hy, bp, slot, tb);
      const D3 x0 = posD<R>(x4[j0], box), x1 = posD<R>(x4[j1], box);
      const D3 dij = minimgD(box, x0 - x1);
      double t[6] = {0, 0, 0, 0, 0, 0};
      D3 f = {0, 0, 0};
      bonded_term<R, false, false, true, true, true>(bp, 0, j0, j1, j2, j3, x4, box, f, nullptr, ctl, bt, lam, q0, q1);
      tensor_add(t, dij.x, dij.y, dij.z, f.x, f.y, f.z);
      if (ar > 2) {
        const D3 dkj = minimgD(box, posD<R>(x4[j2], box) - x1);
        f = {0, 0, 0};
        bonded_term<R, false, false, true, true, true>(bp, 2, j0, j1, j2, j3, x4, box, f, nullptr, ctl, bt, lam, q0, q1);
        tensor_add(t, dkj.x, dkj.y, dkj.z, f.x, f.y, f.z);
        if (ar == 4) {
          const D3 dlj = dkj + minimgD(box, posD<R>(x4[j3], box) - posD<R>(x4[j2], box));
          f = {0, 0, 0};
          bonded_term<R, false, false, true, true, true>(bp, 3, j0, j1, j2, j3, x4, box, f, nullptr, ctl, bt, lam, q0, q1);
          tensor_add(t, dlj.x, dlj.y, dlj.z, f.x, f.y, f.z);
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) vlist[6 * (size_t)es + c] = t[c];
    }
  }
}
// Sums per list of what the observable passes above left per entry: block (l, c) of nlists * ncomp adds val[ncomp * e + c] over
// the entries e < *nent of list l -- strided over the block's threads, then folded in a fixed tree -- into out[ncomp * l + c].
// The order depends on the entry table alone (not on atomics, not on where the particles sit), so a state gives the same bits
// every time it is observed, in every context that holds it.  (The second entry of a quadruple carries no slot: it reads as
// slot 0 and holds zero.)
__global__ __launch_bounds__(256) void k_list_sums(const int* __restrict__ nent, int ncomp, const BondedEntry* __restrict__ bent, const BondedParam* __restrict__ bpar,
                                                   const double* __restrict__ val, double* __restrict__ out) {
  const int l = (int)blockIdx.x / ncomp, c = (int)blockIdx.x % ncomp, ne = *nent;
  double s = 0;
  for (int e = threadIdx.x; e < ne; e += 256) if (bpar[bonded_slot(bent[e].meta)].list == l) s += val[(size_t)ncomp * e + c];
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane_id() == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// Non-bonded part, per-particle rows: the TENSOR instantiation of pair_force_body, four lanes per particle, both table kinds.
// MODE 0 the plain kernel, 4 Coulomb, 5 resolution, 6 caps, 7 resolution and caps (chem_tensor_host.hpp tensor_plan); f4 is scratch.
template <typename R, int MODE>
__global__ __launch_bounds__(256) void k_pair_force_tensor(int n, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                           const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                           Box<R> box, const PairCore<R>* __restrict__ pcore,
                                                           const PairExt<R>* __restrict__ pext, int ntypes,
                                                           const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                           double half_skin, DevCtl* ctl, CoulArgs<R> ca, ResArgs<R> ra, CapArgs<R> cp, double* __restrict__ tout) {
  static_assert(MODE == 0 || (MODE >= 4 && MODE <= 7), "row tensor kernels: MODE 0, 4, 5, 6, 7");
  pair_force_body<R, 4, true, true, MODE == 4, MODE == 5 || MODE == 7, MODE == 6 || MODE == 7, true>(n, x4, f4, nlist, nn, S, box, pcore, pext, ntypes, tab, eout, half_skin, ctl, ca, ra, cp, tout);
}
// ... tiles: the TENSOR instantiation of pair_tiles_body, one lane per particle, 512 threads.  MODE 3 (general, both table kinds:
// what the energy pass of MODE 0..3 evaluates, the excluded pairs of inline bonds taken out again) and 4..7.
template <typename R, int MODE>
__global__ __launch_bounds__(512, sizeof(R) == 8 ? 4 : 1536 / 256) void k_pair_tiles_tensor(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ f4,
                                                           const TileLDS<R>* __restrict__ desc, const unsigned short* __restrict__ nl16,
                                                           const int* __restrict__ nnh, int S16,
                                                           const PairCore<R>* __restrict__ pcore, const PairExt<R>* __restrict__ pext,
                                                           int ntypes, const Vec4<R>* __restrict__ tab, double* __restrict__ eout,
                                                           double half_skin, DevCtl* ctl, TileSub sub_, BondRecs bslots, int bond_mode, ActMask bact,
                                                           CoulArgs<R> ca, ResArgs<R> ra, CapArgs<R> cp, double* __restrict__ tout) {
  static_assert(MODE >= 3 && MODE <= 7, "tile tensor kernels: MODE 3..7");
  pair_tiles_body<R, 1, true, 512, MODE, false, true>(ntiles, CAP, x4, f4, desc, nl16, nnh, S16, pcore, pext, ntypes, tab, UniLJ{}, eout, half_skin, ctl, 0, 0, nullptr,
                                                      sub_, DecideArgs{}, bslots, 0.0, 0.0, bond_mode, bact, ca, ra, cp, tout);
}

// =======================================================================================
// K9/K10  reaction scan + resolve (integrator.ChemicalReaction / Reaction,
//     reaction_setup.py:71-165,416-427)
// =======================================================================================
struct ReactionDev {
  int type_1, type_2, delta_1, delta_2;
  int min1, max1, min2, max2;
  int intramolecular, intraresidual, active, restricted;   // restricted: RestrictReaction -- only pairs of the connection table react
  int cons_role, pad_;   // ReactionConstraintNeighbourState on role 1 | 2: the host evaluates it per particle into a bit table (ConnTable::cons_ok)
  double cut2, mincut2, prob;
};
struct ReactSet { int n; uint64_t seed; uint64_t step; int nearest; ReactionDev r[CHEM_MAX_REACTIONS]; };
// RestrictReaction.define_connection (reaction_setup.py:115-128): per-tag CSR of the allowed partners, one bit per reaction
struct ConnTable { const int* start; const int* partner; const unsigned int* mask; const unsigned int* cons_ok; };   // cons_ok[tag]: bit q = constraint of reaction q holds
__device__ __forceinline__ bool conn_allows(const ConnTable& ct, int ta, int tb, int q) {
  if (!ct.start) return false;
  for (int e = ct.start[ta]; e < ct.start[ta + 1]; ++e) if (ct.partner[e] == tb) return (ct.mask[e] >> q) & 1u;
  return false;
}

struct Candidate { int a, b, r; unsigned int h; double d2; };  // a: role type_1, b: role type_2 (tags)

// Traverses the Verlet list once (pairs with tag_i < tag_j), applies the type/state/res_id
// filters, evaluates the distance criterion in fp64 without FMA contraction (bit-comparable
// with the CPU oracle) and appends the hits with one atomic per wave (ballot compaction).
template <typename R>
__global__ __launch_bounds__(256) void k_react_scan(int i0, int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                    const int* __restrict__ nlist, const int* __restrict__ nn, int S,
                                                    const int* __restrict__ state, const int* __restrict__ res_id,
                                                    const int* __restrict__ mol_id, BoxD box, const ReactSet* __restrict__ rs_g,
                                                    Candidate* __restrict__ cand, int cand_cap, DevCtl* ctl, ConnTable conn) {
  __shared__ ReactSet rs;
  {
    const int* src = reinterpret_cast<const int*>(rs_g);
    int* dst = reinterpret_cast<int*>(&rs);
    for (int k = threadIdx.x; k < (int)(sizeof(ReactSet) / 4); k += blockDim.x) dst[k] = src[k];
  }
  __syncthreads();
  // 8 lanes per particle row; hits are staged per wave in LDS (wave-private region)
  constexpr int TPP = 8;
  constexpr int kWaveBuf = 192;
  __shared__ Candidate sbuf[4 * kWaveBuf];
  Candidate* wbuf = sbuf + (threadIdx.x >> 6) * kWaveBuf;
  int wcount = 0;   // wave-uniform
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = i0 + gid / TPP, sub = gid % TPP;
  int cnt = 0, ti = 0, si = 0, tgi = 0, ri = 0, mi = 0;
  Vec4<R> xi = mk4<R>(0, 0, 0, 0);
  const int* row = nullptr;
  if (i < i0 + n) {
    xi = x4[i]; ti = (int)xi.w; tgi = tag[i]; si = state[tgi]; ri = res_id[tgi]; mi = mol_id[tgi];
    cnt = nn[i]; row = nlist + (size_t)i * S;
    // quick reject: particle cannot take part in any active reaction
    bool any = false;
    for (int q = 0; q < rs.n; ++q) {
      const ReactionDev& R_ = rs.r[q];
      if (!R_.active) continue;
      any |= (ti == R_.type_1 && si >= R_.min1 && si < R_.max1) || (ti == R_.type_2 && si >= R_.min2 && si < R_.max2);
    }
    if (!any) cnt = 0;
  }
  float maxcut2f = 0;
  for (int q = 0; q < rs.n; ++q) if (rs.r[q].active) maxcut2f = fmaxf(maxcut2f, (float)rs.r[q].cut2);
  maxcut2f *= 1.001f;
  const float bLf[3] = {(float)box.L[0], (float)box.L[1], (float)box.L[2]}, biLf[3] = {(float)box.invL[0], (float)box.invL[1], (float)box.invL[2]};
  // uniform trip count inside a wave so that __ballot is convergent
  int maxcnt = cnt;
  for (int o = 32; o > 0; o >>= 1) { int t = __shfl_xor(maxcnt, o); maxcnt = t > maxcnt ? t : maxcnt; }
  for (int k0 = 0; k0 < maxcnt; k0 += TPP) {
    const int k = k0 + sub;
    int j = -1, tj = 0, sj = 0, tgj = 0, rj = 0, mj = 0;
    bool live = k < cnt;
    Vec4<R> xj = xi;
    if (live) {
      j = row[k]; tgj = tag[j];
      live = tgi < tgj;
      if (live) {
        xj = x4[j];
        // cheap reject before the three by-tag gathers and the fp64 arithmetic: the reaction radii are
        // far inside the list radius (1.2 vs 2.8: 8 % of the neighbours).  Same inputs as the fp64
        // distance below, 1e-3 relative margin >> any rounding difference.
        const D3 pi_ = posD<R>(xi, box), pj_ = posD<R>(xj, box);
        const float fx = (float)(pi_.x - pj_.x), fy = (float)(pi_.y - pj_.y), fz = (float)(pi_.z - pj_.z);
        const float gx = fx - bLf[0] * rintf(fx * biLf[0]), gy = fy - bLf[1] * rintf(fy * biLf[1]), gz = fz - bLf[2] * rintf(fz * biLf[2]);
        live = gx * gx + gy * gy + gz * gz <= maxcut2f;
      }
      if (live) { tj = (int)xj.w; sj = state[tgj]; rj = res_id[tgj]; mj = mol_id[tgj]; }
    }
    double d2 = 0;
    if (__any(live)) {
      if (live) {
        D3 d = minimgD(box, posD<R>(xi, box) - posD<R>(xj, box));
        d2 = dist2_unfused(d);
      }
      for (int q = 0; q < rs.n; ++q) {
        const ReactionDev& R_ = rs.r[q];
        bool hit = false; int a = 0, b = 0; unsigned int h = 0;
        if (live && R_.active) {
          const bool fwd = ti == R_.type_1 && si >= R_.min1 && si < R_.max1 && tj == R_.type_2 && sj >= R_.min2 && sj < R_.max2;
          const bool rev = tj == R_.type_1 && sj >= R_.min1 && sj < R_.max1 && ti == R_.type_2 && si >= R_.min2 && si < R_.max2;
          if (fwd || rev) {
            hit = true;
            if (fwd) { a = tgi; b = tgj; } else { a = tgj; b = tgi; }   // tgi < tgj: forward role assignment wins
            if (!R_.intraresidual && ri == rj) hit = false;
            if (!R_.intramolecular && mi == mj) hit = false;
            if (!(d2 >= R_.mincut2 && d2 < R_.cut2)) hit = false;
            if (hit && R_.restricted && !conn_allows(conn, tgi, tgj, q)) hit = false;
            if (hit && R_.cons_role && !((conn.cons_ok[R_.cons_role == 1 ? a : b] >> q) & 1u)) hit = false;
            if (hit) {
              uint32_t rr[4];
              chem_philox::reaction_draw(rs.seed, rs.step, (uint32_t)tgi, (uint32_t)tgj, (uint32_t)q, rr);
              if (R_.prob < 1.0 && !(chem_philox::u01(rr[0]) < R_.prob)) hit = false;
              h = rr[1];
            }
          }
        }
        const unsigned long long m = __ballot(hit);
        if (m) {
          const int nh = __popcll(m);
          if (wcount + nh > kWaveBuf) {   // flush this wave's staged hits: one global atomic per flush
            int base = 0;
            if (lane_id() == 0) base = atomicAdd(&ctl->cand_count, wcount);
            base = __shfl(base, 0);
            for (int t = lane_id(); t < wcount; t += 64) { if (base + t < cand_cap) cand[base + t] = wbuf[t]; else ctl->cand_overflow = 1; }
            wcount = 0;
          }
          if (hit) wbuf[wcount + __popcll(m & lanemask_lt())] = Candidate{a, b, q, h, d2};
          wcount += nh;
        }
      }
    }
  }
  if (wcount > 0) {
    int base = 0;
    if (lane_id() == 0) base = atomicAdd(&ctl->cand_count, wcount);
    base = __shfl(base, 0);
    for (int t = lane_id(); t < wcount; t += 64) { if (base + t < cand_cap) cand[base + t] = wbuf[t]; else ctl->cand_overflow = 1; }
  }
}

// ---- reaction scan on the staged tiles, WITHOUT rebuilding anything.
// Role words of the reaction scan on tiles: for every particle slot (position order) one bit per reaction and role -- bit q:
// "type and state fit role 1 of (active) reaction q", bit 16 + q: role 2 (CHEM_MAX_REACTIONS = 16).  One streaming pass in
// front of the scan (tag -> state is the only gather); the scan stages the words beside the positions (4 bytes per slot), so
// that the role compatibility of a candidate pair is decided in LDS and only the pairs that can react reach the dependent
// global loads (tags, exclusion row, labels, exact fp64 distance).
template <typename R>
__global__ __launch_bounds__(256) void k_react_roles(int nslot, int ntag, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                     const int* __restrict__ state, const ReactSet* __restrict__ rs_g, unsigned int* __restrict__ role) {
  __shared__ ReactSet rs;
  {
    const int* src = reinterpret_cast<const int*>(rs_g);
    int* dst = reinterpret_cast<int*>(&rs);
    for (int k = threadIdx.x; k < (int)(sizeof(ReactSet) / 4); k += 256) dst[k] = src[k];
  }
  __syncthreads();
  for (int g = blockIdx.x * 256 + threadIdx.x; g < nslot; g += gridDim.x * 256) {
    const int tg = tag[g];
    unsigned int bits = 0;
    if (tg >= 0 && tg < ntag) {
      const int t = (int)x4[g].w, st = state[tg];
      for (int q = 0; q < rs.n; ++q) {
        const ReactionDev& R_ = rs.r[q];
        if (!R_.active) continue;
        if (t == R_.type_1 && st >= R_.min1 && st < R_.max1) bits |= 1u << q;
        if (t == R_.type_2 && st >= R_.min2 && st < R_.max2) bits |= 1u << (16 + q);
      }
    }
    role[g] = bits;
  }
}
// stages role[g] of every stencil slot (same addressing as tile_fill's register-lean form)
template <typename R, int BS>
__device__ __forceinline__ void tile_fill_roles(const TileLDS<R>& T, unsigned int* const sr, const int CAP, const unsigned int* __restrict__ role) {
  constexpr int NW = BS / 64;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int r = w; r < NROW; r += NW) {
    const int len = T.celloff[r][SX], o0 = T.rowoff[r];
    for (int e = l; e < len; e += 64) {
      int k = 0;
#pragma unroll
      for (int q = 1; q < SX; ++q) k += (e >= T.celloff[r][q]) ? 1 : 0;
      const int g = T.cellg[r][k] + (e - T.celloff[r][k]);
      if (o0 + e < CAP) sr[o0 + e] = role[g];
    }
  }
}
__host__ __device__ constexpr size_t scan_roles_offset(int CAP, size_t slot_bytes) { return ((size_t)(CAP + 5) * slot_bytes + 15) / 16 * 16; }

// The int32-list scan above needs a fresh list, i.e. a forced rebuild at the reaction step -- and a
// rebuild re-sorts the particles but not their forces, which the next half-kick still needs (the
// reaction sits between the force evaluation of step s and the first kick of step s+1).  This
// kernel needs no list: two particles within a reaction radius (<= rc) now were within
// radius + skin <= rc + skin = one cell edge at the last rebuild, so the 27-cell stencil of the
// tile tables of THAT rebuild still contains every candidate, with the current positions staged
// into LDS.  Per home particle: fp32 pre-test of the stencil candidates against the largest
// reaction radius, then for the few survivors (tag order, states, labels) the fp64 distance from
// the global arrays exactly as k_react_scan computes it, the reaction filters and the Philox draw.
// Round 3: tag and role bits are staged beside the positions (k_react_roles), so a home particle without a role costs
// nothing and a candidate reaches the global loads only if tag order and roles allow a reaction.
// (k_rdf_tiles further down walks the stencil the same way -- home decode, x-window with slack, four-wide LDS gather, lower-tag
//  rule -- as a copy: a change to the traversal here has to be made there too.)
// Output: every tile appends to its own fixed region of `region` through an LDS counter (no
// contended global atomic); k_cand_offsets / k_cand_gather compact the regions afterwards.
template <typename R, int BS>
__global__ __launch_bounds__(BS, 4) void k_react_scan_tiles(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                            const TileLDS<R>* __restrict__ desc, const int* __restrict__ state,
                                                            const int* __restrict__ res_id, const int* __restrict__ mol_id, BoxD box,
                                                            const ReactSet* __restrict__ rs_g, Candidate* __restrict__ region, int region_cap,
                                                            int* __restrict__ tile_count, DevCtl* ctl, R slack,
                                                            const int* __restrict__ excl_start, const int* __restrict__ excl_list, ConnTable conn,
                                                            const unsigned int* __restrict__ role, int roles_staged,      // (roles_staged 0: the image leaves no room behind it -- role words from global memory)
                                                            const int* __restrict__ direct_off, int* __restrict__ tile_need) {
  // tile_need[tile]: the candidates the tile found, however many fitted its region.  Second pass of a step in which a region was
  // too small (direct_off != nullptr; rescan_crowded_tiles): `region` is the candidate array itself, the tile writes its
  // tile_need[tile] records at direct_off[tile], the exclusive scan of tile_need.
  __shared__ TileLDS<R> T;
  __shared__ ReactSet rs;
  __shared__ int s_cnt;
  CHEM_DYN_LDS(R);
  unsigned int* const sr = reinterpret_cast<unsigned int*>(chem_dyn_lds + scan_roles_offset(CAP, sizeof(Vec4<R>)));   // role words behind the image
  {
    const int* src = reinterpret_cast<const int*>(rs_g);
    int* dst = reinterpret_cast<int*>(&rs);
    for (int k = threadIdx.x; k < (int)(sizeof(ReactSet) / 4); k += BS) dst[k] = src[k];
  }
  __syncthreads();
  R maxcut2 = 0;
  for (int q = 0; q < rs.n; ++q) if (rs.r[q].active) maxcut2 = rs.r[q].cut2 > (double)maxcut2 ? (R)rs.r[q].cut2 : maxcut2;
  maxcut2 *= (R)1.001;   // the staged positions carry the periodic shift: one more rounding than the global ones
  for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    const int tile = xcd_remap(vb, ntiles);
    __syncthreads();
    tile_load_desc<R>(T, desc, tile);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    tile_fill<R, BS, true>(T, sx, CAP, x4, 1);
    if (roles_staged) tile_fill_roles<R, BS>(T, sr, CAP, role);
    __syncthreads();
    const int hx = T.geom[0], total = T.geom[3], nhome = T.geom[4];
    if (roles_staged && threadIdx.x == 0 && total < CAP) sr[total] = 0u;      // (the far-away dummy slot: no role)
    __syncthreads();
    Candidate* out = direct_off ? region + direct_off[tile] : region + (size_t)tile * region_cap;
    const int cap = direct_off ? tile_need[tile] : region_cap;
    for (int q = threadIdx.x; q < nhome; q += BS) {
      int sgi = 0;
#pragma unroll
      for (int k = 1; k < NHSEG; ++k) sgi += (q >= T.hoff[k]) ? 1 : 0;
      const int inrun = q - T.hoff[sgi];
      const int p = T.hstart[sgi] + inrun;
      const int ly = sgi % HY, lz = sgi / HY;
      const int hr = (lz + 1) * SY + (ly + 1);
      const int eh = inrun + T.celloff[hr][1];
      int lx = 0;
      for (int k = 2; k <= hx; ++k) lx += (eh >= T.celloff[hr][k]) ? 1 : 0;
      const int sself = T.rowoff[hr] + eh;
      const unsigned int rwi = roles_staged ? sr[sself] : role[p];
      if (!rwi) continue;                                     // no role in any active reaction
      const Vec4<R> xi = sx[sself];
      const int tgi = tag[p];
      const unsigned int ri1 = rwi & 0xffffu, ri2 = rwi >> 16;
      const int ri = res_id[tgi], mi = mol_id[tgi];
      const Vec4<R> xgi = x4[p];
      // x-window of every stencil row, as in the list build (dev_nlist_tile) but for the largest reaction radius and
      // with the tables of the LAST rebuild: a candidate sits within `slack` (= skin/2) of where it was binned, so the
      // row distances shrink and the window grows by that much
      const R rmax = sqrt_r(maxcut2), weps = T.clen[0] * (R)2e-4;
      auto suboff = [&](int r, int f, bool lower) {
        const int k = f >> 2, j = f & 3;
        const int base = T.celloff[r][k];
        if (j == 0) return base;
        const int pk = T.cellsub[r][k];
        if (pk < 0) return lower ? base : T.celloff[r][k + 1];
        return base + ((pk >> (8 * (j - 1))) & 0xff);
      };
#pragma unroll 1
      for (int dzy = 0; dzy < 9; ++dzy) {
        const int dz = dzy / 3, dy = dzy - 3 * dz;
        const int r = (lz + dz) * SY + (ly + dy);
        const R ylo = ((R)(ly + 1) - (R)kRefCells) * T.clen[1], zlo = ((R)(lz + 1) - (R)kRefCells) * T.clen[2];   // (staged coordinates are relative to T.org)
        R ddy = dy == 0 ? xi.y - ylo : (dy == 2 ? ylo + T.clen[1] - xi.y : (R)0);
        R ddz = dz == 0 ? xi.z - zlo : (dz == 2 ? zlo + T.clen[2] - xi.z : (R)0);
        ddy -= slack + weps; ddz -= slack + weps;
        ddy = ddy > 0 ? ddy : (R)0; ddz = ddz > 0 ? ddz : (R)0;
        const R w2 = rmax * rmax - ddy * ddy - ddz * ddz;
        if (w2 < (R)0) continue;
        const R ws = (sqrt_r(w2) + slack + weps) * T.subinv, sxi = (xi.x + (R)kRefCells * T.clen[0]) * T.subinv;
        int f_lo = (int)(sxi - ws), f_hi = (int)(sxi + ws);
        f_lo = f_lo > lx * NSUB ? f_lo : lx * NSUB;
        f_hi = f_hi < (lx + 3) * NSUB - 1 ? f_hi : (lx + 3) * NSUB - 1;
        const int a = T.rowoff[r] + suboff(r, f_lo, true);
        int b = T.rowoff[r] + suboff(r, f_hi + 1, false);
        b = b < total ? b : total;
        // four candidates per trip: their LDS reads are issued together (one latency per four tests; slots behind the
        // run read the far-away dummy at `total`)
        for (int sl0 = a; sl0 < b; sl0 += 4) {
          Vec4<R> xq[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) xq[u] = lds_gather4<R>(sx, sl0 + u < b ? sl0 + u : total);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
          const int sl = sl0 + u;
          const Vec4<R> xj = xq[u];
          const R dx = xi.x - xj.x, dy_ = xi.y - xj.y, dz_ = xi.z - xj.z;
          if (dx * dx + dy_ * dy_ + dz_ * dz_ > maxcut2 || sl == sself || sl >= b) continue;
          const unsigned int rwj = roles_staged ? sr[sl] : role[real_as_idx(xj.w) >> 5];
          const unsigned int fwdm = ri1 & (rwj >> 16), revm = ri2 & (rwj & 0xffffu);   // bit q: reaction q with (i, j) as roles (1, 2) / (2, 1)
          if (!(fwdm | revm)) continue;
          const int j = real_as_idx(xj.w) >> 5;
          const int tgj = tag[j];
          if (!(tgi < tgj)) continue;          // every pair once, from its lower tag (on the rank that owns it)
          if (excl_start) {                    // candidates are Verlet-list pairs: an excluded (e.g. bonded) pair never reacts
            bool ex = false;
            for (int e = excl_start[tgi]; e < excl_start[tgi + 1]; ++e) ex |= excl_list[e] == tgj;
            if (ex) continue;
          }
          const int rj = res_id[tgj], mj = mol_id[tgj];
          const D3 d = minimgD(box, posD<R>(xgi, box) - posD<R>(x4[j], box));
          const double d2 = dist2_unfused(d);
          for (int k = 0; k < rs.n; ++k) {
            const ReactionDev& R_ = rs.r[k];
            const bool fwd = (fwdm >> k) & 1u, rev = (revm >> k) & 1u;      // (bits exist for active reactions only)
            if (!(fwd || rev)) continue;
            if (!R_.intraresidual && ri == rj) continue;
            if (!R_.intramolecular && mi == mj) continue;
            if (!(d2 >= R_.mincut2 && d2 < R_.cut2)) continue;
            if (R_.restricted && !conn_allows(conn, tgi, tgj, k)) continue;
            if (R_.cons_role && !((conn.cons_ok[(R_.cons_role == 1) == fwd ? tgi : tgj] >> k) & 1u)) continue;   // (role 1 is tgi on a forward match)
            uint32_t rr[4];
            chem_philox::reaction_draw(rs.seed, rs.step, (uint32_t)tgi, (uint32_t)tgj, (uint32_t)k, rr);
            if (R_.prob < 1.0 && !(chem_philox::u01(rr[0]) < R_.prob)) continue;
            const int idx = atomicAdd(&s_cnt, 1);
            if (idx < cap) out[idx] = fwd ? Candidate{tgi, tgj, k, rr[1], d2} : Candidate{tgj, tgi, k, rr[1], d2};   // tgi < tgj: forward role assignment wins
            else ctl->cand_overflow = 1;
          }
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) { tile_count[tile] = s_cnt < cap ? s_cnt : cap; if (!direct_off) tile_need[tile] = s_cnt; }
  }
}

// exclusive scan of the per-tile candidate counts (single block) -> tile_off, total -> ctl->cand_count
__global__ __launch_bounds__(1024) void k_cand_offsets(int ntiles, const int* __restrict__ tile_count, int* __restrict__ tile_off, DevCtl* ctl) {
  __shared__ int ws[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = lane_id();
  for (int base = 0; base < ntiles; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < ntiles ? tile_count[i] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < 16; ++k) { if (k < w) off += ws[k]; tot += ws[k]; }
    if (i < ntiles) tile_off[i] = carry_s + off + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) carry_s += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) ctl->cand_count = carry_s;
}

__global__ __launch_bounds__(256) void k_cand_gather(int ntiles, const Candidate* __restrict__ region, int region_cap, const int* __restrict__ tile_count,
                                                     const int* __restrict__ tile_off, Candidate* __restrict__ cand, int cand_cap, DevCtl* ctl) {
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int c = tile_count[tile], o = tile_off[tile];
    const Candidate* src = region + (size_t)tile * region_cap;
    for (int k = threadIdx.x; k < c; k += blockDim.x) { if (o + k < cand_cap) cand[o + k] = src[k]; else ctl->cand_overflow = 1; }
  }
}

// ---- resolve: UniqueA, UniqueB, one-event-per-particle (parallel greedy) -------------
__device__ __forceinline__ unsigned long long cand_key1(const Candidate& c, int nearest) {
  return nearest ? (unsigned long long)__double_as_longlong(c.d2) : (unsigned long long)c.h;
}

// pass 1 of a segmented arg-min: best1[p] = min key1; side 0: p = a, side 1: p = b
__global__ void k_res_min1(int nc, const Candidate* __restrict__ c, const int* __restrict__ alive, int side, int nearest,
                           unsigned long long* __restrict__ best1) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc || !alive[k]) return;
  atomicMin(&best1[side ? c[k].b : c[k].a], cand_key1(c[k], nearest));
}
// pass 2: tie-break on (partner tag, reaction)
__global__ void k_res_min2(int nc, const Candidate* __restrict__ c, const int* __restrict__ alive, int side, int nearest,
                           const unsigned long long* __restrict__ best1, unsigned long long* __restrict__ best2) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc || !alive[k]) return;
  const int p = side ? c[k].b : c[k].a, o = side ? c[k].a : c[k].b;
  if (cand_key1(c[k], nearest) == best1[p]) atomicMin(&best2[p], ((unsigned long long)(unsigned)o << 8) | (unsigned)c[k].r);
}
__global__ void k_res_keep(int nc, const Candidate* __restrict__ c, int* __restrict__ alive, int side, int nearest,
                           const unsigned long long* __restrict__ best1, const unsigned long long* __restrict__ best2) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc || !alive[k]) return;
  const int p = side ? c[k].b : c[k].a, o = side ? c[k].a : c[k].b;
  const bool keep = cand_key1(c[k], nearest) == best1[p] && ((((unsigned long long)(unsigned)o << 8) | (unsigned)c[k].r) == best2[p]);
  if (!keep) alive[k] = 0;
}
// after UniqueA+UniqueB every particle is 'a' of at most one and 'b' of at most one survivor
__global__ void k_res_index(int nc, const Candidate* __restrict__ c, const int* __restrict__ alive, int* __restrict__ asA,
                            int* __restrict__ asB) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc || !alive[k]) return;
  asA[c[k].a] = k; asB[c[k].b] = k;
}
__device__ __forceinline__ bool cand_less(const Candidate& p, const Candidate& q, int nearest) {
  const unsigned long long kp = cand_key1(p, nearest), kq = cand_key1(q, nearest);
  return kp != kq ? kp < kq : p.a < q.a;
}
// one round of priority greedy matching: status 1 alive, 2 accepted, 0 dead
__global__ void k_res_round(int nc, const Candidate* __restrict__ c, const int* __restrict__ st_in, int* __restrict__ st_out,
                            const int* __restrict__ asA, const int* __restrict__ asB, int nearest, DevCtl* ctl) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc) return;
  int s = st_in[k];
  if (s == 1) {
    // neighbours: pairs sharing a particle with k
    int nb[4] = {asB[c[k].a], asA[c[k].b], asA[c[k].a], asB[c[k].b]};
    bool ismin = true, dead = false;
    for (int q = 0; q < 4; ++q) {
      const int o = nb[q];
      if (o < 0 || o == k) continue;
      const int so = st_in[o];
      if (so == 2) dead = true;
      else if (so == 1 && cand_less(c[o], c[k], nearest)) ismin = false;
    }
    if (dead) s = 0; else if (ismin) s = 2; else ctl->alive = 1;
  }
  st_out[k] = s;
}

// apply accepted events: state/type/mass on the device arrays, emit compact event records
struct ReactApply { int delta_1, delta_2, new_type_1, new_type_2; double new_mass_1, new_mass_2; };
struct ReactApplySet { ReactApply r[CHEM_MAX_REACTIONS]; };
template <typename R>
__global__ void k_react_apply(int nc, const Candidate* __restrict__ c, const int* __restrict__ st, ReactApplySet ras,
                              int* __restrict__ state, const int* __restrict__ rtag, Vec4<R>* __restrict__ x4,
                              Vec4<R>* __restrict__ v4, Candidate* __restrict__ out, int* __restrict__ out_count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const bool acc = k < nc && st[k] == 2;
  // output slot: one atomic per wave (a same-address atomic per event serialises in the L2: 250 us for 2.8e5 events)
  const unsigned long long m = __ballot(acc);
  if (!m) return;
  int base = 0;
  if (lane_id() == __ffsll((long long)m) - 1) base = atomicAdd(out_count, __popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (!acc) return;
  const Candidate cd = c[k];
  const ReactApply ra = ras.r[cd.r];
  state[cd.a] += ra.delta_1; state[cd.b] += ra.delta_2;
  // (the new mass goes with a CHANGE of type: an event that names the type the particle already has leaves its mass alone, as the host mirror and the oracle do)
  if (ra.new_type_1 >= 0) { int i = rtag[cd.a]; if (i >= 0 && x4[i].w != (R)ra.new_type_1) { x4[i].w = (R)ra.new_type_1; v4[i].w = (R)ra.new_mass_1; } }
  if (ra.new_type_2 >= 0) { int i = rtag[cd.b]; if (i >= 0 && x4[i].w != (R)ra.new_type_2) { x4[i].w = (R)ra.new_type_2; v4[i].w = (R)ra.new_mass_2; } }
  out[base + __popcll(m & lanemask_lt())] = cd;
}

// property changes computed by the host topology manager (PostProcessChangeNeighboursProperty): by tag
struct PropChangeDev { int tag, type, set_state, state; double mass, q; };
template <typename R>
__global__ void k_apply_props(int nchg, const PropChangeDev* __restrict__ chg, int* __restrict__ state, const int* __restrict__ rtag,
                              Vec4<R>* __restrict__ x4, Vec4<R>* __restrict__ v4) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nchg) return;
  const PropChangeDev c = chg[k];
  if (c.set_state) state[c.tag] = c.state;
  const int i = rtag[c.tag];
  if (i >= 0) { x4[i].w = (R)c.type; v4[i].w = (R)c.mass; }
}

// Charges by tag (the array of the Coulomb term, chem_nb_coulomb): launched behind k_react_apply / k_apply_props only while a
// Coulomb pair is registered, so that those two kernels and their argument blocks stay what they were.  Every rank of a
// decomposition holds all charges and applies every event.  A reaction sets the charge wherever it names a new type.
struct ReactQ { int new_type_1, new_type_2; double new_q_1, new_q_2; };
struct ReactQSet { ReactQ r[CHEM_MAX_REACTIONS]; };
template <typename R>
__global__ void k_react_apply_q(int nc, const Candidate* __restrict__ c, const int* __restrict__ st, ReactQSet rqs, R* __restrict__ qtag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nc || st[k] != 2) return;
  const Candidate cd = c[k];
  const ReactQ rq = rqs.r[cd.r];
  if (rq.new_type_1 >= 0) qtag[cd.a] = (R)rq.new_q_1;
  if (rq.new_type_2 >= 0) qtag[cd.b] = (R)rq.new_q_2;
}
template <typename R>
__global__ void k_apply_props_q(int nchg, const PropChangeDev* __restrict__ chg, R* __restrict__ qtag) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nchg) qtag[chg[k].tag] = (R)chg[k].q;
}

// ---- dissociation reactions (chem_dissociation_add; rule set in include/chem_mi355.h) ----------------------------
// One lane per flat tuple entry (the arrays the bonded CSR is built from).  Entries of a scanned pair list go
// tags -> rtag -> positions (decoded exactly in the fp32 build), state by tag, type from x4.w; the fp64 distance is the
// association scan's (minimgD + dist2_unfused).  Broken bonds are compacted with a wave ballot and one atomic per wave;
// the order the atomics give is arbitrary, the host sorts the records by (list, flat index) = list order.  A record is a
// Candidate: a / b the role-1 / role-2 tags, r the dissociation's own index, h the flat index, d2 = r^2.  The buffer
// holds one record per flat entry, so it cannot overflow.
struct DissDev { int type_1, type_2, min1, max1, min2, max2, list, active, pub, pad; double cut2, prob; };
struct DissSet { int n, pad; unsigned long long seed, step; DissDev r[CHEM_MAX_REACTIONS]; };
template <typename R>
__global__ __launch_bounds__(256) void k_diss_scan(int ne, const int4* __restrict__ fent, const int* __restrict__ flist,
                                                   const Vec4<R>* __restrict__ x4, const int* __restrict__ rtag, int npart,
                                                   const int* __restrict__ state, BoxD box, DissSet ds,
                                                   Candidate* __restrict__ rec, int rec_cap, int* __restrict__ rec_count) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = false;
  Candidate c{0, 0, 0, 0u, 0.0};
  if (e < ne) {
    const int li = flist[e];
    bool scanned = false;
    for (int q = 0; q < ds.n; ++q) scanned |= ds.r[q].active && ds.r[q].list == li;
    const int4 tt = fent[e];
    const int ta = tt.x, tb = tt.y;
    if (scanned && ta >= 0 && tb >= 0 && ta < npart && tb < npart) {
      const int ia = rtag[ta], ib = rtag[tb];
      if (ia >= 0 && ib >= 0) {
        const Vec4<R> xa = x4[ia], xb = x4[ib];
        const int tya = (int)xa.w, tyb = (int)xb.w, sa = state[ta], sb = state[tb];
        const int lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
        const D3 d = lo == ta ? minimgD(box, posD<R>(xa, box) - posD<R>(xb, box)) : minimgD(box, posD<R>(xb, box) - posD<R>(xa, box));
        const double d2 = dist2_unfused(d);
        for (int q = 0; q < ds.n && !hit; ++q) {
          const DissDev& D = ds.r[q];
          if (!D.active || D.list != li) continue;
          const bool fwd = tya == D.type_1 && tyb == D.type_2, rev = tyb == D.type_1 && tya == D.type_2;
          if (!fwd && !rev) continue;
          const bool a_first = fwd && rev ? ta < tb : fwd;     // equal types: the lower tag takes role 1
          const int s1 = a_first ? sa : sb, s2 = a_first ? sb : sa;
          if (!(s1 >= D.min1 && s1 < D.max1 && s2 >= D.min2 && s2 < D.max2)) continue;
          bool brk = D.cut2 > 0.0 && d2 >= D.cut2;
          if (!brk && D.prob > 0.0) {
            uint32_t rr[4];
            chem_philox::dissociation_draw(ds.seed, ds.step, (uint32_t)lo, (uint32_t)hi, (uint32_t)D.pub, rr);
            brk = chem_philox::u01(rr[0]) < D.prob;
          }
          if (brk) { hit = true; c = Candidate{a_first ? ta : tb, a_first ? tb : ta, q, (unsigned int)e, d2}; }
        }
      }
    }
  }
  const unsigned long long m = __ballot(hit);
  if (!m) return;
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane_id() == leader) base = atomicAdd(rec_count, __popcll(m));
  base = __shfl(base, leader);
  if (!hit) return;
  const int pos = base + __popcll(m & lanemask_lt());
  if (pos < rec_cap) rec[pos] = c;
}

// =======================================================================================
// Per-tag CSR tables (bonded entries, exclusions) built ON THE DEVICE from flat, append-only arrays.
// A bond-forming reaction step used to rebuild both tables on the host (a pass over all 10^6 rows, ~14 MB of
// uploads, 3-4 ms); now the host uploads only the NEW tuples / pairs and four small kernels rebuild the CSR:
// count (atomics by tag) -> exclusive scan -> fill (atomic cursor) -> canonical order inside every row
// (one thread per tag, insertion sort: rows hold a handful of entries).  The row order is a pure function of
// the flat arrays, so the tables -- and with them the force sums -- are run-to-run deterministic.
// =======================================================================================
// exclusive scan of n counters -> start[0..n] in three launches (4096 counters per block; block totals scanned by one
// block; offsets added); the counters are cleared on the way (they become the fill cursors)
constexpr int kScanItems = 4096;
__global__ __launch_bounds__(1024) void k_scan_local(int n, int* __restrict__ cnt, int* __restrict__ start, int* __restrict__ btot) {
  __shared__ int ws[16];
  const int i0 = blockIdx.x * kScanItems + threadIdx.x * 4;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] = 0; if (i0 + k < n) { v[k] = cnt[i0 + k]; cnt[i0 + k] = 0; } }
  const int sum = v[0] + v[1] + v[2] + v[3];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  if (lane == 63) ws[w] = incl;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { if (k < w) off += ws[k]; tot += ws[k]; }
  int run = off + incl - sum;
#pragma unroll
  for (int k = 0; k < 4; ++k) { if (i0 + k < n) start[i0 + k] = run; run += v[k]; }
  if (threadIdx.x == 0) btot[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_scan_blocks(int nb, int* __restrict__ btot, int n, int* __restrict__ start) {
  __shared__ int ws[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? btot[i] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < 16; ++k) { if (k < w) off += ws[k]; tot += ws[k]; }
    if (i < nb) btot[i] = carry_s + off + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) carry_s += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) start[n] = carry_s;
}
__global__ __launch_bounds__(1024) void k_scan_add(int n, const int* __restrict__ btot, int* __restrict__ start) {
  const int off = btot[blockIdx.x];
  if (off == 0) return;
  const int i0 = blockIdx.x * kScanItems + threadIdx.x * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) if (i0 + k < n) start[i0 + k] += off;
}

// ---- exclusions: flat pairs (a, b) -> symmetric CSR, rows ascending (= HostTopology::build_excl) ----
__global__ void k_ex_count(int m, const int2* __restrict__ pairs, int* __restrict__ cnt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int2 p = pairs[k];
  atomicAdd(&cnt[p.x], 1); atomicAdd(&cnt[p.y], 1);
}
__global__ void k_ex_fill(int m, const int2* __restrict__ pairs, const int* __restrict__ start, int* __restrict__ cursor, int* __restrict__ list) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int2 p = pairs[k];
  list[start[p.x] + atomicAdd(&cursor[p.x], 1)] = p.y;
  list[start[p.y] + atomicAdd(&cursor[p.y], 1)] = p.x;
}
__global__ void k_ex_sort(int n, const int* __restrict__ start, int* __restrict__ cursor, int* __restrict__ list) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  cursor[t] = 0;
  const int s = start[t], e = start[t + 1];
  for (int i = s + 1; i < e; ++i) {
    const int v = list[i];
    int j = i - 1;
    while (j >= s && list[j] > v) { list[j + 1] = list[j]; --j; }
    list[j + 1] = v;
  }
}

// ---- bonded entries: flat tuples (tags t0..t3, list index) -> per-tag CSR of BondedEntry ----
// parameter slot of a tuple: plain lists have one slot, typed lists one per registered type tuple (matched forwards
// or backwards against the CURRENT particle types); -1 = no parameters for these types (tuple skipped, as
// HostTopology::build_bonded does)
struct SlotKey { int list, t0, t1, t2, t3, by_types, arity, pad; };
template <typename R>
__global__ void k_bt_count(int ne, const int4* __restrict__ fent, const int* __restrict__ flist, int nslot, const SlotKey* __restrict__ keys,
                           const Vec4<R>* __restrict__ x4, const int* __restrict__ rtag, const int* __restrict__ type_by_tag,
                           int* __restrict__ eslot, int* __restrict__ cnt) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int4 tt = fent[e];
  const int li = flist[e];
  const int tg[4] = {tt.x, tt.y, tt.z, tt.w};
  int slot = -1, arity = 2, pad = 0;
  for (int s = 0; s < nslot && slot < 0; ++s) {
    const SlotKey k = keys[s];
    if (k.list != li) continue;      // (li = -1: the second flat record of a hybrid triple or quadruple, read by k_bt_fill)
    arity = k.arity; pad = k.pad;
    if (!k.by_types) { slot = s; break; }
    int ty[4] = {-1, -1, -1, -1};
    for (int q = 0; q < k.arity; ++q) {
      if (type_by_tag) ty[q] = type_by_tag[tg[q]];
      else { const int i = rtag[tg[q]]; ty[q] = i >= 0 ? (int)x4[i].w : -1; }
    }
    const int kt[4] = {k.t0, k.t1, k.t2, k.t3};
    bool fwd = true, rev = true;
    for (int q = 0; q < k.arity; ++q) { fwd &= ty[q] == kt[q]; rev &= ty[k.arity - 1 - q] == kt[q]; }
    if (fwd || rev) slot = s;
  }
  // a hybrid triple or quadruple without its second flat record has no birth step: it is dropped like a tuple without
  // parameters (the host always writes both records), so k_bt_fill reads fent[e + 1] of what is left without a fallback value
  if (slot >= 0 && pad && arity > 2 && !(e + 1 < ne && flist[e + 1] == -1)) slot = -1;
  eslot[e] = slot;
  if (slot < 0) return;
  const int w = (arity == 4 || (pad && arity == 3)) ? 2 : 1;
  for (int q = 0; q < arity; ++q) atomicAdd(&cnt[tg[q]], w);
}
__global__ void k_bt_fill(int ne, const int4* __restrict__ fent, const int* __restrict__ eslot, const SlotKey* __restrict__ keys,
                          const int* __restrict__ start, int* __restrict__ cursor, BondedEntry* __restrict__ bent, int* __restrict__ bkey) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int slot = eslot[e];
  if (slot < 0) return;
  const int4 tt = fent[e];
  const int arity = keys[slot].arity;
  const bool hyt = keys[slot].pad && arity > 2;      // hybrid triple / quadruple: ~birth step in the next flat record (x), two entries
  const int w = (arity == 4 || hyt) ? 2 : 1;
  const int zb = hyt ? fent[e + 1].x : 0;      // (k_bt_count has seen that record)
  const int tg[4] = {tt.x, tt.y, tt.z, tt.w};
  for (int q = 0; q < arity; ++q) {
    const int pos = start[tg[q]] + atomicAdd(&cursor[tg[q]], w);
    bent[pos] = BondedEntry{tt.x, tt.y, (arity > 2 || keys[slot].pad) ? tt.z : 0, bonded_meta(slot, q)};      // (pad: hybrid pair list, z = ~birth step)
    bkey[pos] = 2 * e;
    if (w == 2) { bent[pos + 1] = BondedEntry{arity == 4 ? tt.w : 0, 0, zb, 0}; bkey[pos + 1] = 2 * e + 1; }
  }
}
// rows in flat-array order (key = 2 e + half); counts[0] = tags that own entries
__global__ void k_bt_sort(int n, const int* __restrict__ start, int* __restrict__ cursor, BondedEntry* __restrict__ bent, int* __restrict__ bkey, int* __restrict__ counts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  cursor[t] = 0;
  const int s = start[t], e = start[t + 1];
  if (e > s) atomicAdd(&counts[0], 1);
  for (int i = s + 1; i < e; ++i) {
    const int kv = bkey[i]; const BondedEntry bv = bent[i];
    int j = i - 1;
    while (j >= s && bkey[j] > kv) { bkey[j + 1] = bkey[j]; bent[j + 1] = bent[j]; --j; }
    bkey[j + 1] = kv; bent[j + 1] = bv;
  }
}

template <typename T> __global__ void k_fill(T* p, T v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- region rules (chem_region_add; rule set in include/chem_mi355.h, selection in chem_region_host.hpp) -------------------
// k_region_scan: a launch of its own behind the second half kick of a step on which an enabled rule is due.  One thread per
// particle: one 16/32-byte load of (x, y, z, type), an exit on the type mask of the due rules, then the fp64 box test of every
// due rule on the decoded, folded position -- the expressions of chem_get_state(CHEM_STATE_POS), without FMA contraction.
// A particle that is a candidate of at least one due rule is compacted (wave ballot, one atomic per wave) as (tag, type, bits
// of the boxes it is in); candidates and mode-1 acceptances are counted per rule.  The last workgroup to finish knows the
// counts: if no rule changes anything it clears them and the run goes on, no host involved; otherwise it stops the
// asynchronous run (DevCtl::halt = 4: "step halt_step is complete, nothing of the next one has happened"), every later launch
// leaves at once, and the host applies the selection over the records and resumes.
struct RegionDev { double lo[3], hi[3], value; unsigned long long seed; int target_type, mode, num, rule; };
struct RegionSet { int n, par, gen; unsigned int type_mask; unsigned long long step; RegionDev r[kRegionMaxRules]; };
struct RegionOut { int nrec, done, ncand[kRegionMaxRules], nacc[kRegionMaxRules]; };
__device__ __forceinline__ double region_coord(float c, double qs, double qh) {
#pragma clang fp contract(off)
  const double p = (double)qbits(c) * qs;
  return p + qh;
}
__device__ __forceinline__ double region_coord(double c, double, double) { return c; }
template <typename R>
__global__ __launch_bounds__(256) void k_region_scan(int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag, BoxD box, RegionSet rs,
                                                     RegionCand* __restrict__ rec, int rec_cap, RegionOut* __restrict__ out, DevCtl* ctl, IdleHint* hint) {
  if (ctl->halt) return;   // (a stopped run: the step this launch belongs to is redone)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int candm = 0, accm = 0;
  RegionCand c{0, 0, 0u, 0u};
  if (i < n) {
    const Vec4<R> p = x4[i];
    const int ty = (int)p.w;
    if ((rs.type_mask >> (ty & 31)) & 1u) {
      const double x = region_fold(region_coord(p.x, box.qs[0], box.qh[0]), box.L[0]), y = region_fold(region_coord(p.y, box.qs[1], box.qh[1]), box.L[1]),
                   z = region_fold(region_coord(p.z, box.qs[2], box.qh[2]), box.L[2]);
      const int tg = tag[i];
      for (int k = 0; k < rs.n; ++k) {
        const RegionDev& D = rs.r[k];
        if (!region_inside(D.lo, D.hi, x, y, z)) continue;
        c.inbox |= 1u << D.rule;
        if (D.target_type != ty) continue;
        candm |= 1u << k;
        if (D.mode == kRegionProb) {
          uint32_t rr[4];
          chem_philox::region_draw(D.seed, rs.step, (uint32_t)tg, (uint32_t)D.rule, rr);
          if (chem_philox::u01(rr[1]) < D.value) accm |= 1u << k;
        }
      }
      c.tag = tg; c.type = ty;
    }
  }
  const unsigned long long m = __ballot(candm != 0);
  if (m) {
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane_id() == leader) base = atomicAdd(&out->nrec, __popcll(m));
    base = __shfl(base, leader);
    if (candm) { const int pos = base + __popcll(m & lanemask_lt()); if (pos < rec_cap) rec[pos] = c; }
    for (int k = 0; k < rs.n; ++k) {
      const int nc = __popcll(__ballot((candm >> k) & 1u)), na = __popcll(__ballot((accm >> k) & 1u));
      if (lane_id() == leader) { if (nc) atomicAdd(&out->ncand[k], nc); if (na) atomicAdd(&out->nacc[k], na); }
    }
  }
  __shared__ int last;
  __syncthreads();
  if (threadIdx.x == 0) { __threadfence(); last = atomicAdd(&out->done, 1) == (int)gridDim.x - 1; }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __threadfence();
  bool change = false;
  for (int k = 0; k < rs.n; ++k)
    change |= region_quota(rs.r[k].mode, rs.r[k].value, rs.r[k].num, atomicAdd(&out->ncand[k], 0), atomicAdd(&out->nacc[k], 0)) > 0;
  if (change) {
    ctl->halt_step = (long long)rs.step; ctl->halt_par = rs.par; ctl->halt = 4;
    if (hint) { volatile IdleHint* h = hint; h->halted = rs.gen; }
  } else {
    out->nrec = 0;
    for (int k = 0; k < rs.n; ++k) { out->ncand[k] = 0; out->nacc[k] = 0; }
  }
  out->done = 0;
}

// the resets of a region rule, behind k_apply_props: v := 0 (flag 1), stored force := 0 (flag 2), exactly
struct RegionReset { int tag, flags; };
template <typename R>
__global__ void k_region_reset(int nchg, const RegionReset* __restrict__ chg, const int* __restrict__ rtag, Vec4<R>* __restrict__ v4, Vec4<R>* __restrict__ f4) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nchg) return;
  const int i = rtag[chg[k].tag];
  if (i < 0) return;
  if (chg[k].flags & 1) { Vec4<R> v = v4[i]; v.x = v.y = v.z = (R)0; v4[i] = v; }
  if (chg[k].flags & 2) { Vec4<R> f = f4[i]; f.x = f.y = f.z = (R)0; f4[i] = f; }
}

// =======================================================================================
// Radial distribution functions (chem_rdf_*; rule set: include/chem_mi355.h, host rules and launch plan: chem_rdf_host.hpp).
// Every unordered pair of distinct particles inside r_max is counted once, from its lower tag, excluded pairs included; the
// distance is the reaction scan's (posD, minimgD, dist2_unfused), the bin is rdf_bin's.  The histogram of a workgroup is u32
// words in LDS (behind whatever the kernel stages), bumped with LDS atomics; at the end the workgroup adds its non-zero words to
// the u64 accumulators with global atomics whose result nobody reads.  The kernels only read the particle data, and a launch of
// a stopped run (DevCtl::halt) leaves at once like every other launch of the step: that step is redone and sampled then.
// =======================================================================================
__device__ __forceinline__ void rdf_bump(unsigned int* const hist, const RdfArgs& a, unsigned int m, const int part, const int k) {
  while (m) {
    const int s = __ffs((int)m) - 1;
    m &= m - 1;
    atomicAdd(&hist[(s * a.parts + part) * a.nbins + k], 1u);
  }
}
__device__ __forceinline__ void rdf_flush(const unsigned int* const hist, const int nh, unsigned long long* __restrict__ acc) {
  for (int k = threadIdx.x; k < nh; k += blockDim.x) {
    const unsigned int v = hist[k];
    if (v) atomicAdd(&acc[kRdfHead + k], (unsigned long long)v);
  }
}

// Tiles (fused and unfused rebuild): k_react_scan_tiles's traversal -- the stencil of a tile staged in LDS with the current
// positions, the x-window of every stencil row widened by `slack` for the tables of the last rebuild, the fp32 pre-test against
// the largest radius with its 1e-3 margin -- without the role, exclusion, state and label filters.  Persistent: the grid is a
// small multiple of the compute units (rdf_plan), a workgroup loops over tiles and keeps its histogram until the end.
// The traversal is a COPY of k_react_scan_tiles's, not shared code: keep the two in step by hand.
template <typename R, int BS>
__global__ __launch_bounds__(BS) void k_rdf_tiles(int ntiles, int CAP, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag,
                                                  const TileLDS<R>* __restrict__ desc, const int* __restrict__ mol_id, BoxD box, RdfArgs a,
                                                  int hist_off, unsigned long long* __restrict__ acc, const DevCtl* __restrict__ ctl, R slack) {
  if (ctl->halt) return;
  __shared__ TileLDS<R> T;
  __shared__ unsigned char smask[kMaxTypes * kMaxTypes];
  CHEM_DYN_LDS(R);
  unsigned int* const hist = reinterpret_cast<unsigned int*>(chem_dyn_lds + hist_off);
  const int nh = a.nbins * a.nsel * a.parts;
  for (int k = threadIdx.x; k < nh; k += BS) hist[k] = 0u;
  for (int k = threadIdx.x; k < kMaxTypes * kMaxTypes; k += BS) smask[k] = a.mask[k / kMaxTypes][k % kMaxTypes];
  __syncthreads();
  R maxcut2 = (R)rdf_edge2(a.nbins, a.dr);
  maxcut2 *= (R)1.001;   // the staged positions carry the periodic shift: one more rounding than the global ones
  for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    const int tile = xcd_remap(vb, ntiles);
    __syncthreads();
    tile_load_desc<R>(T, desc, tile);
    __syncthreads();
    tile_fill<R, BS, true>(T, sx, CAP, x4, 1);
    __syncthreads();
    const int hx = T.geom[0], total = T.geom[3], nhome = T.geom[4];
    for (int q = threadIdx.x; q < nhome; q += BS) {
      int sgi = 0;
#pragma unroll
      for (int k = 1; k < NHSEG; ++k) sgi += (q >= T.hoff[k]) ? 1 : 0;
      const int inrun = q - T.hoff[sgi];
      const int p = T.hstart[sgi] + inrun;
      const int ly = sgi % HY, lz = sgi / HY;
      const int hr = (lz + 1) * SY + (ly + 1);
      const int eh = inrun + T.celloff[hr][1];
      int lx = 0;
      for (int k = 2; k <= hx; ++k) lx += (eh >= T.celloff[hr][k]) ? 1 : 0;
      const int sself = T.rowoff[hr] + eh;
      if (sself >= CAP) continue;                             // (a tile beyond its capacity: stage_overflow is raised where the tables are built)
      const Vec4<R> xi = sx[sself];
      const int tgi = tag[p];
      const Vec4<R> xgi = x4[p];
      const int ti = (int)xgi.w & (kMaxTypes - 1);
      const int mi = a.parts == 2 ? mol_id[tgi] : 0;
      const R rmax = sqrt_r(maxcut2), weps = T.clen[0] * (R)2e-4;
      auto suboff = [&](int r, int f, bool lower) {
        const int k = f >> 2, j = f & 3;
        const int base = T.celloff[r][k];
        if (j == 0) return base;
        const int pk = T.cellsub[r][k];
        if (pk < 0) return lower ? base : T.celloff[r][k + 1];
        return base + ((pk >> (8 * (j - 1))) & 0xff);
      };
#pragma unroll 1
      for (int dzy = 0; dzy < 9; ++dzy) {
        const int dz = dzy / 3, dy = dzy - 3 * dz;
        const int r = (lz + dz) * SY + (ly + dy);
        const R ylo = ((R)(ly + 1) - (R)kRefCells) * T.clen[1], zlo = ((R)(lz + 1) - (R)kRefCells) * T.clen[2];   // (staged coordinates are relative to T.org)
        R ddy = dy == 0 ? xi.y - ylo : (dy == 2 ? ylo + T.clen[1] - xi.y : (R)0);
        R ddz = dz == 0 ? xi.z - zlo : (dz == 2 ? zlo + T.clen[2] - xi.z : (R)0);
        ddy -= slack + weps; ddz -= slack + weps;
        ddy = ddy > 0 ? ddy : (R)0; ddz = ddz > 0 ? ddz : (R)0;
        const R w2 = rmax * rmax - ddy * ddy - ddz * ddz;
        if (w2 < (R)0) continue;
        const R ws = (sqrt_r(w2) + slack + weps) * T.subinv, sxi = (xi.x + (R)kRefCells * T.clen[0]) * T.subinv;
        int f_lo = (int)(sxi - ws), f_hi = (int)(sxi + ws);
        f_lo = f_lo > lx * NSUB ? f_lo : lx * NSUB;
        f_hi = f_hi < (lx + 3) * NSUB - 1 ? f_hi : (lx + 3) * NSUB - 1;
        const int s0 = T.rowoff[r] + suboff(r, f_lo, true);
        int b = T.rowoff[r] + suboff(r, f_hi + 1, false);
        b = b < total ? b : total;
        for (int sl0 = s0; sl0 < b; sl0 += 4) {
          Vec4<R> xq[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) xq[u] = lds_gather4<R>(sx, sl0 + u < b ? sl0 + u : total);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int sl = sl0 + u;
            const Vec4<R> xj = xq[u];
            const R dx = xi.x - xj.x, dy_ = xi.y - xj.y, dz_ = xi.z - xj.z;
            if (dx * dx + dy_ * dy_ + dz_ * dz_ > maxcut2 || sl == sself || sl >= b) continue;
            const int wj = real_as_idx(xj.w);
            const unsigned int m = smask[ti * kMaxTypes + (wj & (kMaxTypes - 1))];
            if (!m) continue;
            const int j = wj >> 5;
            const int tgj = tag[j];
            if (!(tgi < tgj)) continue;          // every pair once, from its lower tag
            const D3 d = minimgD(box, posD<R>(xgi, box) - posD<R>(x4[j], box));
            const int k = rdf_bin(dist2_unfused(d), a.dr, a.inv_dr, a.nbins);
            if (k < 0) continue;
            rdf_bump(hist, a, m, a.parts == 2 && mol_id[tgj] != mi ? 1 : 0, k);
          }
        }
      }
    }
  }
  __syncthreads();
  rdf_flush(hist, nh, acc);
}

// Per-cell and brute-force lists (single domain): all pairs.  These paths exist where the cell grid is too small for tiles, so a
// particle's partners inside r_max are a large part of the system anyway; a workgroup stages kRdfChunk particles at a time
// (decoded position, tag, type, molecule) and every thread tests its own particle against them.
template <typename R>
__global__ __launch_bounds__(kRdfChunk) void k_rdf_all(int n, const Vec4<R>* __restrict__ x4, const int* __restrict__ tag, const int* __restrict__ mol_id,
                                                       BoxD box, RdfArgs a, int hist_off, unsigned long long* __restrict__ acc, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  __shared__ unsigned char smask[kMaxTypes * kMaxTypes];
  extern __shared__ __attribute__((aligned(16))) unsigned char chem_dyn_lds[];
  double* const cx = reinterpret_cast<double*>(chem_dyn_lds);
  int* const ci = reinterpret_cast<int*>(chem_dyn_lds + (size_t)kRdfChunk * 3 * sizeof(double));   // tag, type, molecule
  unsigned int* const hist = reinterpret_cast<unsigned int*>(chem_dyn_lds + hist_off);
  const int nh = a.nbins * a.nsel * a.parts, t = threadIdx.x;
  for (int k = t; k < nh; k += kRdfChunk) hist[k] = 0u;
  for (int k = t; k < kMaxTypes * kMaxTypes; k += kRdfChunk) smask[k] = a.mask[k / kMaxTypes][k % kMaxTypes];
  for (int i0 = blockIdx.x * kRdfChunk; i0 < n; i0 += gridDim.x * kRdfChunk) {
    const int i = i0 + t;
    const bool live = i < n;
    D3 pi = {0, 0, 0}; int tgi = 0, ti = 0, mi = 0;
    if (live) { const Vec4<R> xi = x4[i]; pi = posD<R>(xi, box); ti = (int)xi.w & (kMaxTypes - 1); tgi = tag[i]; mi = a.parts == 2 ? mol_id[tgi] : 0; }
    for (int j0 = 0; j0 < n; j0 += kRdfChunk) {
      __syncthreads();
      if (j0 + t < n) {
        const Vec4<R> xj = x4[j0 + t];
        const D3 pj = posD<R>(xj, box);
        const int tgj = tag[j0 + t];
        cx[3 * t] = pj.x; cx[3 * t + 1] = pj.y; cx[3 * t + 2] = pj.z;
        ci[3 * t] = tgj; ci[3 * t + 1] = (int)xj.w & (kMaxTypes - 1); ci[3 * t + 2] = a.parts == 2 ? mol_id[tgj] : 0;
      }
      __syncthreads();
      if (!live) continue;
      const int nj = n - j0 < kRdfChunk ? n - j0 : kRdfChunk;
      for (int jj = 0; jj < nj; ++jj) {
        if (!(tgi < ci[3 * jj])) continue;
        const unsigned int m = smask[ti * kMaxTypes + ci[3 * jj + 1]];
        if (!m) continue;
        const D3 pj = {cx[3 * jj], cx[3 * jj + 1], cx[3 * jj + 2]};
        const int k = rdf_bin(dist2_unfused(minimgD(box, pi - pj)), a.dr, a.inv_dr, a.nbins);
        if (k < 0) continue;
        rdf_bump(hist, a, m, a.parts == 2 && ci[3 * jj + 2] != mi ? 1 : 0, k);
      }
    }
  }
  __syncthreads();
  rdf_flush(hist, nh, acc);
}

// Frame bookkeeping behind the pair pass (single domain; on slabs the host keeps the books, see CtxT::rdf_launch).
// k_rdf_count: the type counts of the owned particles, many workgroups, one global atomic per type and workgroup into the words
// at kRdfTypes.  k_rdf_frame: one wave reads and clears them, computes M per selector (rdf_norm_pairs) and bumps frames,
// pairs[s] += M, density[s] += M / V in frame order.  V comes in by value.
template <typename R>
__global__ __launch_bounds__(256) void k_rdf_count(int i0, int n, const Vec4<R>* __restrict__ x4, unsigned long long* __restrict__ acc, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  __shared__ int cnt[kMaxTypes];
  const int t = threadIdx.x;
  if (t < kMaxTypes) cnt[t] = 0;
  __syncthreads();
  int mine[kMaxTypes];
#pragma unroll
  for (int u = 0; u < kMaxTypes; ++u) mine[u] = 0;
  for (int i = blockIdx.x * 256 + t; i < n; i += gridDim.x * 256) {
    const int ty = (int)x4[i0 + i].w & (kMaxTypes - 1);
#pragma unroll
    for (int u = 0; u < kMaxTypes; ++u) mine[u] += ty == u ? 1 : 0;
  }
#pragma unroll
  for (int u = 0; u < kMaxTypes; ++u) {
    int v = mine[u];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane_id() == 0 && v) atomicAdd(&cnt[u], v);
  }
  __syncthreads();
  if (t < kMaxTypes && cnt[t]) atomicAdd(&acc[kRdfTypes + t], (unsigned long long)cnt[t]);
}
__global__ __launch_bounds__(64) void k_rdf_frame(RdfArgs a, double V, unsigned long long* __restrict__ acc, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  __shared__ unsigned char smask[kMaxTypes][kMaxTypes];
  __shared__ long long c[kMaxTypes];
  const int t = threadIdx.x;
  for (int k = t; k < kMaxTypes * kMaxTypes; k += 64) smask[k / kMaxTypes][k % kMaxTypes] = a.mask[k / kMaxTypes][k % kMaxTypes];
  if (t < kMaxTypes) { c[t] = (long long)acc[kRdfTypes + t]; acc[kRdfTypes + t] = 0ull; }
  __syncthreads();
  if (t == 0) {
    acc[kRdfFrames] += 1ull;
    for (int s = 0; s < a.nsel; ++s) {
      const unsigned long long M = rdf_norm_pairs(smask, s, c);
      acc[kRdfPairs + s] += M;
      acc[kRdfDensity + s] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)acc[kRdfDensity + s]) + (double)M / V);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------------
// Static structure factor (chem_sq_*; rule set: include/chem_mi355.h, enumeration, classes and launch plan: chem_sq_host.hpp).
// All fp64 in both builds, no floating-point atomics: every sum has one owner and a fixed order.
//
// k_sq_walk: workgroup (blockIdx.x, blockIdx.y) owns the kSqQBlock wave vectors from blockIdx.x * kSqQBlock (kSqVpl per lane, in
// registers for the whole launch) and the particle slots [blockIdx.y * per, min(n, (blockIdx.y + 1) * per)) of the range x4[i0 ..
// i0 + n).  It stages kSqChunk particles at a time: thread (axis, j) decodes particle j, takes one sincospi of 2 f_a and writes
// e_a(m) = exp(-i 2 pi m f_a), m = 0..nmax, by the recurrence e(m) = e(m - 1) e(1); negative m is the conjugate.  Then every lane
// walks the staged particles in slot order: the product of its three table entries, added to the sums of the classes the particle
// belongs to (the class mask is the same for the whole wave, so that is a scalar branch).  A lane's vectors are consecutive in k,
// i.e. mostly the same (nx, ny) and consecutive nz: two of the three LDS reads are broadcasts.  part[((super * ncls + c) * nvec +
// k) * 2 ..] = the partial of (class c, vector k) over the super-chunk.
template <typename R>
__global__ __launch_bounds__(kSqBlock) void k_sq_walk(int i0, int n, const Vec4<R>* __restrict__ x4, BoxD box, SqArgs a, int per, double* __restrict__ part,
                                                      const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char chem_dyn_lds[];
  __shared__ int smask[kSqChunk];
  double2* const tab = reinterpret_cast<double2*>(chem_dyn_lds);      // [axis][particle][m]
  const int t = threadIdx.x, M1 = a.nmax + 1;
  const int lo = blockIdx.y * per, hi = n - lo < per ? n : lo + per;
  int ox[kSqVpl], oy[kSqVpl], oz[kSqVpl]; double sy[kSqVpl], sz[kSqVpl];
  double re[kSqVpl][kSqMaxClasses], im[kSqVpl][kSqMaxClasses];
#pragma unroll
  for (int v = 0; v < kSqVpl; ++v) {
    const long long k = (long long)blockIdx.x * kSqQBlock + v * kSqBlock + t;
    int nx = 0, ny = 0, nz = 0;
    if (k < a.nvec) sq_vec(k, a.nmax, nx, ny, nz);
    ox[v] = nx; oy[v] = kSqChunk * M1 + (ny < 0 ? -ny : ny); oz[v] = 2 * kSqChunk * M1 + (nz < 0 ? -nz : nz);
    sy[v] = ny < 0 ? -1.0 : 1.0; sz[v] = nz < 0 ? -1.0 : 1.0;
#pragma unroll
    for (int c = 0; c < kSqMaxClasses; ++c) { re[v][c] = 0.0; im[v][c] = 0.0; }
  }
  for (int s0 = lo; s0 < hi; s0 += kSqChunk) {
    __syncthreads();
    if (t < 3 * kSqChunk) {
      const int axis = t / kSqChunk, j = t % kSqChunk;
      if (s0 + j < hi) {
        const Vec4<R> xq = x4[i0 + s0 + j];
        const D3 p = posD<R>(xq, box);
        const double f = (axis == 0 ? p.x : axis == 1 ? p.y : p.z) * box.invL[axis];
        double sn, cs;
        ::sincospi(2.0 * f, &sn, &cs);
        double2* const e = tab + (axis * kSqChunk + j) * M1;
        double2 w = {1.0, 0.0};
        e[0] = w;
        for (int m = 1; m <= a.nmax; ++m) {
          const double wr = w.x * cs + w.y * sn, wi = w.y * cs - w.x * sn;      // w * (cs - i sn)
          w.x = wr; w.y = wi;
          e[m] = w;
        }
        if (axis == 0) smask[j] = a.tmask[(int)xq.w & (kMaxTypes - 1)];
      }
    }
    __syncthreads();
    const int nj = hi - s0 < kSqChunk ? hi - s0 : kSqChunk;
    for (int j = 0; j < nj; ++j) {
      const int cm = __builtin_amdgcn_readfirstlane(smask[j]);
      const double2* const e = tab + j * M1;
#pragma unroll
      for (int v = 0; v < kSqVpl; ++v) {
        const double2 ex = e[ox[v]], ey = e[oy[v]], ez = e[oz[v]];
        const double eyi = ey.y * sy[v], ezi = ez.y * sz[v];
        const double qr = ex.x * ey.x - ex.y * eyi, qi = ex.x * eyi + ex.y * ey.x;
        const double pr = qr * ez.x - qi * ezi, pi = qr * ezi + qi * ez.x;
#pragma unroll
        for (int c = 0; c < kSqMaxClasses; ++c)
          if ((cm >> c) & 1) { re[v][c] += pr; im[v][c] += pi; }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < kSqVpl; ++v) {
    const long long k = (long long)blockIdx.x * kSqQBlock + v * kSqBlock + t;
    if (k >= a.nvec) continue;
#pragma unroll
    for (int c = 0; c < kSqMaxClasses; ++c)
      if (c < a.ncls) {
        double2* const o = reinterpret_cast<double2*>(part) + ((size_t)blockIdx.y * a.ncls + c) * a.nvec + k;
        *o = double2{re[v][c], im[v][c]};
      }
  }
}

// rho[(c * nvec + k) * 2 ..] = the partials of (class c, vector k) summed over the super-chunks in index order
__global__ __launch_bounds__(256) void k_sq_reduce(SqArgs a, int nsuper, const double* __restrict__ part, double* __restrict__ rho, const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  const size_t w = (size_t)a.ncls * a.nvec, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w) return;
  const double2* const p = reinterpret_cast<const double2*>(part);
  double2 s = {0.0, 0.0};
  for (int u = 0; u < nsuper; ++u) { const double2 q = p[(size_t)u * w + i]; s.x += q.x; s.y += q.y; }
  reinterpret_cast<double2*>(rho)[i] = s;
}

// sums[s][k] += Re(rho_A(k) conj rho_B(k)) from the (global) rho.  books != 0 (single domain): thread 0 of workgroup 0 also keeps
// the books of the frame -- frames, na, nb from the type counts k_rdf_count left at kSqTypes (cleared again), box_sum; on slabs the
// host keeps them (CtxT::sq_launch).
__global__ __launch_bounds__(256) void k_sq_accum(SqArgs a, BoxD box, int books, const double* __restrict__ rho, double* __restrict__ acc,
                                                  const DevCtl* __restrict__ ctl) {
  if (ctl->halt) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < a.nvec) {
    const double2* const r = reinterpret_cast<const double2*>(rho);
    for (int s = 0; s < a.nsel; ++s) {
      const double2 ra = r[(size_t)a.sel_a[s] * a.nvec + k], rb = r[(size_t)a.sel_b[s] * a.nvec + k];
      acc[kSqHead + (size_t)s * a.nvec + k] += ra.x * rb.x + ra.y * rb.y;
    }
  }
  if (books && blockIdx.x == 0 && threadIdx.x == 0) {
    unsigned long long* const tc = reinterpret_cast<unsigned long long*>(acc) + kSqTypes;
    long long cnt[kMaxTypes];
    for (int u = 0; u < kMaxTypes; ++u) { cnt[u] = (long long)tc[u]; tc[u] = 0ull; }
    acc[kSqFrames] += 1.0;
    for (int s = 0; s < a.nsel; ++s) {
      acc[kSqNa + s] += (double)sq_class_count(a, a.sel_a[s], cnt);
      acc[kSqNb + s] += (double)sq_class_count(a, a.sel_b[s], cnt);
    }
    for (int d = 0; d < 3; ++d) acc[kSqBox + d] += box.L[d];
  }
}

}  // namespace chem
