// chem_sq_host.hpp -- static structure factor (chem_sq_*): the enumeration of the wave vectors and its inverse, validation, the
// selector -> type-class table, the accumulator layout and the launch plan.  Rule set: include/chem_mi355.h ("static structure
// factor").  Plain C++ like chem_rdf_host.hpp, so that tests/host/sq_harness.cpp checks it on the CPU; the functions marked
// CHEM_SQHD are also what k_sq_walk, k_sq_reduce and k_sq_accum (md_kernels.hpp) call on the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/chem_mi355.h"

#if defined(__HIPCC__)
#define CHEM_SQHD __host__ __device__ inline
#else
#define CHEM_SQHD inline
#endif

namespace chem {

constexpr int kSqMaxN = CHEM_SQ_MAX_N, kSqMaxPairs = CHEM_SQ_MAX_PAIRS, kSqMaxClasses = 2 * CHEM_SQ_MAX_PAIRS;
// doubles in front of the sums in the accumulator array: frames, na[4], nb[4], box_sum[3]; from kSqTypes on the type counts of the
// frame being taken, as u64 words (filled by k_rdf_count, read and cleared by k_sq_accum)
constexpr int kSqFrames = 0, kSqNa = 1, kSqNb = 1 + kSqMaxPairs, kSqBox = 1 + 2 * kSqMaxPairs, kSqTypes = 32, kSqHead = 32 + CHEM_MAX_TYPES;

// ---- wave vectors: the canonical half of |n_a| <= nmax, lexicographic in (nx, ny, nz) ----
CHEM_SQHD long long sq_nvec(int nmax) { const long long w = 2LL * nmax + 1; return (w * w * w - 1) / 2; }
CHEM_SQHD bool sq_kept(int nx, int ny, int nz) { return nx > 0 || (nx == 0 && (ny > 0 || (ny == 0 && nz > 0))); }
// k -> n: first (0, 0, 1..nmax), then (0, 1..nmax, -nmax..nmax), then (1..nmax, -nmax..nmax, -nmax..nmax)
CHEM_SQHD void sq_vec(long long k, int nmax, int& nx, int& ny, int& nz) {
  const long long w = 2LL * nmax + 1;
  if (k < nmax) { nx = 0; ny = 0; nz = (int)k + 1; return; }
  k -= nmax;
  if (k < nmax * w) { nx = 0; ny = 1 + (int)(k / w); nz = (int)(k % w) - nmax; return; }
  k -= nmax * w;
  nx = 1 + (int)(k / (w * w));
  const long long r = k % (w * w);
  ny = (int)(r / w) - nmax; nz = (int)(r % w) - nmax;
}
// n -> k, or -1 where n is not a kept vector of this nmax
CHEM_SQHD long long sq_index(int nx, int ny, int nz, int nmax) {
  if (!sq_kept(nx, ny, nz)) return -1;
  if (nx > nmax || ny > nmax || ny < -nmax || nz > nmax || nz < -nmax) return -1;
  const long long w = 2LL * nmax + 1;
  if (nx == 0 && ny == 0) return nz - 1;
  if (nx == 0) return nmax + (long long)(ny - 1) * w + (nz + nmax);
  return nmax + nmax * w + (long long)(nx - 1) * w * w + (long long)(ny + nmax) * w + (nz + nmax);
}

// chem_sq_init: 0, or CHEM_EINVAL with the reason in `why`
inline int sq_validate(int nmax, int npairs, const int32_t* tp, std::string& why) {
  auto bad = [&](const std::string& w) { why = w; return CHEM_EINVAL; };
  if (npairs < 0 || npairs > kSqMaxPairs) return bad("sq: npairs " + std::to_string(npairs) + " outside 0.." + std::to_string(kSqMaxPairs));
  if (npairs == 0) return 0;
  if (nmax < 1 || nmax > kSqMaxN) return bad("sq: nmax " + std::to_string(nmax) + " outside 1.." + std::to_string(kSqMaxN));
  if (!tp) return bad("sq: null type_pairs");
  for (int k = 0; k < 2 * npairs; ++k)
    if (tp[k] < -1 || tp[k] >= CHEM_MAX_TYPES) return bad("sq: type " + std::to_string(tp[k]) + " outside -1.." + std::to_string(CHEM_MAX_TYPES - 1));
  return 0;
}

// what the kernels take by value.  A class is a set of types: one type, or all of them (-1).  rho is accumulated per class; the
// selector s pairs the classes sel_a[s] and sel_b[s].  tmask[t]: the classes a particle of type t belongs to.
struct SqArgs {
  int nmax, nvec, ncls, nsel;
  int cls[kSqMaxClasses];
  int sel_a[kSqMaxPairs], sel_b[kSqMaxPairs];
  unsigned char tmask[CHEM_MAX_TYPES];
};
// the distinct type sets of the selectors in the order of their first appearance (t1 of selector 0, t2 of selector 0, ...)
inline void sq_fill_classes(int nmax, int npairs, const int32_t* tp, SqArgs& a) {
  a = SqArgs{};
  a.nmax = nmax; a.nvec = (int)sq_nvec(nmax); a.nsel = npairs;
  for (int k = 0; k < 2 * npairs; ++k) {
    int c = 0;
    while (c < a.ncls && a.cls[c] != tp[k]) ++c;
    if (c == a.ncls) a.cls[a.ncls++] = tp[k];
    if (k & 1) a.sel_b[k / 2] = c; else a.sel_a[k / 2] = c;
  }
  for (int t = 0; t < CHEM_MAX_TYPES; ++t) {
    unsigned m = 0;
    for (int c = 0; c < a.ncls; ++c) if (a.cls[c] < 0 || a.cls[c] == t) m |= 1u << c;
    a.tmask[t] = (unsigned char)m;
  }
}
// the particles of class c, from the type counts
CHEM_SQHD long long sq_class_count(const SqArgs& a, int c, const long long* cnt) {
  long long m = 0;
  for (int t = 0; t < CHEM_MAX_TYPES; ++t) if ((a.tmask[t] >> c) & 1u) m += cnt[t];
  return m;
}

// ---- launch plan ----
// k_sq_walk: a workgroup of kSqBlock threads owns kSqQBlock wave vectors (kSqVpl per lane) and one super-chunk of `per` particle
// slots, which it stages kSqChunk particles at a time: three phasor tables of nmax + 1 complex doubles per particle in LDS.  It
// writes one partial per (class, vector); k_sq_reduce sums the super-chunks in index order.  The partials are bounded at
// kSqScratchMax bytes by taking fewer, longer super-chunks; nothing inside the limits of chem_sq_init is refused.
constexpr int kSqBlock = 256, kSqVpl = 2, kSqQBlock = kSqBlock * kSqVpl, kSqChunk = 64;
constexpr size_t kSqScratchMax = (size_t)32 << 20;
struct SqPlan { int nqb, nsuper, per, block; size_t lds_bytes, scratch_bytes; };
inline size_t sq_lds_bytes(int nmax) { return (size_t)3 * kSqChunk * (nmax + 1) * 2 * sizeof(double); }
inline size_t sq_partial_bytes(int nmax, int ncls) { return (size_t)ncls * (size_t)sq_nvec(nmax) * 2 * sizeof(double); }   // of one super-chunk
// the most super-chunks any particle count gets (what the scratch is allocated for)
inline int sq_super_cap(int nmax, int ncls, int ncu) {
  const long long nqb = (sq_nvec(nmax) + kSqQBlock - 1) / kSqQBlock;
  long long want = (4LL * (ncu > 0 ? ncu : 1) + nqb - 1) / nqb;
  const long long fit = (long long)(kSqScratchMax / sq_partial_bytes(nmax, ncls));
  if (want > fit) want = fit;
  return (int)(want > 1 ? want : 1);
}
// n: particle slots of the range (>= 1); budget: the dynamic LDS a workgroup may ask for; ncu: compute units
inline bool sq_plan(long long n, int nmax, int ncls, size_t budget, int ncu, SqPlan& p, std::string& why) {
  if (nmax < 1 || nmax > kSqMaxN) { why = "sq: nmax outside 1.." + std::to_string(kSqMaxN); return false; }
  if (ncls < 1 || ncls > kSqMaxClasses) { why = "sq: classes outside 1.." + std::to_string(kSqMaxClasses); return false; }
  if (n < 1 || n > 0x7fffffffLL - kSqChunk) { why = "sq: particle count"; return false; }
  p.block = kSqBlock;
  p.lds_bytes = sq_lds_bytes(nmax);
  if (p.lds_bytes > budget) { why = "sq: phasor tables of " + std::to_string(p.lds_bytes) + " bytes beyond the LDS budget " + std::to_string(budget); return false; }
  p.nqb = (int)((sq_nvec(nmax) + kSqQBlock - 1) / kSqQBlock);
  const long long chunks = (n + kSqChunk - 1) / kSqChunk;
  long long ns = sq_super_cap(nmax, ncls, ncu);
  if (ns > chunks) ns = chunks;
  const long long per_chunks = (chunks + ns - 1) / ns;
  p.per = (int)(per_chunks * kSqChunk);
  p.nsuper = (int)((chunks + per_chunks - 1) / per_chunks);      // (no empty super-chunk)
  p.scratch_bytes = (size_t)p.nsuper * sq_partial_bytes(nmax, ncls);
  return true;
}

}  // namespace chem
