// chem_rdf_host.hpp -- radial distribution functions (chem_rdf_*): the edge table, the bin of a squared distance, the selector
// match and its 16 x 16 mask table, the normaliser M from the type counts, the LDS budget and the launch plan.
// Rule set: include/chem_mi355.h ("radial distribution functions").  Plain C++ like chem_region_host.hpp, so that
// tests/host/rdf_harness.cpp checks it on the CPU; the functions marked CHEM_RDFHD are also what k_rdf_tiles, k_rdf_all and
// k_rdf_frame (md_kernels.hpp) call on the device, so host and device cannot drift apart.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/chem_mi355.h"

#if defined(__HIPCC__)
#define CHEM_RDFHD __host__ __device__ inline
#else
#define CHEM_RDFHD inline
#endif

namespace chem {

constexpr int kRdfMaxPairs = CHEM_RDF_MAX_PAIRS, kRdfMaxBins = CHEM_RDF_MAX_BINS;
// words in front of the histograms in the accumulator array (u64 each): frames, pairs[8], density[8] (the bits of a double), types[16]
constexpr int kRdfFrames = 0, kRdfPairs = 1, kRdfDensity = 1 + kRdfMaxPairs, kRdfTypes = 32, kRdfHead = 32 + CHEM_MAX_TYPES;
// (kRdfTypes: the type counts of the frame being taken, filled by k_rdf_count and cleared again by k_rdf_frame)
// the all-pairs pass of the per-cell and brute-force paths is O(N^2): refused above this many particles
constexpr int kRdfAllPairsMax = 65536;

// what the kernels take by value
struct RdfArgs {
  double dr, inv_dr;      // r_max / nbins in fp64 (the edges derive from dr alone), and its reciprocal for the guess
  int nbins, nsel, parts; // parts: 1, or 2 with the molecule split (intra first, then inter)
  int pad_;
  unsigned char mask[CHEM_MAX_TYPES][CHEM_MAX_TYPES];      // bit s: selector s counts a pair of these two types
};

// e[k] = (double)k * dr and e2[k] = e[k] * e[k], each one rounding, no contraction
CHEM_RDFHD double rdf_edge(int k, double dr) { return (double)k * dr; }
CHEM_RDFHD double rdf_edge2(int k, double dr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double e = (double)k * dr;
  return e * e;
}
// the bin k with e2[k] <= d2 < e2[k + 1], or -1 where d2 >= e2[nbins] (or d2 is not a number).  The square root only guesses;
// the edges decide, so the answer does not depend on how sqrt or the division round.
CHEM_RDFHD int rdf_bin(double d2, double dr, double inv_dr, int nbins) {
  if (!(d2 < rdf_edge2(nbins, dr))) return -1;
  if (!(d2 >= 0.0)) return -1;
  const double g = ::sqrt(d2) * inv_dr;
  int k = g < (double)nbins ? (int)g : nbins - 1;
  if (k < 0) k = 0;
  if (k > nbins - 1) k = nbins - 1;
  while (k > 0 && d2 < rdf_edge2(k, dr)) --k;
  while (k < nbins - 1 && d2 >= rdf_edge2(k + 1, dr)) ++k;
  return k;
}

// selector (t1, t2), unordered, -1 = any type
CHEM_RDFHD bool rdf_match(int t1, int t2, int a, int b) {
  return ((t1 < 0 || t1 == a) && (t2 < 0 || t2 == b)) || ((t1 < 0 || t1 == b) && (t2 < 0 || t2 == a));
}
inline void rdf_fill_masks(int nsel, const int32_t* tp, unsigned char mask[CHEM_MAX_TYPES][CHEM_MAX_TYPES]) {
  for (int a = 0; a < CHEM_MAX_TYPES; ++a)
    for (int b = 0; b < CHEM_MAX_TYPES; ++b) {
      unsigned m = 0;
      for (int s = 0; s < nsel; ++s) if (rdf_match(tp[2 * s], tp[2 * s + 1], a, b)) m |= 1u << s;
      mask[a][b] = (unsigned char)m;
    }
}
// M of selector s: unordered pairs of distinct particles whose types match, from the type counts c[]
CHEM_RDFHD unsigned long long rdf_norm_pairs(const unsigned char mask[CHEM_MAX_TYPES][CHEM_MAX_TYPES], int s, const long long* c) {
  unsigned long long m = 0;
  for (int u = 0; u < CHEM_MAX_TYPES; ++u)
    for (int v = u; v < CHEM_MAX_TYPES; ++v) {
      if (!((mask[u][v] >> s) & 1u)) continue;
      m += u == v ? (unsigned long long)(c[u] * (c[u] - 1) / 2) : (unsigned long long)(c[u] * c[v]);
    }
  return m;
}

// chem_rdf_init: 0, or CHEM_EINVAL with the reason in `why`
inline int rdf_validate(double r_max, int nbins, int npairs, const int32_t* tp, std::string& why) {
  auto bad = [&](const std::string& w) { why = w; return CHEM_EINVAL; };
  if (npairs < 0 || npairs > kRdfMaxPairs) return bad("rdf: npairs " + std::to_string(npairs) + " outside 0.." + std::to_string(kRdfMaxPairs));
  if (npairs == 0) return 0;
  if (!std::isfinite(r_max) || !(r_max > 0)) return bad("rdf: r_max must be finite and positive");
  if (nbins < 1 || nbins > kRdfMaxBins) return bad("rdf: nbins " + std::to_string(nbins) + " outside 1.." + std::to_string(kRdfMaxBins));
  if (!tp) return bad("rdf: null type_pairs");
  for (int k = 0; k < 2 * npairs; ++k)
    if (tp[k] < -1 || tp[k] >= CHEM_MAX_TYPES) return bad("rdf: type " + std::to_string(tp[k]) + " outside -1.." + std::to_string(CHEM_MAX_TYPES - 1));
  return 0;
}

inline size_t rdf_hist_words(int nbins, int nsel, int parts) { return (size_t)nbins * nsel * parts; }

// Launch plan.  path 0: tiles (k_rdf_tiles: the staged image of a tile, the histogram behind it), 1: per-cell or brute-force
// list (k_rdf_all: all pairs in chunks of kRdfChunk staged particles).  The histogram is u32 words in LDS on both.
constexpr int kRdfChunk = 256;
constexpr size_t kRdfChunkBytes = (size_t)kRdfChunk * (3 * sizeof(double) + 3 * sizeof(int));   // position, tag, type, molecule
struct RdfPlan { int grid, block; size_t hist_off, lds_bytes; };
inline size_t rdf_align16(size_t b) { return (b + 15) / 16 * 16; }
// image_bytes: the tile image (path 0); budget: the dynamic LDS a workgroup may ask for; ncu: compute units; work: tiles (path 0)
// or particles (path 1).  Refuses (false, reason in `why`) a histogram that does not fit beside the staged data.
inline bool rdf_plan(int path, int nbins, int nsel, int parts, size_t image_bytes, size_t budget, int ncu, long long work, RdfPlan& p, std::string& why) {
  if (nbins < 1 || nbins > kRdfMaxBins) { why = "rdf: nbins outside 1.." + std::to_string(kRdfMaxBins); return false; }
  if (nsel < 1 || nsel > kRdfMaxPairs) { why = "rdf: npairs outside 1.." + std::to_string(kRdfMaxPairs); return false; }
  if (parts < 1 || parts > 2) { why = "rdf: parts"; return false; }
  const size_t hist = rdf_hist_words(nbins, nsel, parts) * sizeof(uint32_t);
  p.hist_off = rdf_align16(path == 0 ? image_bytes : kRdfChunkBytes);
  p.lds_bytes = p.hist_off + hist;
  if (p.lds_bytes > budget) {
    why = "rdf: a histogram of " + std::to_string(hist) + " bytes does not fit the LDS beside " + std::to_string(p.hist_off) + " bytes of staged particles (budget " +
          std::to_string(budget) + "): fewer bins or selectors";
    return false;
  }
  if (path != 0 && work > kRdfAllPairsMax) {
    why = "rdf: " + std::to_string(work) + " particles on a path without tiles: the all-pairs pass is O(N^2) and stops at " + std::to_string(kRdfAllPairsMax) +
          " particles (a box of at least five cells per axis runs on the tile path)";
    return false;
  }
  if (path == 0) {
    // persistent: a workgroup keeps its histogram over the tiles it loops over and flushes once.  As many workgroups as fit
    // the LDS of a compute unit (160 KB), two at the most.
    const int per_cu = p.lds_bytes * 2 + 8192 <= 160 * 1024 ? 2 : 1;
    p.block = 512;
    long long g = (long long)per_cu * (ncu > 0 ? ncu : 1);
    p.grid = (int)(work < g ? (work > 0 ? work : 1) : g);
  } else {
    p.block = 256;
    long long g = (work + p.block - 1) / p.block, cap = 4LL * (ncu > 0 ? ncu : 1);
    if (g > cap) g = cap;
    p.grid = (int)(g > 0 ? g : 1);
  }
  return true;
}

}  // namespace chem
