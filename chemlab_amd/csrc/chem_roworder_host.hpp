// chem_roworder_host.hpp -- where the rows of a tile's force list are stored (option row_order).
// A lane of the force kernel owns one row and walks it in chunks of eight entries; the 64 lanes of a wave walk to the longest
// of their rows.  Rows of one wave should therefore be equally long: the fused rebuild stores a tile's rows ordered by their
// chunk count, and the rows of the last, partly filled pass of P lanes -- whose lanes have walked a row of every full pass
// before -- are the shortest of the tile.  Every row keeps its entries and their order; the count word of a position (nnh)
// names, beside the row's entries, the home particle (its index in the tile's cell-run order, `qnat`) whose row sits there:
// one load gives the force kernel both, and no pointer more to hold (its scalar registers are all taken).
// The arithmetic is shared by the kernels
// (md_kernels.hpp dev_row_order) and the host; tests/host/roworder_harness.cpp checks it on the CPU.  No HIP include.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/chem_philox.h"      // CHEM_HD

namespace chem {

constexpr int kRowClasses = 32;       // chunk-count classes the device's counting sort keeps: rows of up to 8 * 31 entries
constexpr int kRowStageMax = 2048;    // home particles of a tile the device orders (32 wave-passes); fuller tiles keep the natural order

// count word of a stored row: entries (<= the row stride, < 65536) | home << 16 (a tile stages < 65536 slots)
CHEM_HD int row_word(int cnt, int home) { return (int)((unsigned int)cnt | ((unsigned int)home << 16)); }
CHEM_HD int row_word_count(int w) { return w & 0xffff; }
CHEM_HD int row_word_home(int w) { return (int)((unsigned int)w >> 16); }

CHEM_HD int row_chunks(int cnt) { return (cnt + 7) >> 3; }
// size of the last pass: nh - (ceil(nh / P) - 1) P  (nh <= P: all of them; an empty tile: none)
CHEM_HD int row_last_pass(int nh, int P) { return nh <= 0 ? 0 : nh - ((nh + P - 1) / P - 1) * P; }
// position of the row with rank `rank` in ascending (chunks, natural index) order: the R shortest fill the last pass, the
// others the full passes in ascending order
CHEM_HD int row_position(int rank, int nh, int P) {
  const int R = row_last_pass(nh, P);
  return rank < R ? (nh - R) + rank : rank - R;
}

// the whole order of one tile on the host: cnt[i] = entries of the row of home i (natural index), out: qnat[position] = i.
// Counting sort over the chunk counts (stable: ties resolve by natural index).
inline std::vector<unsigned short> row_order(const int* cnt, int nh, int P) {
  std::vector<unsigned short> qnat((size_t)std::max(nh, 0));
  int kmax = 0;
  for (int i = 0; i < nh; ++i) kmax = std::max(kmax, row_chunks(cnt[i]));
  std::vector<int> start((size_t)kmax + 2, 0);
  for (int i = 0; i < nh; ++i) ++start[(size_t)row_chunks(cnt[i]) + 1];
  for (int k = 0; k <= kmax; ++k) start[(size_t)k + 1] += start[(size_t)k];
  for (int i = 0; i < nh; ++i) qnat[(size_t)row_position(start[(size_t)row_chunks(cnt[i])]++, nh, P)] = (unsigned short)i;
  return qnat;
}

// ---- plan.  The device orders a tile behind its sweep, which therefore writes into a staging region of the workgroup: rows
// of `cap` home particles.  Twice the mean occupancy of a full tile of home_cells cells (gelation makes tiles unequal; the
// narrower tiles at the box's edges hold less) and never more than a tile can stage; a tile with more home particles than
// that is stored in the natural order.
inline int row_stage_cap(int npart, int ncell, int home_cells, int tile_cap) {
  const long long full = ncell > 0 ? ((long long)npart * home_cells + ncell - 1) / ncell : 0;
  return (int)std::max<long long>(64, std::min<long long>(std::min<long long>(2 * full + 64, tile_cap), kRowStageMax));
}
// the option holds on the single-domain fused tile path, for row strides the classes cover.  (The force kernel reads qnat
// at every lane-per-row setting; the rule is made for one lane per row, P = the force kernel's workgroup size.)
inline bool row_order_on(int opt, bool fused, bool tiles, bool dd_on, int S16) {
  return opt != 0 && fused && tiles && !dd_on && S16 / 8 + 1 <= kRowClasses;
}

}  // namespace chem
