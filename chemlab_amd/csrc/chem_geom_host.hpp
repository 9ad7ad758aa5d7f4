// chem_geom_host.hpp -- the planning rules of one context: how many cells the box has, which cell layers a slab owns,
// whether the LDS tiles or the per-cell kernels run, the capacities of tiles, list rows and slab buffers, and how each
// grows after an overflow.  Plain integer and double arithmetic over plain structs: CtxT (chem_api.hip) calls these
// between its allocations and launches, tests/host/geometry_harness.cpp checks them on the CPU.  No device code and no
// HIP include; the tile geometry at the top is shared with the kernels (md_kernels.hpp includes this header).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/chem_philox.h"      // CHEM_HD: __host__ __device__ inline under hipcc, inline otherwise
#include "chem_host.hpp"

namespace chem {

// ---- tile geometry (md_kernels.hpp "Tiled path"): a tile = HX x HY x HZ home cells, staged with its stencil of SX x SY x SZ
#ifndef CHEM_HX
#define CHEM_HX 3
#endif
#ifndef CHEM_HY
#define CHEM_HY 3
#endif
#ifndef CHEM_HZ
#define CHEM_HZ 3
#endif
constexpr int HX = CHEM_HX, HY = CHEM_HY, HZ = CHEM_HZ;   // ~490 home particles at 18/cell: one pass of a 512-thread block; stencil 5^3 cells (x4.6)
constexpr int SX = HX + 2, SY = HY + 2, SZ = HZ + 2;

// Tiles along x: xs_nb tiles of HX cells, then tiles of xs_w cells (Box::xs_nb / xs_w).  A force launch of one-shot
// workgroups ends with a partly filled last round (1728 equal tiles on 768 resident slots: 2.25 rounds take the time of 3);
// a share of narrow tiles -- shorter jobs, scheduled last by the largest-first order -- fills it.  Splitting along x (the
// fastest tile index) gives every XCD's contiguous tile range the same mix.
CHEM_HD int tile_nbx(int nx, int xs_nb) { return xs_nb * HX >= nx ? (nx + HX - 1) / HX : xs_nb; }      // wide tiles in a row (the last may be cut)
CHEM_HD int tile_ntx(int nx, int xs_nb, int xs_w) {
  const int nb = tile_nbx(nx, xs_nb);
  return nb * HX >= nx ? nb : nb + (nx - nb * HX + xs_w - 1) / xs_w;
}
CHEM_HD void tile_xrange(int tx, int nx, int xs_nb, int xs_w, int& cx0, int& hx) {
  const int nb = tile_nbx(nx, xs_nb);
  if (tx < nb) { cx0 = tx * HX; hx = HX < nx - cx0 ? HX : nx - cx0; }
  else { cx0 = nb * HX + (tx - nb) * xs_w; hx = xs_w < nx - cx0 ? xs_w : nx - cx0; }
}

// ---- cells: floor(L / (rc + skin_eff)) per axis; fewer than 3 on ANY axis -> no cells at all (brute-force list)
struct CellGrid { int nc[3]; bool cells; };      // nc = 0 without cells
inline CellGrid cell_grid(const double L[3], double rl) {
  CellGrid g{{0, 0, 0}, true};
  for (int d = 0; d < 3; ++d) { g.nc[d] = (int)std::floor(L[d] / rl); if (g.nc[d] < 3) g.cells = false; }
  if (!g.cells) g.nc[0] = g.nc[1] = g.nc[2] = 0;
  return g;
}

// ---- slab layout: rank rk of P owns the cell layers [z0, z0 + ncz) of the nzg along z; the first nzg % P ranks own one more
struct SlabLayers { int nzg, ncz, z0, lower, upper; };
inline SlabLayers slab_layers(const CellGrid& g, int P, int rk) {
  if (!g.cells) throw ChemError(CHEM_EINVAL, "domain decomposition needs at least 3 cells of edge rc+skin per axis");
  const int nzg = g.nc[2], base = nzg / P, rem = nzg % P;
  if (base < 2) throw ChemError(CHEM_EINVAL, "domain decomposition: fewer than 2 cell layers per rank along z");
  return SlabLayers{nzg, base + (rk < rem ? 1 : 0), rk * base + std::min(rk, rem), (rk + P - 1) % P, (rk + 1) % P};
}
// the layer of a coordinate: folded into [0, Lz) (s = the boxes taken off), scaled, clamped
struct SlabCoord { double z, s; int layer; };
inline SlabCoord slab_layer_of(double z, double Lz, int nzg) {
  const double s = std::floor(z / Lz);
  z -= s * Lz; if (z >= Lz) z -= Lz;
  const int gz = (int)std::floor(z * nzg / Lz);
  return SlabCoord{z, s, std::min(std::max(gz, 0), nzg - 1)};
}
// capacities of a slab: ghost layers are one cell layer each (G, in front of and behind the reals), the migration
// buffers hold a quarter layer (mcap), the reals fluctuate with the slab occupancy (cap = everything allocated)
struct SlabCaps { int G, mcap, cap; };
inline SlabCaps slab_capacities(int nglob, int nzg, int ncz) {
  const double per_layer = (double)nglob / nzg;
  SlabCaps c{};
  c.G = (int)(per_layer * 1.5) + 1024;
  c.mcap = std::max(4096, (int)(per_layer / 4));
  c.cap = 2 * c.G + (int)(per_layer * ncz * 1.2) + 2 * c.mcap + 4096;
  return c;
}

// ---- automatic list skin (measured on the 1M-particle melt, profiles/round3_list_skin.txt): two cells fewer per axis than
// the workload's skin would give, i.e. ~0.2 sigma more skin at rc + skin = 2.8 -- the lists live ~60 % longer for ~20 % more
// entries -- and always the whole cell edge (the slack between L / floor(L / rl) and rl is free skin).
// opt_list_skin: < 0 automatic, 0 off, > 0 explicit; npart: all particles of the system.  0 = the workload's skin stays.
inline double pick_list_skin(const double L[3], double rc, double skin, double opt_list_skin, int criterion, bool tiles, bool fused,
                             bool dd_on, int P, int npart) {
  if (opt_list_skin == 0.0 || criterion != 0 || !tiles || (!dd_on && !fused)) return 0.0;
  const double rl = rc + skin;
  double edge = 1e300;
  for (int d = 0; d < 3; ++d) {
    int nc = (int)std::floor(L[d] / (opt_list_skin > 0 ? rc + opt_list_skin : rl));
    if (opt_list_skin < 0) { if (npart < 100000) return 0.0; nc -= 2; }
    if (nc < 5) return 0.0;
    if (dd_on && d == 2 && nc / P < 2) return 0.0;      // (a slab needs two cell layers)
    edge = std::min(edge, L[d] / nc);
  }
  const double s = edge * (1.0 - 1e-9) - rc;
  return s > skin ? s : 0.0;
}

// ---- row stride of the neighbour list: 1.6 x the mean count of a sphere of radius rl (+48), or the user's capacity; never more
// than the other particles; in multiples of 16
inline int row_stride(const double L[3], double rl, int npart, int user_capacity) {
  const double vol = L[0] * L[1] * L[2];
  const double expect = 4.0 / 3.0 * 3.14159265358979323846 * rl * rl * rl * npart / vol;
  int ncap = user_capacity > 0 ? user_capacity : (int)(expect * 1.6 + 48);
  ncap = std::min(ncap, std::max(npart - 1, 1));
  return (ncap + 15) / 16 * 16;
}

// ---- tile plan.  ncx, ncy: cells along x and y; nz_own: cell layers whose tiles this context runs (a slab: its own layers);
// nz_all: layers of the whole box; npart: particles of the whole box.  lds_need(cap) = bytes of dynamic LDS the kernels ask
// for a tile of `cap` slots.  tile_cap stays 0 where the cell grid allows no tiles.
struct TilePlan { bool use_tiles; int tile_cap, xs_nb, xs_w, ntiles; };
inline int tiles_per_layer(int ncx, int ncy, int xs_nb, int xs_w) { return tile_ntx(ncx, xs_nb, xs_w) * ((ncy + HY - 1) / HY); }
template <class LdsNeed>
inline TilePlan plan_tiles(int ncx, int ncy, int nz_own, int nz_all, int npart, bool dd_on, bool opt_tiles, int tile_split, LdsNeed lds_need,
                           size_t lds_budget) {
  TilePlan p{false, 0, 1 << 20, 1, 0};      // (all tiles HX wide unless tile_split says otherwise)
  p.use_tiles = opt_tiles && ncx >= HX + 2 && ncy >= HY + 2 && (dd_on || nz_own >= HZ + 2);
  if (dd_on && !(ncx >= HX + 2 && ncy >= HY + 2)) throw ChemError(CHEM_EINVAL, "domain decomposition needs >= 5 cells along x and y");
  // (the per-cell kernels know nothing of ghost layers: with tiles=0 a slab used to run on and return wrong forces -- found by
  //  tests/test_gpu_sweep.py case 100)
  if (dd_on && !p.use_tiles) throw ChemError(CHEM_EINVAL, "domain decomposition needs the LDS-staged tiles: option tiles=0 is a single-domain switch");
  if (p.use_tiles) {
    // LDS capacity from the mean stencil occupancy (+12 % for density fluctuations), in 256-slot steps
    const double per_cell = (double)npart / ((double)ncx * ncy * nz_all);
    const int need = (int)(SX * SY * SZ * per_cell * 1.12) + 64;
    p.tile_cap = std::max(1024, (need + 255) / 256 * 256);
    // every kernel that stages a tile must fit: the force kernel's image AND the list build's (SoA groups + type masks +
    // slice boundaries: ~22 B per slot against 16), next to the static __shared__ of k_rebuild_fused / k_nlist_tiles
    if (lds_need(p.tile_cap) > lds_budget) {   // cells too crowded: per-cell kernels
      if (dd_on) throw ChemError(CHEM_ENOSPC, "domain decomposition needs the LDS-staged tiles, and a stencil of this density does not fit the LDS");
      p.use_tiles = false;
    }
  }
  // Narrow tiles (tile_xrange): option tile_split = nb * 10 + w, 0 = off (default).
  // Built to fill the last round of the force launch (1728 equal one-shot workgroups on 768 resident slots: 2.25 rounds of
  // work) with shorter jobs, and measured: no gain at any mix -- C5: 7811 steps/s unsplit, 7549 with 10 wide + 6 one-cell
  // tiles per row, 7721 with 11 + 3; 125k particles: 22980 unsplit, 20134 all one cell wide (profiles/round3_tile_split.txt).
  // The workgroups of the last round run faster on their emptier CUs than the model assumed; the extra staging is not paid back.
  if (p.use_tiles && tile_split > 0 && HX >= 2) {
    const int nb = tile_split / 10, w = std::max(1, std::min(tile_split % 10, HX));
    if (nb * HX < ncx) { p.xs_nb = nb; p.xs_w = w; }
  }
  p.ntiles = p.use_tiles ? tiles_per_layer(ncx, ncy, p.xs_nb, p.xs_w) * ((nz_own + HZ - 1) / HZ) : 0;
  return p;
}

// ---- growth after an overflow (`overflow` = what the device asked for): tile capacity +12.5 % in 256-slot steps, row stride
// +25 % in multiples of 16 and never beyond the nmax particles of the system
inline int grown_tile_cap(int overflow) { return (overflow + overflow / 8 + 255) / 256 * 256; }
inline int grown_row_stride(int overflow, int nmax) {
  return std::min(((int)(overflow * 1.25) + 31) / 16 * 16, std::max((nmax + 15) / 16 * 16, 16));
}

// ---- tile order of the fused rebuild (single domain): inside each of the eight contiguous ranges xcd_remap hands to the
// XCDs, the tiles with the most home cells first (stable).  pos is the inverse of ord.  Fewer than 8 tiles: no order.
struct TileOrder { std::vector<int> ord, pos; };
inline TileOrder tile_order(const int nc[3], int xs_nb, int xs_w, int ntiles) {
  TileOrder o;
  if (ntiles < 8) return o;
  const int ntx = tile_ntx(nc[0], xs_nb, xs_w), nty = (nc[1] + HY - 1) / HY;
  auto home_cells = [&](int tile) {
    const int tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
    int cx0, hx;
    tile_xrange(tx, nc[0], xs_nb, xs_w, cx0, hx);
    return hx * std::min(HY, nc[1] - ty * HY) * std::min(HZ, nc[2] - tz * HZ);
  };
  o.ord.resize(ntiles); o.pos.resize(ntiles);
  const int q = ntiles >> 3, r = ntiles & 7;
  for (int x = 0, off = 0; x < 8; ++x) {
    const int cnt = q + (x < r ? 1 : 0);
    for (int k = 0; k < cnt; ++k) o.ord[off + k] = off + k;
    std::stable_sort(o.ord.begin() + off, o.ord.begin() + off + cnt, [&](int a, int b) { return home_cells(a) > home_cells(b); });
    for (int k = 0; k < cnt; ++k) o.pos[o.ord[off + k]] = off + k;
    off += cnt;
  }
  return o;
}

// ---- segment shift of the fused rebuild's scans: segments of 1 << shift items, at least 1 << lo, at most maxseg of them
inline int segment_shift(int nitem, int lo, int maxseg) {
  int sh = lo;
  while (((nitem + (1 << sh) - 1) >> sh) > maxseg) ++sh;
  return sh;
}

// ---- tile layers of a slab (tiles are numbered x fastest, z slowest: a layer = ntxy consecutive tiles).  The force launch
// runs all tiles (which = 0), the interior ones (1: every layer but the lowest and the highest, they need no ghost) or
// the two boundary layers (2); the fields are md_kernels.hpp TileSub's, count = workgroups of the launch.
struct TileLayers { int base1, n1, base2, count; };
inline TileLayers tile_subset(int ntiles, int ntxy, int which) {
  if (which == 1) return TileLayers{ntxy, ntiles - 2 * ntxy, 0, ntiles - 2 * ntxy};
  if (which == 2) return TileLayers{0, ntxy, ntiles - ntxy, 2 * ntxy};
  return TileLayers{0, ntiles, 0, ntiles};
}
// Interior forces while the halo exchange is in flight.  Measured with one rank (1M particles, RCCL to self): the
// cross-stream hand-over costs ~15 us and the boundary launch cannot fill the chip, so the overlap only pays once the
// interior force kernel is much longer than that -- automatic (opt_overlap < 0) for slabs of >= 8192 tiles (~4M particles
// per GPU), option overlap_halo.
inline bool halo_overlap(int opt_overlap, bool use_tiles, int ntiles, int ntxy, bool host_polls) {
  const bool want_overlap = opt_overlap > 0 || (opt_overlap < 0 && ntiles >= 8192);
  return want_overlap && use_tiles && ntiles > 2 * ntxy && host_polls;
}

}  // namespace chem
