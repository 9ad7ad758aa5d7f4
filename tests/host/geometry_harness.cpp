// Test harness (CPU only): drives the planning rules of chemlab_amd/csrc/chem_geom_host.hpp from a plain-text script on stdin
// and prints what they return, so that a pytest can compare it with a model of its own.  Not part of the product library.
// Every double travels as the decimal bit pattern of its 8 bytes (<x>), so that a box edge arrives as the very float the
// engine is given.  A ChemError prints "error <code> <message>".
//   cells <Lx> <Ly> <Lz> <rl>                          "cells <0|1> nx ny nz"
//   slab <nzg> <P> <rk>                                "slab ncz z0 lower upper"
//   layer <Lz> <nzg> <k> <z>...                        "layer g..."
//   caps <nglob> <nzg> <ncz>                           "caps G mcap cap"
//   skin <Lx> <Ly> <Lz> <rc> <skin> <opt> criterion tiles fused dd P npart     "skin <bits of the result>"
//   stride <Lx> <Ly> <Lz> <rl> npart user_capacity     "stride S"
//   grow overflow nmax                                 "grow tile_cap row_stride"
//   tiles <Lx> <Ly> <Lz> <rc> <skin> n <opt_list_skin> criterion tiles fused tile_split dd P rk bytes_per_slot budget
//        the whole plan as CtxT::setup_geometry_once runs it (list skin, cells, slab, row stride, tile plan; the LDS need of
//        a capacity is bytes_per_slot * capacity, budget 0 = unlimited):
//        "tiles ntiles ncx nwide w rows tile_cap" (the six numbers of chem_debug_tiles) + " use_tiles S z0 ncz"
//   xrange nx xs_nb xs_w                               "xrange ntx cx0:hx..."
//   order ncx ncy ncz xs_nb xs_w ntiles                "order k ord[0..k) pos[0..k)" (k = 0: no order)
//   shift nitem lo maxseg                              "shift sh"
//   layers ntiles ntxy which                           "layers base1 n1 base2 count"
//   overlap opt use_tiles ntiles ntxy host_polls       "overlap <0|1>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_geom_host.hpp"
using namespace chem;
static double rd(std::istream& is) { unsigned long long b = 0; is >> b; double v; std::memcpy(&v, &b, 8); return v; }
static void run(const std::string& cmd, std::istream& is) {
  if (cmd == "cells") {
    double L[3] = {rd(is), rd(is), rd(is)}; const double rl = rd(is);
    const CellGrid g = cell_grid(L, rl);
    printf("cells %d %d %d %d\n", g.cells ? 1 : 0, g.nc[0], g.nc[1], g.nc[2]);
  } else if (cmd == "slab") {
    int nzg, P, rk; is >> nzg >> P >> rk;
    const SlabLayers s = slab_layers(CellGrid{{5, 5, nzg}, true}, P, rk);
    printf("slab %d %d %d %d\n", s.ncz, s.z0, s.lower, s.upper);
  } else if (cmd == "layer") {
    const double Lz = rd(is); int nzg; size_t k; is >> nzg >> k;
    printf("layer");
    for (size_t i = 0; i < k; ++i) printf(" %d", slab_layer_of(rd(is), Lz, nzg).layer);
    printf("\n");
  } else if (cmd == "caps") {
    int nglob, nzg, ncz; is >> nglob >> nzg >> ncz;
    const SlabCaps c = slab_capacities(nglob, nzg, ncz);
    printf("caps %d %d %d\n", c.G, c.mcap, c.cap);
  } else if (cmd == "skin") {
    double L[3] = {rd(is), rd(is), rd(is)}; const double rc = rd(is), skin = rd(is), opt = rd(is);
    int crit, tiles, fused, dd, P, npart; is >> crit >> tiles >> fused >> dd >> P >> npart;
    const double s = pick_list_skin(L, rc, skin, opt, crit, tiles != 0, fused != 0, dd != 0, P, npart);
    unsigned long long b; std::memcpy(&b, &s, 8);
    printf("skin %llu\n", b);
  } else if (cmd == "stride") {
    double L[3] = {rd(is), rd(is), rd(is)}; const double rl = rd(is); int npart, user; is >> npart >> user;
    printf("stride %d\n", row_stride(L, rl, npart, user));
  } else if (cmd == "grow") {
    int ov, nmax; is >> ov >> nmax;
    printf("grow %d %d\n", grown_tile_cap(ov), grown_row_stride(ov, nmax));
  } else if (cmd == "tiles") {
    double L[3] = {rd(is), rd(is), rd(is)}; const double rc = rd(is), skin = rd(is); int n; is >> n; const double opt_skin = rd(is);
    int crit, tiles, fused, split, dd, P, rk; long long slope, budget; is >> crit >> tiles >> fused >> split >> dd >> P >> rk >> slope >> budget;
    const double skin_list = pick_list_skin(L, rc, skin, opt_skin, crit, tiles != 0, fused != 0, dd != 0, P, n);
    const double rl = rc + (skin_list > skin ? skin_list : skin);
    const CellGrid g = cell_grid(L, rl);
    SlabLayers sl{g.nc[2], g.nc[2], 0, 0, 0};
    if (dd) sl = slab_layers(g, P, rk);
    const int S = row_stride(L, rl, n, 0);
    const TilePlan p = plan_tiles(g.nc[0], g.nc[1], sl.ncz, g.nc[2], n, dd != 0, tiles != 0, split,
                                  [&](int cap) { return (size_t)(slope * cap); }, budget > 0 ? (size_t)budget : ~(size_t)0);
    const int ntx = p.use_tiles ? tile_ntx(g.nc[0], p.xs_nb, p.xs_w) : 0;
    printf("tiles %d %d %d %d %d %d %d %d %d %d\n", p.ntiles, g.nc[0], p.use_tiles ? tile_nbx(g.nc[0], p.xs_nb) : 0, p.xs_w, ntx ? p.ntiles / ntx : 0,
           p.tile_cap, p.use_tiles ? 1 : 0, S, sl.z0, sl.ncz);
  } else if (cmd == "xrange") {
    int nx, nb, w; is >> nx >> nb >> w;
    const int ntx = tile_ntx(nx, nb, w);
    printf("xrange %d", ntx);
    for (int tx = 0; tx < ntx; ++tx) { int cx0, hx; tile_xrange(tx, nx, nb, w, cx0, hx); printf(" %d:%d", cx0, hx); }
    printf("\n");
  } else if (cmd == "order") {
    int nc[3], nb, w, ntiles; is >> nc[0] >> nc[1] >> nc[2] >> nb >> w >> ntiles;
    const TileOrder o = tile_order(nc, nb, w, ntiles);
    printf("order %zu", o.ord.size());
    for (int v : o.ord) printf(" %d", v);
    for (int v : o.pos) printf(" %d", v);
    printf("\n");
  } else if (cmd == "shift") {
    int nitem, lo, maxseg; is >> nitem >> lo >> maxseg;
    printf("shift %d\n", segment_shift(nitem, lo, maxseg));
  } else if (cmd == "layers") {
    int ntiles, ntxy, which; is >> ntiles >> ntxy >> which;
    const TileLayers t = tile_subset(ntiles, ntxy, which);
    printf("layers %d %d %d %d\n", t.base1, t.n1, t.base2, t.count);
  } else if (cmd == "overlap") {
    int opt, use, ntiles, ntxy, polls; is >> opt >> use >> ntiles >> ntxy >> polls;
    printf("overlap %d\n", halo_overlap(opt, use != 0, ntiles, ntxy, polls != 0) ? 1 : 0);
  } else if (!cmd.empty()) printf("unknown %s\n", cmd.c_str());
}
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    try { run(cmd, is); }
    catch (const ChemError& e) { printf("error %d %s\n", e.code, e.what()); }
  }
  return 0;
}
