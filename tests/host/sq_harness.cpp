// sq_harness.cpp -- drives chem_sq_host.hpp (static structure factor: the enumeration of the wave vectors and its inverse,
// validation, the selector -> class table and the launch plan) from stdin for tests/test_host_sq.py.  Plain C++: built with g++,
// also with -fsanitize=address,undefined, as a stand-alone program.
//
//   nvec nmax                                 -> "nvec N"
//   enum nmax                                 -> "enum N bad": every k in 0..nvec-1 through sq_vec, then back through sq_index; bad
//                                                counts k whose vector is not kept, out of range, not the successor of the one
//                                                before in lexicographic order, or does not map back to k
//   vec nmax k                                -> "vec nx ny nz"
//   index nmax nx ny nz                       -> "index k"   (-1: not a kept vector of this nmax)
//   valid nmax npairs [null] t1 t2 ...        -> "valid rc"
//   classes npairs t1 t2 ...                  -> "classes ncls c0 .. | a0 b0 a1 b1 .. | tmask[0] .. tmask[15]"
//   count npairs t1 t2 ... c0 .. c15          -> "count na0 nb0 na1 nb1 ..."
//   plan n nmax ncls budget ncu               -> "plan ok nqb nsuper per block lds_bytes scratch_bytes cap_bytes" or "plan refused"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../chemlab_amd/csrc/chem_sq_host.hpp"

using namespace chem;

static std::vector<int32_t> read_pairs(std::istringstream& in, int npairs) {
  std::vector<int32_t> tp(2 * (size_t)(npairs > 0 ? npairs : 0));
  for (auto& t : tp) in >> t;
  return tp;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "nvec") {
      int nmax = 0;
      in >> nmax;
      std::printf("nvec %lld\n", sq_nvec(nmax));
    } else if (cmd == "enum") {
      int nmax = 0;
      in >> nmax;
      const long long nv = sq_nvec(nmax);
      long long bad = 0;
      int px = 0, py = 0, pz = 0;
      for (long long k = 0; k < nv; ++k) {
        int nx = 99, ny = 99, nz = 99;
        sq_vec(k, nmax, nx, ny, nz);
        const bool in_range = nx >= -nmax && nx <= nmax && ny >= -nmax && ny <= nmax && nz >= -nmax && nz <= nmax;
        const bool after = k == 0 || nx > px || (nx == px && (ny > py || (ny == py && nz > pz)));
        if (!in_range || !sq_kept(nx, ny, nz) || !after || sq_index(nx, ny, nz, nmax) != k) ++bad;
        px = nx; py = ny; pz = nz;
      }
      std::printf("enum %lld %lld\n", nv, bad);
    } else if (cmd == "vec") {
      int nmax = 0, nx = 0, ny = 0, nz = 0;
      long long k = 0;
      in >> nmax >> k;
      sq_vec(k, nmax, nx, ny, nz);
      std::printf("vec %d %d %d\n", nx, ny, nz);
    } else if (cmd == "index") {
      int nmax = 0, nx = 0, ny = 0, nz = 0;
      in >> nmax >> nx >> ny >> nz;
      std::printf("index %lld\n", sq_index(nx, ny, nz, nmax));
    } else if (cmd == "valid") {
      int nmax = 0, npairs = 0;
      in >> nmax >> npairs;
      std::vector<int32_t> tp;
      std::string tok;
      bool null = false;
      while (in >> tok) { if (tok == "null") null = true; else tp.push_back((int32_t)std::stoi(tok)); }
      tp.resize(2 * (size_t)(npairs > 0 && npairs <= kSqMaxPairs ? npairs : 0), 0);
      std::string why;
      std::printf("valid %d\n", sq_validate(nmax, npairs, null || tp.empty() ? nullptr : tp.data(), why));
    } else if (cmd == "classes" || cmd == "count") {
      int npairs = 0;
      in >> npairs;
      if (npairs < 0 || npairs > kSqMaxPairs) { std::printf("%s refused\n", cmd.c_str()); continue; }
      const std::vector<int32_t> tp = read_pairs(in, npairs);
      SqArgs a;
      sq_fill_classes(3, npairs, tp.data(), a);
      if (cmd == "classes") {
        std::printf("classes %d", a.ncls);
        for (int c = 0; c < a.ncls; ++c) std::printf(" %d", a.cls[c]);
        std::printf(" |");
        for (int s = 0; s < npairs; ++s) std::printf(" %d %d", a.sel_a[s], a.sel_b[s]);
        std::printf(" |");
        for (int t = 0; t < CHEM_MAX_TYPES; ++t) std::printf(" %d", (int)a.tmask[t]);
        std::printf("\n");
      } else {
        long long c[CHEM_MAX_TYPES];
        for (auto& v : c) in >> v;
        std::printf("count");
        for (int s = 0; s < npairs; ++s) std::printf(" %lld %lld", sq_class_count(a, a.sel_a[s], c), sq_class_count(a, a.sel_b[s], c));
        std::printf("\n");
      }
    } else if (cmd == "plan") {
      long long n = 0;
      int nmax = 0, ncls = 0, ncu = 0;
      unsigned long long budget = 0;
      in >> n >> nmax >> ncls >> budget >> ncu;
      SqPlan p{};
      std::string why;
      if (sq_plan(n, nmax, ncls, (size_t)budget, ncu, p, why))
        std::printf("plan ok %d %d %d %d %zu %zu %zu\n", p.nqb, p.nsuper, p.per, p.block, p.lds_bytes, p.scratch_bytes,
                    (size_t)sq_super_cap(nmax, ncls, ncu) * sq_partial_bytes(nmax, ncls));
      else std::printf("plan refused\n");
    } else {
      std::printf("unknown\n");
    }
  }
  return 0;
}
