// rdf_harness.cpp -- drives chem_rdf_host.hpp (radial distribution functions: edges, the bin of a squared distance, selector
// masks, the normaliser M, validation and the launch plan) from stdin for tests/test_host_rdf.py.  Plain C++: built with g++,
// also with -fsanitize=address,undefined, as a stand-alone program.  Doubles travel as their decimal bit patterns.
//
//   edge2 dr nbins k                          -> "edge2 <bits of e2[k]>"
//   bin dr nbins d2                           -> "bin k"   (-1: not counted)
//   mask nsel t1 t2 ... a b                   -> "mask m"  (bit s: selector s counts a pair of types a, b)
//   norm nsel t1 t2 ... c0 .. c15             -> "norm M0 M1 ..."
//   valid r_max nbins npairs t1 t2 ...        -> "valid rc"
//   plan path nbins nsel parts image budget ncu work -> "plan ok grid block hist_off lds_bytes" or "plan refused"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../chemlab_amd/csrc/chem_rdf_host.hpp"

using namespace chem;

static double rd(std::istringstream& in) {
  unsigned long long b = 0;
  in >> b;
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
static unsigned long long bits(double d) {
  unsigned long long b;
  std::memcpy(&b, &d, 8);
  return b;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "edge2") {
      const double dr = rd(in);
      int nbins = 0, k = 0;
      in >> nbins >> k;
      std::printf("edge2 %llu\n", bits(rdf_edge2(k, dr)));
    } else if (cmd == "bin") {
      const double dr = rd(in);
      int nbins = 0;
      in >> nbins;
      const double d2 = rd(in);
      std::printf("bin %d\n", rdf_bin(d2, dr, 1.0 / dr, nbins));
    } else if (cmd == "mask" || cmd == "norm") {
      int nsel = 0;
      in >> nsel;
      std::vector<int32_t> tp(2 * (size_t)(nsel > 0 ? nsel : 0));
      for (auto& t : tp) in >> t;
      unsigned char mask[CHEM_MAX_TYPES][CHEM_MAX_TYPES];
      rdf_fill_masks(nsel, tp.data(), mask);
      if (cmd == "mask") {
        int a = 0, b = 0;
        in >> a >> b;
        std::printf("mask %d\n", (a >= 0 && a < CHEM_MAX_TYPES && b >= 0 && b < CHEM_MAX_TYPES) ? (int)mask[a][b] : -1);
      } else {
        long long c[CHEM_MAX_TYPES];
        for (auto& v : c) in >> v;
        std::printf("norm");
        for (int s = 0; s < nsel; ++s) std::printf(" %llu", rdf_norm_pairs(mask, s, c));
        std::printf("\n");
      }
    } else if (cmd == "valid") {
      const double r_max = rd(in);
      int nbins = 0, npairs = 0;
      in >> nbins >> npairs;
      std::vector<int32_t> tp;
      int32_t t;
      while (in >> t) tp.push_back(t);
      tp.resize(2 * (size_t)(npairs > 0 && npairs <= kRdfMaxPairs ? npairs : 0), 0);
      std::string why;
      const int rc = rdf_validate(r_max, nbins, npairs, tp.empty() ? nullptr : tp.data(), why);
      std::printf("valid %d\n", rc);
    } else if (cmd == "plan") {
      int path = 0, nbins = 0, nsel = 0, parts = 0, ncu = 0;
      unsigned long long image = 0, budget = 0;
      long long work = 0;
      in >> path >> nbins >> nsel >> parts >> image >> budget >> ncu >> work;
      RdfPlan p{};
      std::string why;
      if (rdf_plan(path, nbins, nsel, parts, (size_t)image, (size_t)budget, ncu, work, p, why)) std::printf("plan ok %d %d %zu %zu\n", p.grid, p.block, p.hist_off, p.lds_bytes);
      else std::printf("plan refused\n");
    } else {
      std::printf("unknown\n");
    }
  }
  return 0;
}
