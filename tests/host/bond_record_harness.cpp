// Test harness (CPU only): the host rule of chemlab_amd/csrc/chem_launch_host.hpp that says whether inline bonds may be switched
// on for a staged tile of a given capacity (bond_records_fit: every LDS slot must fit the 16 bits a bond record gives it, below
// the "no partner" mark).  Plain-text script on stdin, one answer per line.  Not part of the product library.
//   none                 "none v"            (kBondRecNone)
//   fit cap              "fit 0|1"           (bond_records_fit of one capacity; cap: any 64-bit integer)
//   scan lo hi           "scan n v1 .. vn"   (every v in (lo, hi] at which the answer differs from that for v - 1)
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_launch_host.hpp"
using namespace chem;
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "none") printf("none %u\n", kBondRecNone);
    else if (cmd == "fit") { long long cap = 0; is >> cap; printf("fit %d\n", bond_records_fit(cap) ? 1 : 0); }
    else if (cmd == "scan") {
      long long lo = 0, hi = 0; is >> lo >> hi;
      std::string out; int n = 0;
      bool prev = bond_records_fit(lo);
      for (long long v = lo + 1; v <= hi; ++v) {
        const bool now = bond_records_fit(v);
        if (now != prev) { out += " " + std::to_string(v); ++n; prev = now; }
      }
      printf("scan %d%s\n", n, out.c_str());
    } else printf("error unknown command\n");
  }
  return 0;
}
