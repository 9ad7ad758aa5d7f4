// Test harness (CPU only): drives the pure fixed-distance routines of chemlab_amd/csrc/chem_fix_host.hpp (FixState: add with
// validation, release by reaction and by type, compaction, the log, the device order) from a plain-text script on stdin.  A
// program of its own, so that it can also be built with -fsanitize=address,undefined.  Not part of the product library.
//   ntags <N>                                   number of particles (tags 0 .. N-1; -1 stands for an unknown id)
//   create <anchor_type> <target_type>          prints "set <handle | error code>"
//   add <set> <dist> <n> <a t>...               prints "add <0 | error code>"
//   rule <reaction> <role> <set> <count>
//   types <t0> <t1> ...                         the type mirror (N values)
//   settype <tag> <type>
//   react <step> <k> <reaction role tag>...     release_by_reaction; prints "rel <count>" and one line "<step> <set> <a> <t> <cause>" per record
//   bytype <step>                               release_by_type on the type mirror; prints as react
//   get <set>                                   prints "get <count>" and one line "<a> <t> <dist> <seq>" per live entry
//   log                                         prints "log <count>" and one line per record
//   order                                       prints "order <a:t> ..." (the flat device order)
//   count                                       prints "count <live entries of all sets> <targets> <anchors>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../chemlab_amd/csrc/chem_fix_host.hpp"
using namespace chem;
static void print_records(const char* head, const std::vector<FixRecord>& r) {
  printf("%s %zu\n", head, r.size());
  for (const FixRecord& x : r) printf("%lld %d %d %d %d\n", (long long)x.step, x.set, x.anchor, x.target, x.cause);
}
int main() {
  FixState fs;
  std::vector<int32_t> type;
  long long ntags = 0;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "ntags") { is >> ntags; type.assign((size_t)ntags, 0); }
    else if (cmd == "create") { int a, t; is >> a >> t; printf("set %d\n", fs.create(a, t)); }
    else if (cmd == "add") {
      int set; std::string ds; long long n; is >> set >> ds >> n;
      std::vector<int32_t> p((size_t)(2 * n));
      for (auto& v : p) is >> v;
      std::string why;
      const int rc = fs.add(set, n, p.data(), std::stod(ds), ntags, why);
      printf("add %d\n", rc);
      if ((rc != 0) != !why.empty()) { printf("refusal without a reason\n"); return 1; }
    }
    else if (cmd == "rule") { FixRule r; is >> r.reaction >> r.role >> r.set >> r.count; fs.rules.push_back(r); }
    else if (cmd == "types") { for (auto& v : type) is >> v; }
    else if (cmd == "settype") { int i, t; is >> i >> t; type[(size_t)i] = t; }
    else if (cmd == "react") {
      long long step; int k; is >> step >> k;
      std::vector<FixReactant> rc((size_t)k);
      for (auto& r : rc) is >> r.reaction >> r.role >> r.tag;
      print_records("rel", fs.release_by_reaction(rc, step));
    }
    else if (cmd == "bytype") { long long step; is >> step; print_records("rel", fs.release_by_type(type, step)); }
    else if (cmd == "get") {
      int set; is >> set;
      const FixSet& s = fs.sets[(size_t)set];
      printf("get %zu\n", s.ent.size());
      for (const FixEntry& e : s.ent) printf("%d %d %.17g %lld\n", e.anchor, e.target, e.dist, (long long)e.seq);
    }
    else if (cmd == "log") print_records("log", fs.log);
    else if (cmd == "order") { printf("order"); for (const FixEntry& e : fs.device_order()) printf(" %d:%d", e.anchor, e.target); printf("\n"); }
    else if (cmd == "count") printf("count %lld %zu %zu\n", (long long)fs.count(), fs.targets.size(), fs.anchors.size());
  }
  return 0;
}
