// region_harness.cpp -- drives chem_region_host.hpp (region rules: box test, firing rule, selection, validation) from stdin for
// tests/test_host_region.py.  Plain C++: built with g++, also with -fsanitize=address,undefined, as a stand-alone program.
//
//   rule lo0 lo1 lo2 hi0 hi1 hi2 target new interval mode value num seed enabled   -> "rule <rc or index>"
//   fire step L0 L1 L2 n, then n lines "tag type x y z"     -> "chg m" + m lines "step tag rule", "stat k" + k lines
//                                                              "step rule candidates changed", "types" + the n types
//   quota mode value num ncand naccept                       -> "quota q"
// The records are formed as the scan kernel forms them: a particle is recorded when it is a candidate of at least one due rule
// under its current type, with the bits of every due rule whose box holds it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../chemlab_amd/csrc/chem_region_host.hpp"

using namespace chem;

int main() {
  std::vector<chem_region_desc> rules;
  std::vector<uint8_t> enabled;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "rule") {
      chem_region_desc d{};
      int en = 0;
      unsigned long long seed = 0;
      in >> d.lo[0] >> d.lo[1] >> d.lo[2] >> d.hi[0] >> d.hi[1] >> d.hi[2] >> d.target_type >> d.new_type >> d.interval >> d.mode >> d.value >> d.num >> seed >> en;
      d.seed = seed; d.new_mass = -1.0;
      std::string why;
      const int rc = region_validate(d, why);
      if (rc != 0) { std::printf("rule %d\n", rc); continue; }
      rules.push_back(d); enabled.push_back((uint8_t)(en != 0));
      std::printf("rule %d\n", (int)rules.size() - 1);
    } else if (cmd == "fire") {
      long long step = 0; double L[3]; int n = 0;
      in >> step >> L[0] >> L[1] >> L[2] >> n;
      std::vector<int> tags(n), types(n);
      std::vector<RegionCand> recs;
      for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream pin(line);
        double x[3];
        pin >> tags[i] >> types[i] >> x[0] >> x[1] >> x[2];
        for (int d = 0; d < 3; ++d) x[d] = region_fold(x[d], L[d]);
        RegionCand c{tags[i], types[i], 0u, 0u};
        bool cand = false;
        for (size_t k = 0; k < rules.size(); ++k) {
          if (!region_due(rules[k], enabled[k] != 0, step) || !region_inside(rules[k].lo, rules[k].hi, x[0], x[1], x[2])) continue;
          c.inbox |= 1u << k;
          cand |= rules[k].target_type == types[i];
        }
        if (cand) recs.push_back(c);
      }
      std::vector<RegionChange> chg;
      std::vector<RegionStat> st;
      region_fire(rules, enabled, step, recs, chg, st);
      std::printf("chg %zu\n", chg.size());
      for (const RegionChange& c : chg) std::printf("%lld %d %d\n", (long long)c.step, c.tag, c.rule);
      std::printf("stat %zu\n", st.size());
      for (const RegionStat& s : st) std::printf("%lld %d %lld %lld\n", (long long)s.step, s.rule, (long long)s.candidates, (long long)s.changed);
      for (const RegionCand& r : recs) for (int i = 0; i < n; ++i) if (tags[i] == r.tag) types[i] = r.type;
      std::printf("types");
      for (int i = 0; i < n; ++i) std::printf(" %d", types[i]);
      std::printf("\n");
    } else if (cmd == "quota") {
      int mode = 0, num = 0; double value = 0; long long nc = 0, na = 0;
      in >> mode >> value >> num >> nc >> na;
      std::printf("quota %lld\n", region_quota(mode, value, num, nc, na));
    }
  }
  return 0;
}
