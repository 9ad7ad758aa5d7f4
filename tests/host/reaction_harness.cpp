// Test harness (CPU only): drives the host algorithms of the reaction step in chemlab_amd/csrc/chem_react_host.hpp
// (build_restrict_csr, constraint_bits, sort_bond_events, trim_accepted, atrp_select) from a plain-text script on stdin
// and prints what they return, so that a pytest can compare it with a brute-force model.  Not part of the product library.
//   sort <m> <a b>...                      events (r = input index) through sort_bond_events; prints "a b r" per event
//   trim <nearest> <cap> <m> <a h d2bits status>...   d2 as the decimal bit pattern of the double; prints changed + statuses
//   csr <n> <m> <lo hi mask>...            prints start, partner and mask rows
//   n <N>; type <tag> <t>; state <tag> <s>; edge <a> <b>; reaction <type_1> <type_2>;
//   constraint <role> <nb_type> <min_state> <max_state>     one per reaction row, in order
//   cons                                   prints constraint_bits, one word per particle
//   atrp <num_particles> <select_from_all> <ratio_act> <ratio_deact> <delta_catalyst> <k_act> <k_deact> <seed>
//   center <type> <state> <is_activator> <new_type> <delta_state> <new_mass> <new_q>
//   fire <step>                            one atrp_select; prints the stats row, the changes and the mirrors
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_react_host.hpp"
using namespace chem;
struct Rec { int a, b, r; unsigned int h; double d2; };   // layout of the device's candidate / event record
int main() {
  HostTopology t;
  std::vector<chem_reaction_desc> reactions;
  std::vector<NbCons> constraints;
  chem_atrp_desc atrp{};
  std::vector<AtrpCenter> centers;
  std::vector<Rec> scratch;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "sort") {
      size_t m; is >> m; std::vector<Rec> ev(m);
      for (size_t k = 0; k < m; ++k) { is >> ev[k].a >> ev[k].b; ev[k].r = (int)k; ev[k].h = 0; ev[k].d2 = 0; }
      sort_bond_events(ev, scratch);
      printf("sorted %zu\n", ev.size());
      for (auto& e : ev) printf("%d %d %d\n", e.a, e.b, e.r);
    } else if (cmd == "trim") {
      int nearest; long long cap; size_t m; is >> nearest >> cap >> m;
      std::vector<Rec> rec(m); std::vector<int> st(m);
      for (size_t k = 0; k < m; ++k) { unsigned long long bits; is >> rec[k].a >> rec[k].h >> bits >> st[k]; std::memcpy(&rec[k].d2, &bits, 8); rec[k].b = 0; rec[k].r = 0; }
      const bool ch = trim_accepted(rec, st, cap, nearest != 0);
      printf("trim %d", ch ? 1 : 0);
      for (int s : st) printf(" %d", s);
      printf("\n");
    } else if (cmd == "csr") {
      int n; size_t m; is >> n >> m; std::map<std::pair<int32_t, int32_t>, uint32_t> mp;
      for (size_t k = 0; k < m; ++k) { int lo, hi; unsigned mask; is >> lo >> hi >> mask; mp[{lo, hi}] |= mask; }
      const RestrictCsr c = build_restrict_csr(mp, n);
      printf("start"); for (int v : c.start) printf(" %d", v); printf("\n");
      printf("partner"); for (int v : c.partner) printf(" %d", v); printf("\n");
      printf("mask"); for (unsigned v : c.mask) printf(" %u", v); printf("\n");
    } else if (cmd == "n") {
      is >> t.n; t.type.assign(t.n, 0); t.state.assign(t.n, 0); t.mass.assign(t.n, 1.0); t.q.assign(t.n, 0.0); t.graph.assign(t.n, TagRow());
    } else if (cmd == "type") { int a, b; is >> a >> b; t.type[a] = b; }
    else if (cmd == "state") { int a, b; is >> a >> b; t.state[a] = b; }
    else if (cmd == "edge") { int a, b; is >> a >> b; t.graph_add(a, b); }
    else if (cmd == "reaction") { chem_reaction_desc d{}; is >> d.type_1 >> d.type_2; reactions.push_back(d); }
    else if (cmd == "constraint") { NbCons c; is >> c.role >> c.nb_type >> c.min_state >> c.max_state; constraints.push_back(c); }
    else if (cmd == "cons") {
      printf("cons");
      for (unsigned v : constraint_bits(t, reactions, constraints)) printf(" %u", v);
      printf("\n");
    } else if (cmd == "atrp") {
      is >> atrp.num_particles >> atrp.select_from_all >> atrp.ratio_activator >> atrp.ratio_deactivator >> atrp.delta_catalyst >> atrp.k_activate >> atrp.k_deactivate >> atrp.seed;
    } else if (cmd == "center") {
      AtrpCenter c{}; is >> c.type >> c.state >> c.is_activator >> c.new_type >> c.delta_state >> c.new_mass >> c.new_q; centers.push_back(c);
    } else if (cmd == "fire") {
      long long step; is >> step;
      const AtrpOutcome o = atrp_select(t, atrp, centers, step);
      const chem_atrp_stats& s = o.stats;
      printf("stats %lld %lld %lld %lld %lld %.17g %.17g %d\n", (long long)s.step, (long long)s.candidates, (long long)s.selected, (long long)s.activated,
             (long long)s.deactivated, s.ratio_activator, s.ratio_deactivator, o.types_changed ? 1 : 0);
      printf("ratios %.17g %.17g\n", atrp.ratio_activator, atrp.ratio_deactivator);
      printf("changes %zu\n", o.changes.size());
      for (auto& c : o.changes) printf("%d %d %d %d %.17g %.17g\n", c.tag, c.type, c.set_state, c.state, c.mass, c.q);
      printf("mirrors");
      for (int64_t i = 0; i < t.n; ++i) printf(" %d:%d", t.type[i], t.state[i]);
      printf("\n");
    }
  }
  return 0;
}
