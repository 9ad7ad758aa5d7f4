// Test harness (CPU only): drives the hybrid pair lists of chemlab_amd/csrc/chem_host.hpp (HostList::set_hybrid, the birth
// steps kept by list_insert / push_pair / remove_bonds, HostList::lambda_at, the entry and slot encoding the device consumes)
// from a plain-text script on stdin.  A program of its own, so that it can also be built with -fsanitize=address,undefined.
// Not part of the product library.
//   n <N>; list <arity> [by_types]
//   hybrid <list> <lambda0> <rate>   prints "hyb <return code>"
//   step <s>                         the context's step counter from here on
//   bond <list> <a> <b>              list_insert + on_new_bonds, prints "ins 0|1"
//   push <list> <a> <b>              HostList::push_pair (the reaction step's deferred insert)
//   remove <k> <list a b unexclude>...   one batch through remove_bonds
//   lam <list> <s>                   prints "lam <count>" and one line "a b birth lambda" per entry (birth -1: list keeps none)
//   slots                            prints "slots <count>" and one line "list pad lambda0 rate" per parameter slot
//   entries                          prints "entries <count>" and one line "t0 t1 t2 slot pos" per per-tag CSR entry (build_bonded)
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_host.hpp"
using namespace chem;
int main() {
  HostTopology t;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "n") { is >> t.n; t.type.assign(t.n, 0); t.res_id.resize(t.n); t.mol_id.resize(t.n); t.mass.assign(t.n, 1.0); t.q.assign(t.n, 0.0);
      t.graph.assign(t.n, TagRow()); t.excl.assign(t.n, TagRow());
      for (int64_t i = 0; i < t.n; ++i) { t.res_id[i] = (int32_t)i + 1; t.mol_id[i] = (int32_t)i; } }
    else if (cmd == "list") { int ar, bt = 0; is >> ar >> bt; HostList l; l.arity = ar; l.kind = 1; l.by_types = bt; l.has_plain = !bt;
      if (bt) l.typed[std::array<int, 4>{0, 0, ar > 2 ? 0 : -1, -1}] = {};
      t.lists.push_back(l); }
    else if (cmd == "hybrid") { int li; std::string a, b; is >> li >> a >> b; printf("hyb %d\n", t.lists[li].set_hybrid(std::stod(a), std::stod(b))); }
    else if (cmd == "step") { is >> t.cur_step; }
    else if (cmd == "bond") {
      int li; int32_t p[2]; is >> li >> p[0] >> p[1];
      const bool ins = t.list_insert(t.lists[li], p);
      if (ins) { std::vector<std::pair<int32_t, int32_t>> nb{{p[0], p[1]}}; std::vector<int32_t> touched; t.on_new_bonds(nb, touched); }
      printf("ins %d\n", ins ? 1 : 0);
    } else if (cmd == "push") {
      int li; int32_t p[2]; is >> li >> p[0] >> p[1];
      t.lists[li].push_pair(p, t.cur_step); t.lists[li].seen.insert(tuple_key(p, 2));
      std::vector<std::pair<int32_t, int32_t>> nb{{p[0], p[1]}}; std::vector<int32_t> touched; t.on_new_bonds(nb, touched);
    } else if (cmd == "remove") {
      int k; is >> k; std::vector<HostTopology::BrokenBond> bb;
      for (int i = 0; i < k; ++i) { HostTopology::BrokenBond b{}; is >> b.list >> b.a >> b.b >> b.unexclude; bb.push_back(b); }
      std::vector<int32_t> touched; t.remove_bonds(bb, touched);
    } else if (cmd == "lam") {
      int li; long long s; is >> li >> s;
      const HostList& l = t.lists[li];
      printf("lam %lld\n", (long long)l.size());
      if (l.hybrid && (int64_t)l.birth.size() != l.size()) { printf("birth array out of step: %zu\n", l.birth.size()); return 1; }
      for (int64_t e = 0; e < l.size(); ++e)
        printf("%d %d %lld %.17g\n", l.ent[2 * e], l.ent[2 * e + 1], l.hybrid ? (long long)l.birth[e] : -1ll, l.lambda_at((size_t)e, s));
    } else if (cmd == "slots") {
      std::vector<HBondedParam> bp; std::vector<HostTopology::HSlotKey> keys; std::vector<std::array<double, 2>> hyb;
      t.build_params(bp, keys); t.hybrid_params(bp, hyb);
      printf("slots %zu\n", bp.size());
      for (size_t s = 0; s < bp.size(); ++s) printf("%d %d %d %.17g %.17g\n", bp[s].list, bp[s].pad, keys[s].pad, hyb[s][0], hyb[s][1]);
    } else if (cmd == "entries") {
      std::vector<int32_t> bstart; std::vector<HBondedEntry> bent; std::vector<HBondedParam> bp;
      t.build_bonded(bstart, bent, bp);
      printf("entries %zu\n", bent.size());
      for (auto& e : bent) printf("%d %d %d %d %d\n", e.t0, e.t1, e.t2, bonded_slot(e.meta), bonded_member(e.meta));
    }
  }
  return 0;
}
