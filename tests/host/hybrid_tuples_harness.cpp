// Test harness (CPU only): drives the hybrid triple and quadruple lists of chemlab_amd/csrc/chem_host.hpp
// (HostList::set_hybrid_tuples, the birth steps kept by list_insert / spawn_tuple / remove_bonds, HostList::lambda_at, the entry
// encoding the device consumes) and their birth arrays through chem_ckpt_host.hpp, from a plain-text script on stdin.  A
// program of its own, so that it can also be built with -fsanitize=address,undefined.  Not part of the product library.
//   n <N>; type <tag> <type>; list <arity> [by_types]
//   reg <list> <t0> <t1> <t2> [<t3>]   a type tuple the topology manager spawns into that list (chem_topology_register)
//   hybrid <list> <lambda0> <rate>     HostList::set_hybrid (pairs), prints "hyb <return code>"
//   hybt <list> <lambda0> <rate>       HostList::set_hybrid_tuples, prints "hybt <return code>"
//   step <s>                           the context's step counter from here on
//   add <list> <tags...>               list_insert alone (chem_list_add of a triple or quadruple), prints "ins 0|1"
//   bonds <list> <k> <a b>...          one reaction step: k pairs inserted, then on_new_bonds over the whole batch
//   remove <k> <list a b unexclude>... one batch through remove_bonds
//   lam <list> <s>                     prints "lam <count>" and one line "<tags...> birth lambda" per entry (birth -1: list keeps none)
//   excl                               prints "excl <count>" and one line "a b" per excluded pair (a < b)
//   entries                            prints "entries <count>" and one line "owner t0 t1 t2 slot pos" per per-tag CSR entry (build_bonded)
//   ckpt <mode> <list>                 the lists through ckpt_write / ckpt_read at step cur_step; mode ok | short (one birth step of
//                                      <list> dropped) | late (its first birth step = step + 1) | early (= -1) | stray (<list> is not
//                                      hybrid and gets one birth step per entry all the same) | hex (as ok, and the blob is printed
//                                      as "hex <bytes>" first); prints "ckpt <rc> <births equal 0|1> <reason>"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_host.hpp"
#include "../../chemlab_amd/csrc/chem_ckpt_host.hpp"
using namespace chem;
int main() {
  HostTopology t;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "n") { is >> t.n; t.type.assign(t.n, 0); t.res_id.resize(t.n); t.mol_id.resize(t.n); t.mass.assign(t.n, 1.0); t.q.assign(t.n, 0.0);
      t.state.assign(t.n, 0); t.graph.assign(t.n, TagRow()); t.excl.assign(t.n, TagRow());
      for (int64_t i = 0; i < t.n; ++i) { t.res_id[i] = (int32_t)i + 1; t.mol_id[i] = (int32_t)i; } }
    else if (cmd == "type") { int tg, ty; is >> tg >> ty; t.type[tg] = ty; }
    else if (cmd == "list") { int ar, bt = 0; is >> ar >> bt; HostList l; l.arity = ar; l.kind = 1; l.by_types = bt; l.has_plain = !bt; t.lists.push_back(l); }
    else if (cmd == "reg") {
      int li; is >> li; HostList& l = t.lists[li];
      std::array<int, 4> key{-1, -1, -1, -1};
      for (int k = 0; k < l.arity; ++k) is >> key[k];
      l.registered.push_back(key);
      if (l.by_types) l.typed[key] = {};
    }
    else if (cmd == "hybrid") { int li; std::string a, b; is >> li >> a >> b; printf("hyb %d\n", t.lists[li].set_hybrid(std::stod(a), std::stod(b))); }
    else if (cmd == "hybt") { int li; std::string a, b; is >> li >> a >> b; printf("hybt %d\n", t.lists[li].set_hybrid_tuples(std::stod(a), std::stod(b))); }
    else if (cmd == "step") { is >> t.cur_step; }
    else if (cmd == "add") {
      int li; is >> li; int32_t p[4] = {0, 0, 0, 0};
      for (int k = 0; k < t.lists[li].arity; ++k) is >> p[k];
      printf("ins %d\n", t.list_insert(t.lists[li], p) ? 1 : 0);
    } else if (cmd == "bonds") {
      int li, k; is >> li >> k;
      std::vector<std::pair<int32_t, int32_t>> nb;
      for (int i = 0; i < k; ++i) { int32_t p[2]; is >> p[0] >> p[1]; if (t.list_insert(t.lists[li], p)) nb.emplace_back(p[0], p[1]); }
      std::vector<int32_t> touched; t.on_new_bonds(nb, touched);
    } else if (cmd == "remove") {
      int k; is >> k; std::vector<HostTopology::BrokenBond> bb;
      for (int i = 0; i < k; ++i) { HostTopology::BrokenBond b{}; is >> b.list >> b.a >> b.b >> b.unexclude; bb.push_back(b); }
      std::vector<int32_t> touched; t.remove_bonds(bb, touched);
    } else if (cmd == "lam") {
      int li; long long s; is >> li >> s;
      const HostList& l = t.lists[li];
      printf("lam %lld\n", (long long)l.size());
      if ((int64_t)l.birth.size() != (l.hybrid ? l.size() : 0)) { printf("birth array out of step: %zu\n", l.birth.size()); return 1; }
      for (int64_t e = 0; e < l.size(); ++e) {
        for (int k = 0; k < l.arity; ++k) printf("%d ", l.ent[l.arity * e + k]);
        printf("%lld %.17g\n", l.hybrid ? (long long)l.birth[e] : -1ll, l.lambda_at((size_t)e, s));
      }
    } else if (cmd == "excl") {
      printf("excl %lld\n", (long long)t.n_excl_pairs);
      for (int64_t a = 0; a < t.n; ++a) for (int32_t b : t.excl[a]) if (a < b) printf("%lld %d\n", (long long)a, b);
    } else if (cmd == "entries") {
      std::vector<int32_t> bstart; std::vector<HBondedEntry> bent; std::vector<HBondedParam> bp;
      t.build_bonded(bstart, bent, bp);
      printf("entries %zu\n", bent.size());
      for (int64_t o = 0; o < t.n; ++o)
        for (int32_t e = bstart[o]; e < bstart[o + 1]; ++e) printf("%lld %d %d %d %d %d\n", (long long)o, bent[e].t0, bent[e].t1, bent[e].t2, bonded_slot(bent[e].meta), bonded_member(bent[e].meta));
    } else if (cmd == "ckpt") {
      std::string mode; int li; is >> mode >> li;
      CkptFingerprint fp; fp.npart = t.n;
      CkptState s; s.step = t.cur_step; s.L[0] = s.L[1] = s.L[2] = 10.0;
      for (int64_t i = 0; i < t.n; ++i) {
        s.id.push_back(i + 1); s.type.push_back(t.type[i]); s.state.push_back(0); s.res_id.push_back(t.res_id[i]); s.mol_id.push_back(t.mol_id[i]); s.mass.push_back(1.0); s.q.push_back(0.0);
        for (int d = 0; d < 3; ++d) { s.pos.push_back(0.5 * (double)i); s.image.push_back(0); s.vel.push_back(0.0); }
      }
      for (const HostList& l : t.lists) {
        fp.lists.push_back(CkptListKind{l.arity, l.kind, l.by_types, l.hybrid ? 1 : 0});
        CkptState::List c; c.ent = l.ent; if (l.hybrid) c.birth = l.birth;
        s.lists.push_back(c);
      }
      if (mode == "short") s.lists[li].birth.pop_back();
      else if (mode == "late") s.lists[li].birth[0] = s.step + 1;
      else if (mode == "early") s.lists[li].birth[0] = -1;
      else if (mode == "stray") s.lists[li].birth.assign((size_t)t.lists[li].size(), 0);
      const std::vector<uint8_t> blob = ckpt_write(64, fp, s);
      if (mode == "hex") { printf("hex "); for (uint8_t b : blob) printf("%02x", b); printf("\n"); }
      std::unique_ptr<uint8_t[]> exact(new uint8_t[blob.size()]);      // exactly nbytes: the sanitizer sees any read beyond
      std::memcpy(exact.get(), blob.data(), blob.size());
      CkptState got; std::string why;
      const int rc = ckpt_read(exact.get(), (int64_t)blob.size(), 64, fp, got, why);
      bool same = rc == 0 && got.lists.size() == t.lists.size();
      for (size_t l = 0; same && l < t.lists.size(); ++l) same = got.lists[l].ent == t.lists[l].ent && got.lists[l].birth == (t.lists[l].hybrid ? t.lists[l].birth : std::vector<int64_t>());
      printf("ckpt %d %d %s\n", rc, same ? 1 : 0, why.c_str());
    }
  }
  return 0;
}
