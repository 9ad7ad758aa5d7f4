// Test harness (CPU only): drives the host rule of chemlab_amd/csrc/chem_launch_host.hpp -- which force kernel runs, or why none
// does -- from a plain-text script on stdin, one answer per line, so that a pytest can compare it with a model of its own.  Not
// part of the product library.
//   plan use_tiles n opt_tpp pair_bs energy coul res cap lj_only uniform_lj cubic_tab diag res_a res_b cap_a cap_b
//        "ok <t|r> mode tpp block energy diag cubic member"   (member: variant_built of the answer)   or   "refuse code text..."
//   tiles_built / tiles_unlaunched / rows_built      the sets, one line: "mode:tpp:block:energy:diag ..." / "mode:tpp:cubic ..."
//   respair m0 .. m15                                 "pair a b"   (first_res_pair of the 16 mask words)
//   cappair k a1 b1 .. ak bk                          "pair a b"   (first_cap_pair with those entries capped, as given: not mirrored)
//   bonded nbent inline excl_over work_list coul14 hybrid bonds_only nb_owner      "bonded <none|work|each> <plain|hybrid|charged> bonds_only inline nown"
//   kind coul14 hybrid                                "kind <plain|hybrid|charged>"   (bonded_kind: the family rule on its own)
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_launch_host.hpp"
using namespace chem;
static bool rb(std::istream& is) { int v = 0; is >> v; return v != 0; }
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "plan") {
      PairInput in{};
      in.use_tiles = rb(is); is >> in.n >> in.opt_tpp >> in.pair_bs;
      in.energy = rb(is); in.coul = rb(is); in.res = rb(is); in.cap = rb(is); in.lj_only = rb(is); in.uniform_lj = rb(is); in.cubic_tab = rb(is); in.diag = rb(is);
      is >> in.res_a >> in.res_b >> in.cap_a >> in.cap_b;
      const PairPlan p = pair_plan(in);
      if (p.code != CHEM_OK) printf("refuse %d %s\n", p.code, pair_refusal_text(p).c_str());
      else printf("ok %c %d %d %d %d %d %d %d\n", p.v.family == PairFamily::tiles ? 't' : 'r', p.v.mode, p.v.tpp, p.v.block, p.v.energy ? 1 : 0, p.v.diag ? 1 : 0,
                  p.v.cubic ? 1 : 0, variant_built(p.v) ? 1 : 0);
    } else if (cmd == "tiles_built") {
      printf("tiles");
      for_each_tile_variant([](const PairVariant& v) { printf(" %d:%d:%d:%d:%d", v.mode, v.tpp, v.block, v.energy ? 1 : 0, v.diag ? 1 : 0); });
      printf("\n");
    } else if (cmd == "tiles_unlaunched") {
      printf("tiles");
      for (int m = -1; m < 9; ++m) for (int t = 0; t <= 64; ++t) for (int b : {64, 128, 256, 512, 1024, 2048}) for (int e = 0; e < 2; ++e) for (int d = 0; d < 2; ++d)
        if (tile_variant_unlaunched(m, t, b, e != 0, d != 0)) printf(" %d:%d:%d:%d:%d", m, t, b, e, d);
      printf("\n");
    } else if (cmd == "rows_built") {
      printf("rows");
      for (int m = -1; m < 9; ++m) for (int t = 0; t <= 128; ++t) for (int c = 0; c < 2; ++c) if (row_variant_built(m, t, c != 0)) printf(" %d:%d:%d", m, t, c);
      printf("\n");
    } else if (cmd == "respair") {
      uint32_t mask[CHEM_MAX_TYPES] = {};
      for (auto& m : mask) is >> m;
      int a = -1, b = -1; first_res_pair(mask, a, b);
      printf("pair %d %d\n", a, b);
    } else if (cmd == "cappair") {
      double cap[CHEM_MAX_TYPES][CHEM_MAX_TYPES] = {};
      int k = 0; is >> k;
      for (int i = 0; i < k; ++i) { int a = 0, b = 0; is >> a >> b; cap[a][b] = 0.5; }
      int a = -1, b = -1; first_cap_pair(cap, a, b);
      printf("pair %d %d\n", a, b);
    } else if (cmd == "bonded") {
      BondedInput in{};
      is >> in.nbent; in.inline_bonds = rb(is); is >> in.excl_over; in.work_list = rb(is); in.has_coul14 = rb(is); in.has_hybrid = rb(is); in.bonds_only = rb(is); is >> in.nb_owner;
      const BondedPlan p = bonded_plan(in);
      printf("bonded %s %s %d %d %d\n", p.launch == BondedLaunch::none ? "none" : p.launch == BondedLaunch::work_list ? "work" : "each",
             p.kind == BondedKind::plain ? "plain" : p.kind == BondedKind::hybrid ? "hybrid" : "charged", p.bonds_only ? 1 : 0, p.inline_bonds ? 1 : 0, p.nown);
    } else if (cmd == "kind") {
      const bool coul14 = rb(is), hybrid = rb(is);
      const BondedKind k = bonded_kind(coul14, hybrid);
      printf("kind %s\n", k == BondedKind::plain ? "plain" : k == BondedKind::hybrid ? "hybrid" : "charged");
    } else printf("error unknown command\n");
  }
  return 0;
}
