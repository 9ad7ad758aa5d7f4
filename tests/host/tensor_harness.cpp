// Test harness (CPU only): drives the host rule of chemlab_amd/csrc/chem_tensor_host.hpp -- which pressure-tensor kernel runs,
// or why none does -- from a plain-text script on stdin, one answer per line, so that a pytest can compare it with a model of
// its own.  Not part of the product library.
//   plan use_tiles n opt_tpp pair_bs energy coul res cap lj_only uniform_lj cubic_tab diag res_a res_b cap_a cap_b
//        "ok <t|r> mode tpp block member"   (member: tensor_variant_built of the answer)   or   "refuse code text..."
//   built        the set, one line: "<t|r>:mode:tpp:block ..."
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_tensor_host.hpp"
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
      const TensorPlan p = tensor_plan(in);
      if (p.code != CHEM_OK) printf("refuse %d %s\n", p.code, pair_refusal_text(p.refused).c_str());
      else printf("ok %c %d %d %d %d\n", p.v.family == PairFamily::tiles ? 't' : 'r', p.v.mode, p.v.tpp, p.v.block,
                  tensor_variant_built(p.v.family, p.v.mode, p.v.tpp, p.v.block) ? 1 : 0);
    } else if (cmd == "built") {
      printf("built");
      for (int f = 0; f < 2; ++f) for (int m = -1; m < 9; ++m) for (int t = 0; t <= 64; ++t) for (int b : {64, 128, 256, 512, 1024, 2048})
        if (tensor_variant_built(f ? PairFamily::rows : PairFamily::tiles, m, t, b)) printf(" %c:%d:%d:%d", f ? 'r' : 't', m, t, b);
      printf("\n");
    } else printf("error unknown command\n");
  }
  return 0;
}
