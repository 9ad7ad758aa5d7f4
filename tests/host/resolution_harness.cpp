// Test harness (CPU only): drives the pure resolution routines of chemlab_amd/csrc/chem_res_host.hpp (res_lambda,
// res_full_step, ResState: stamps, re-stamping, completions, the pieces of a run) from a plain-text script on stdin.  A
// program of its own, so that it can also be built with -fsanitize=address,undefined.  Not part of the product library.
//   lam <lambda0> <s0> <alpha> <s>       prints "lam <value>"
//   full <lambda0> <s0> <alpha>          prints "full <s_full | -1>"
//   n <N> <type>...                      the particles (all at lambda 1)
//   setlam <i> <value> <s>               stamp (value, s)
//   settype <i> <type> <s>               the mirror type changes, then restamp_type_changes at s; prints "changed <count>"
//   rate <type> <alpha> <s> <new_type>   set_rate at step s (new_type -1: no change)
//   get <s>                              prints "get" and one line "lambda0 s0 type lambda(s)" per particle
//   next <s>                             prints "next <next_completion(s)>"
//   run <step> <nsteps>                  the loop of chem_run: pieces by res_next_piece, completions applied (type, stamp (1, step))
//                                        at the end of every piece; prints "run <pieces...>" and "done <step> <i>..." per piece that completed something
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../chemlab_amd/csrc/chem_res_host.hpp"
using namespace chem;
int main() {
  ResState rs;
  std::vector<int32_t> type;
  std::string line;
  auto num = [](std::istringstream& is) { std::string t; is >> t; return std::stod(t); };
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "lam") { const double l0 = num(is); long long s0; is >> s0; const double a = num(is); long long s; is >> s; printf("lam %.17g\n", res_lambda(l0, s0, a, s)); }
    else if (cmd == "full") { const double l0 = num(is); long long s0; is >> s0; const double a = num(is); printf("full %lld\n", (long long)res_full_step(l0, s0, a)); }
    else if (cmd == "n") { int n; is >> n; type.resize(n); for (int i = 0; i < n; ++i) is >> type[i]; rs.clear(); rs.ensure(type); }
    else if (cmd == "setlam") { int i; is >> i; const double v = num(is); long long s; is >> s; rs.stamp((size_t)i, v, s); }
    else if (cmd == "settype") { int i, t; long long s; is >> i >> t >> s; type[i] = t; std::vector<int32_t> ch; rs.restamp_type_changes(type, s, ch); printf("changed %zu\n", ch.size()); }
    else if (cmd == "rate") { int t; is >> t; const double a = num(is); long long s; int nt; is >> s >> nt; std::vector<int32_t> ch; ResRate r; r.alpha = a; r.new_type = nt; r.new_mass = 1.0; rs.set_rate(t, r, s, ch); }
    else if (cmd == "get") { long long s; is >> s; printf("get\n"); for (size_t i = 0; i < type.size(); ++i) printf("%.17g %lld %d %.17g\n", rs.lambda0[i], (long long)rs.s0[i], rs.seen[i], rs.lambda_at(i, s)); }
    else if (cmd == "next") { long long s; is >> s; printf("next %lld\n", (long long)rs.next_completion(s)); }
    else if (cmd == "run") {
      long long step, nsteps; is >> step >> nsteps;
      std::string pieces = "run", done;
      for (long long left = nsteps; left > 0;) {
        const int64_t len = res_next_piece(step, left, rs.next_completion(step));
        if (len <= 0 || len > left) { printf("bad piece %lld\n", (long long)len); return 1; }
        pieces += " " + std::to_string(len); step += len; left -= len;
        const std::vector<ResCompletion> c = rs.completions_at(step);
        if (!c.empty()) done += "done " + std::to_string(step);
        for (const ResCompletion& k : c) { type[k.tag] = k.new_type; rs.stamp(k.tag, 1.0, step); rs.seen[k.tag] = k.new_type; done += " " + std::to_string(k.tag); }
        if (!c.empty()) done += "\n";
      }
      printf("%s\n%s", pieces.c_str(), done.c_str());
    }
  }
  return 0;
}
