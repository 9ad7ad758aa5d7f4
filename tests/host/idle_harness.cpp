// Test harness (CPU only): drives the host rule of chemlab_amd/csrc/chem_idle_host.hpp -- does a step get its neighbour launch?
// -- from a plain-text script on stdin, one answer per line, so that a pytest can compare it with a model of its own.  Not
// part of the product library.  Every double travels as the decimal bit pattern of its 8 bytes (<x>).
//   launch step <acc> <d> hint_gen halted host_gen requested diagnostics s <half_skin> <kappa>      "launch <0|1>"
//   fresh step hint_gen host_gen s lag                                                              "fresh <0|1>"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_idle_host.hpp"
using namespace chem;
static double rd(std::istream& is) { unsigned long long b = 0; is >> b; double v; std::memcpy(&v, &b, 8); return v; }
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "launch") {
      IdleHint h{}; IdleHost host{};
      is >> h.step; h.acc = rd(is); h.d = rd(is); is >> h.gen >> h.halted;
      int req, diag; long long s; is >> host.gen >> req >> diag >> s;
      host.requested = req != 0; host.diagnostics = diag != 0;
      const double half_skin = rd(is), kappa = rd(is);
      printf("launch %d\n", idle_launch(h, host, s, half_skin, kappa) ? 1 : 0);
    } else if (cmd == "fresh") {
      IdleHint h{}; int gen, lag; long long s;
      is >> h.step >> h.gen >> gen >> s >> lag;
      printf("fresh %d\n", idle_hint_fresh(h, gen, s, lag) ? 1 : 0);
    } else printf("error unknown command\n");
  }
  return 0;
}
