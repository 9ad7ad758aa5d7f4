// Test harness (CPU only): drives the Langevin-piston rules of chemlab_amd/csrc/chem_baro_host.hpp -- the two factors, the
// piston force and the stop condition -- from a plain-text script on stdin, one answer per line, so that a pytest can compare
// them with tests/piston_ref.py.  Not part of the product library.  Every double travels as the decimal bit pattern of its 8
// bytes (<x>), in and out.
//   factors <pe> <W> <nf> <dt>                                               "factors <sv> <mu> ok"
//   force <V> <P> <P0> <nf> <mv2> <gammaP> <pe> <W> <kT> <dt> <u>            "force <G> <pe + dt G>"
//   draw seed step                                                           "draw o0 o1 o2 o3"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include "../../chemlab_amd/csrc/chem_baro_host.hpp"
using namespace chem;
static double rd(std::istream& is) { unsigned long long b = 0; is >> b; double v; std::memcpy(&v, &b, 8); return v; }
static unsigned long long bits(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "factors") {
      const double pe = rd(is), w = rd(is), nf = rd(is), dt = rd(is);
      const double sv = piston_sv(pe, w, nf, dt), mu = piston_mu(pe, w, dt);
      printf("factors %llu %llu %d\n", bits(sv), bits(mu), piston_ok(pe, mu, sv) ? 1 : 0);
    } else if (cmd == "force") {
      double a[11]; for (double& x : a) x = rd(is);
      const double g = piston_force(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]);
      printf("force %llu %llu\n", bits(g), bits(a[6] + a[9] * g));
    } else if (cmd == "draw") {
      unsigned long long seed = 0, step = 0; is >> seed >> step;
      uint32_t o[4];
      chem_philox::barostat_draw(seed, step, o);
      printf("draw %u %u %u %u\n", o[0], o[1], o[2], o[3]);
    } else printf("error unknown command\n");
  }
  return 0;
}
