// chem_baro_host.hpp -- the rules of the pressure observable, of the Berendsen barostat and of the Langevin piston
// (chem_get_pressure, chem_barostat_berendsen, chem_barostat_langevin; include/chem_mi355.h "Pressure and barostat"): plain
// double arithmetic over plain values.  The device (k_baro_mu, k_baro_piston, md_kernels.hpp) and the host (CtxT::baro_measure,
// CtxT::baro_apply, chem_api.hip) call the same expressions, tests/host/barostat_harness.cpp and tests/host/piston_harness.cpp
// check them on the CPU.  No HIP include.
#pragma once
#include <cmath>

#include "../../include/chem_philox.h"      // CHEM_HD: __host__ __device__ inline under hipcc, inline otherwise
#include "chem_geom_host.hpp"

namespace chem {

// P = (sum_i m_i v_i^2 + W) / (3 V)
CHEM_HD double baro_pressure(double mv2, double virial, double volume) { return (mv2 + virial) / (3.0 * volume); }

// mu^3 = 1 - (dt / tau) (P0 - P): the factor of the volume.  No clamp: a value <= 0 (or a NaN) stops the run.
CHEM_HD double baro_mu3(double dt, double tau, double p0, double p) { return 1.0 - (dt / tau) * (p0 - p); }
CHEM_HD bool baro_mu3_ok(double mu3) { return mu3 > 0.0; }      // (false for a NaN)
CHEM_HD double baro_mu(double mu3) { return cbrt(mu3); }

// ---- Langevin piston (chem_barostat_langevin) ----
// pe: the piston momentum, eps_dot = pe / W.  nf = 3 n degrees of freedom, c = 1 + 3 / nf.
// sv = exp(-c eps_dot dt / 2): the factor of the velocities on either side of a step's two half kicks.
CHEM_HD double piston_sv(double pe, double w, double nf, double dt) { return exp(-0.5 * (1.0 + 3.0 / nf) * (pe / w) * dt); }
// mu = exp(eps_dot dt): the factor of the box and of the drifted positions.
CHEM_HD double piston_mu(double pe, double w, double dt) { return exp((pe / w) * dt); }
// G = 3 V (P - P0) + (3 / nf) sum m v^2 - gammaP pe + sqrt(24 gammaP W kT / dt) (u - 1/2),  u uniform in (0, 1): pe <- pe + dt G
CHEM_HD double piston_force(double volume, double p, double p0, double nf, double mv2, double gamma_p, double pe, double w, double kT, double dt, double u) {
  return 3.0 * volume * (p - p0) + (3.0 / nf) * mv2 - gamma_p * pe + sqrt(24.0 * gamma_p * w * kT / dt) * (u - 0.5);
}
// No clamp: a momentum or a factor that is not finite (or a mu of 0, whose 1 / sqrt(mu) is not) stops the run.
CHEM_HD bool piston_ok(double pe, double mu, double sv) { return isfinite(pe) && isfinite(mu) && isfinite(sv) && mu > 0.0; }

// Scaling every coordinate by mu changes a separation r by |mu - 1| r.  Every listed separation is at most rc + skin_eff, so
// each of its two particles is charged half of |mu - 1| (rc + skin_eff) as displacement, in the unit the rebuild criterion
// accumulates (a distance, compared with skin_eff / 2).
inline double baro_list_charge(double mu, double rc, double skin_eff) { return 0.5 * std::fabs(mu - 1.0) * (rc + skin_eff); }

// After a scaling: does the box ask for another cell grid than the one in force?  (cell_grid: floor(L / (rc + skin_eff)) per
// axis, none below 3 on any axis.)  Either direction counts, so the geometry in force is always the one a fresh context plans.
inline bool baro_replan(const double L[3], double rl, const int nc_in_force[3]) {
  const CellGrid g = cell_grid(L, rl);
  return g.nc[0] != nc_in_force[0] || g.nc[1] != nc_in_force[1] || g.nc[2] != nc_in_force[2];
}

}  // namespace chem
