// chem_baro_host.hpp -- the rules of the pressure observable and of the Berendsen barostat (chem_get_pressure,
// chem_barostat_berendsen; include/chem_mi355.h "Pressure and barostat"): plain double arithmetic over plain values.  The
// device (k_baro_mu, md_kernels.hpp) and the host (CtxT::baro_step, chem_api.hip) call the same expressions,
// tests/host/barostat_harness.cpp checks them on the CPU.  No HIP include.
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
