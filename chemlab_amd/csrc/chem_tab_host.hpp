// chem_tab_host.hpp -- host fitter of the spline kinds of the tabulated potentials (Tabulated / TabulatedAngular /
// TabulatedDihedral with itype 2 and 3; include/chem_mi355.h "Interpolation kinds").  Plain C++ like
// chem_react_host.hpp: no device code, so that tests/host/table_harness.cpp checks it on the CPU.  This is the only place
// the two rules are written down in the product: the kernels see interval coefficients and evaluate a cubic.
//
// A column y_0 .. y_{n-1} on a uniform grid becomes, per interval k = 0 .. n-2, four coefficients in the local coordinate
// w = (x - x_k) / dr in [0, 1]:   y(w) = c0 + w (c1 + w (c2 + w c3)).   Slopes and second derivatives are per grid step.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace chem {

enum { TAB_LINEAR = 1, TAB_AKIMA = 2, TAB_CUBIC = 3 };

// what chem_nb_table_interp / chem_table_create_interp accept: itype 1 from two rows on, the spline kinds from four
inline bool tab_args_ok(int itype, int64_t nrow) {
  return itype == TAB_LINEAR ? nrow >= 2 : ((itype == TAB_AKIMA || itype == TAB_CUBIC) && nrow >= 4);
}

// Hermite form on one interval: end values y0, y1 (d = y1 - y0) and end slopes t0, t1
inline void hermite_coeffs(double y0, double d, double t0, double t1, double* c) {
  c[0] = y0; c[1] = t0; c[2] = 3.0 * d - 2.0 * t0 - t1; c[3] = t0 + t1 - 2.0 * d;
}

// itype 2, Akima (1970): 4 (n - 1) coefficients.  Differences d_k = y_{k+1} - y_k, continued by two on each side
// (d_-1 = 2 d_0 - d_1, d_-2 = 2 d_-1 - d_0, likewise at the upper end); node slope
//   t_k = (|d_{k+1} - d_k| d_{k-1} + |d_{k-1} - d_{k-2}| d_k) / s_k,   s_k = sum of the two weights,
// and t_k = (d_{k-1} + d_k) / 2 where s_k <= 1e-9 max_j s_j (the tie rule of scipy's Akima1DInterpolator).
inline std::vector<double> fit_akima(const double* y, size_t n) {
  std::vector<double> c;
  if (n < 4) return c;
  std::vector<double> m(n + 3);      // m[k + 2] = d_k, k = -2 .. n
  for (size_t k = 0; k + 1 < n; ++k) m[k + 2] = y[k + 1] - y[k];
  m[1] = 2.0 * m[2] - m[3]; m[0] = 2.0 * m[1] - m[2];
  m[n + 1] = 2.0 * m[n] - m[n - 1]; m[n + 2] = 2.0 * m[n + 1] - m[n];
  std::vector<double> w1(n), w2(n), t(n);
  double smax = 0;
  for (size_t k = 0; k < n; ++k) {
    w1[k] = std::fabs(m[k + 3] - m[k + 2]); w2[k] = std::fabs(m[k + 1] - m[k]);
    smax = std::fmax(smax, w1[k] + w2[k]);
  }
  for (size_t k = 0; k < n; ++k) {
    const double s = w1[k] + w2[k];
    t[k] = s > 1e-9 * smax ? (w1[k] * m[k + 1] + w2[k] * m[k + 2]) / s : 0.5 * (m[k + 1] + m[k + 2]);
  }
  c.resize(4 * (n - 1));
  for (size_t k = 0; k + 1 < n; ++k) hermite_coeffs(y[k], m[k + 2], t[k], t[k + 1], &c[4 * k]);
  return c;
}

// itype 3, natural cubic spline: M_k = second derivative times dr^2, M_0 = M_{n-1} = 0,
//   M_{k-1} + 4 M_k + M_{k+1} = 6 (y_{k+1} - 2 y_k + y_{k-1})   (Thomas algorithm),
//   c1 = d_k - (2 M_k + M_{k+1}) / 6,  c2 = M_k / 2,  c3 = (M_{k+1} - M_k) / 6.
inline std::vector<double> fit_natural_cubic(const double* y, size_t n) {
  std::vector<double> c;
  if (n < 4) return c;
  std::vector<double> M(n, 0.0), cp(n, 0.0), dp(n, 0.0);
  for (size_t k = 1; k + 1 < n; ++k) {      // rows 1 .. n-2: sub- and super-diagonal 1, diagonal 4
    const double rhs = 6.0 * (y[k + 1] - 2.0 * y[k] + y[k - 1]);
    const double den = 4.0 - cp[k - 1];
    cp[k] = 1.0 / den;
    dp[k] = (rhs - dp[k - 1]) / den;
  }
  for (size_t k = n - 2; k >= 1; --k) M[k] = dp[k] - cp[k] * M[k + 1];
  c.resize(4 * (n - 1));
  for (size_t k = 0; k + 1 < n; ++k) {
    const double d = y[k + 1] - y[k];
    c[4 * k] = y[k]; c[4 * k + 1] = d - (2.0 * M[k] + M[k + 1]) / 6.0; c[4 * k + 2] = 0.5 * M[k]; c[4 * k + 3] = (M[k + 1] - M[k]) / 6.0;
  }
  return c;
}

inline std::vector<double> fit_column(const double* y, size_t n, int itype) {
  return itype == TAB_AKIMA ? fit_akima(y, n) : fit_natural_cubic(y, n);
}

// Device layouts of the spline kinds, 8 numbers per interval (the two columns are fitted independently: the force is
// the spline of the f column, not the derivative of the e spline):
//   pair tables (md_kernels.hpp PairCore kind 3): two 4-vectors per interval, (f c0..c3) then (e c0..c3) -- the force-only
//     kernel reads the first alone;
//   bonded tables (md_kernels.hpp BTab): four (e, f) pairs per interval, (e c0, f c0) .. (e c3, f c3).
inline std::vector<double> pack_pair_rows(const double* e, const double* f, size_t n, int itype) {
  const std::vector<double> ce = fit_column(e, n, itype), cf = fit_column(f, n, itype);
  std::vector<double> out(2 * ce.size());
  for (size_t k = 0; k + 1 < n; ++k)
    for (int q = 0; q < 4; ++q) { out[8 * k + q] = cf[4 * k + q]; out[8 * k + 4 + q] = ce[4 * k + q]; }
  return out;
}
inline std::vector<double> pack_bond_rows(const double* e, const double* f, size_t n, int itype) {
  const std::vector<double> ce = fit_column(e, n, itype), cf = fit_column(f, n, itype);
  std::vector<double> out(2 * ce.size());
  for (size_t k = 0; k + 1 < n; ++k)
    for (int q = 0; q < 4; ++q) { out[8 * k + 2 * q] = ce[4 * k + q]; out[8 * k + 2 * q + 1] = cf[4 * k + q]; }
  return out;
}

}  // namespace chem
