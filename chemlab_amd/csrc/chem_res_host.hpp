// chem_res_host.hpp -- per-particle resolution lambda (BasicDynamicResolution, VerletListDynamicResolution*): the pure host
// routines.  Rule set: include/chem_mi355.h (chem_nb_resolution, chem_resolution_rate, chem_set_resolution).  Plain C++ like
// chem_react_host.hpp: no device code, so that tests/host/resolution_harness.cpp checks them on the CPU.
//
// Per tag a stamp (lambda0, s0); with alpha(t) the rate registered for type t (0 if none) the resolution at step s is
//     lambda(s) = min(1.0, lambda0 + alpha(type) * (double)(s - s0))        fp64, in this order, no fused multiply-add
// -- no array that is updated per step.  A particle is re-stamped with (its current lambda, the current step) when lambda is
// set explicitly, when its type changes by any route and when the rate of its type changes; between two stamps type and rate
// are constant, so the expression is exact history.  The device evaluates the same expression (md_kernels.hpp res_lambda_dev).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/chem_mi355.h"

namespace chem {

// the ONE definition of the ramp (res_raw: before the clamp)
inline double res_raw(double lambda0, double alpha, int64_t age) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ramp = alpha * (double)age;
  return lambda0 + ramp;
}
inline double res_lambda(double lambda0, int64_t s0, double alpha, int64_t s) {
  const double l = res_raw(lambda0, alpha, s - s0);
  return l < 1.0 ? l : 1.0;
}
// s_full: the first step s >= s0 at which the expression evaluates to >= 1.0; -1: never (no rate and lambda0 < 1, or further
// away than 2^53 steps).  The estimate from the division is corrected against the expression itself, which decides.
inline int64_t res_full_step(double lambda0, int64_t s0, double alpha) {
  if (lambda0 >= 1.0) return s0;
  if (!(alpha > 0.0)) return -1;
  const double est = std::ceil((1.0 - lambda0) / alpha);
  if (!(est < 9007199254740992.0)) return -1;
  int64_t k = est > 0.0 ? (int64_t)est : 0;
  auto raw = [&](int64_t age) { return res_raw(lambda0, alpha, age); };
  while (k > 0 && raw(k - 1) >= 1.0) --k;
  while (raw(k) < 1.0) ++k;
  return s0 + k;
}

// BasicDynamicResolution entry of one type: the rate and the property change at lambda = 1 (PostProcessChangeProperty)
struct ResRate { double alpha = 0.0; int new_type = -1; double new_mass = 0.0, new_q = 0.0; int new_state = -1; };   // new_type < 0: no change; new_state < 0: state kept
struct ResCompletion { int32_t tag; int new_type; double new_mass, new_q; int new_state; };

// The stamps by tag and the rates by type.  Empty (`on() == false`) until the first call that sets a lambda or a rate: every
// particle is then at lambda = 1 and nothing is allocated.  `seen` is the type each stamp was taken under.
struct ResState {
  std::vector<double> lambda0; std::vector<int64_t> s0; std::vector<int32_t> seen;
  ResRate rate[CHEM_MAX_TYPES];
  bool on() const { return !lambda0.empty(); }
  bool any_rate() const { for (const ResRate& r : rate) if (r.alpha > 0.0) return true; return false; }
  void clear() { lambda0.clear(); s0.clear(); seen.clear(); }
  void ensure(const std::vector<int32_t>& type) {
    if (lambda0.size() == type.size()) return;
    lambda0.assign(type.size(), 1.0); s0.assign(type.size(), 0); seen = type;
  }
  double alpha_of(int type) const { return type >= 0 && type < CHEM_MAX_TYPES ? rate[type].alpha : 0.0; }
  double lambda_at(size_t t, int64_t step) const { return on() ? res_lambda(lambda0[t], s0[t], alpha_of(seen[t]), step) : 1.0; }
  void stamp(size_t t, double lam, int64_t step) { lambda0[t] = lam; s0[t] = step; }
  // type changes: every tag whose mirror type differs from the one its stamp was taken under is re-stamped at `step` with the
  // lambda the OLD type's rate gave it; the tags go to `changed`
  void restamp_type_changes(const std::vector<int32_t>& type, int64_t step, std::vector<int32_t>& changed) {
    if (!on()) return;
    for (size_t t = 0; t < type.size(); ++t) if (type[t] != seen[t]) { stamp(t, lambda_at(t, step), step); seen[t] = type[t]; changed.push_back((int32_t)t); }
  }
  // a new rate entry for `ty`: its particles are re-stamped under the old rate first
  void set_rate(int ty, const ResRate& r, int64_t step, std::vector<int32_t>& changed) {
    for (size_t t = 0; t < seen.size(); ++t) if (seen[t] == ty && lambda0[t] < 1.0) { stamp(t, lambda_at(t, step), step); changed.push_back((int32_t)t); }
    rate[ty] = r;
    if (!(r.alpha > 0.0)) rate[ty] = ResRate{};
  }
  // s_full of tag t if a property change is pending on it, -1 otherwise
  int64_t pending_full_step(size_t t) const {
    if (!(lambda0[t] < 1.0)) return -1;
    const ResRate& r = rate[seen[t]];
    return r.alpha > 0.0 && r.new_type >= 0 ? res_full_step(lambda0[t], s0[t], r.alpha) : -1;
  }
  // the first step > `step` at which some pending change completes; -1: none
  int64_t next_completion(int64_t step) const {
    int64_t best = -1;
    if (!on() || !any_rate()) return best;
    for (size_t t = 0; t < lambda0.size(); ++t) { const int64_t f = pending_full_step(t); if (f > step && (best < 0 || f < best)) best = f; }
    return best;
  }
  // the changes that are complete at `step` (s_full <= step), by ascending tag.  The caller applies them and stamps the tags
  // (1, step) under their new type.
  std::vector<ResCompletion> completions_at(int64_t step) const {
    std::vector<ResCompletion> out;
    if (!on() || !any_rate()) return out;
    for (size_t t = 0; t < lambda0.size(); ++t) {
      const int64_t f = pending_full_step(t);
      if (f >= 0 && f <= step) { const ResRate& r = rate[seen[t]]; out.push_back(ResCompletion{(int32_t)t, r.new_type, r.new_mass, r.new_q, r.new_state}); }
    }
    return out;
  }
};

// Split points of chem_run: a call of `left` steps from `step` runs in pieces that each end at the next completion step `f`
// (next_completion; -1: none) or at the end of the call.  The stamps change at every split, so `f` is asked again per piece.
inline int64_t res_next_piece(int64_t step, int64_t left, int64_t f) { return (f > step && f - step < left) ? f - step : left; }
template <class NextFn> inline std::vector<int64_t> res_run_pieces(int64_t step, int64_t nsteps, NextFn next) {
  std::vector<int64_t> pieces;
  for (int64_t left = nsteps; left > 0;) {
    const int64_t len = res_next_piece(step, left, next(step));
    pieces.push_back(len); step += len; left -= len;
  }
  return pieces;
}

}  // namespace chem
