// chem_region_host.hpp -- region rules (chem_region_add; FreezeRegion, ChangeParticleType): the box test, the firing rule and
// the selection.  Rule set: include/chem_mi355.h ("region rules").  Plain C++ like chem_fix_host.hpp, so that
// tests/host/region_harness.cpp checks it on the CPU; the three small functions marked CHEM_RHD are also what k_region_scan
// (md_kernels.hpp) calls on the device, so host and device cannot drift apart.
//
// The device compacts one record per particle that is a candidate of at least one due rule under its current type: (tag, type,
// bit k set = inside the box of rule k).  A particle that an earlier rule of the step turns into the target of a later one was
// a candidate of the earlier rule, so it has a record: region_fire walks the rules in insertion order over the records alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/chem_mi355.h"
#include "../../include/chem_philox.h"

#if defined(__HIPCC__)
#define CHEM_RHD __host__ __device__ inline
#else
#define CHEM_RHD inline
#endif

namespace chem {

constexpr int kRegionMaxRules = CHEM_MAX_REGIONS;
constexpr int kRegionAll = 0, kRegionProb = 1, kRegionNum = 2, kRegionFraction = 3;

// a coordinate as chem_get_state(CHEM_STATE_POS) folds it
CHEM_RHD double region_fold(double x, double L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = ::floor(x / L);
  x -= s * L;
  if (x >= L) x -= L;
  return x;
}
// lo[d] <= x[d] < hi[d] on every axis, folded coordinates, fp64
CHEM_RHD bool region_inside(const double lo[3], const double hi[3], double x, double y, double z) {
  return lo[0] <= x && x < hi[0] && lo[1] <= y && y < hi[1] && lo[2] <= z && z < hi[2];
}
// how many of `ncand` candidates (`naccept` of them with u01(out[1]) < value) a rule changes
CHEM_RHD long long region_quota(int mode, double value, int num, long long ncand, long long naccept) {
  switch (mode) {
    case kRegionAll: return ncand;
    case kRegionProb: return naccept;
    case kRegionNum: return (long long)num < ncand ? (long long)num : ncand;
    case kRegionFraction: return (long long)::floor(value * (double)ncand);
  }
  return 0;
}

inline bool region_due(const chem_region_desc& d, bool enabled, int64_t step) { return enabled && step > 0 && step % d.interval == 0; }

// chem_region_add: 0, or CHEM_EINVAL with the reason in `why`
inline int region_validate(const chem_region_desc& d, std::string& why) {
  auto bad = [&](const char* w) { why = w; return CHEM_EINVAL; };
  if (d.target_type < 0 || d.target_type >= CHEM_MAX_TYPES) return bad("target_type outside [0, CHEM_MAX_TYPES)");
  if (d.new_type < 0 || d.new_type >= CHEM_MAX_TYPES) return bad("new_type outside [0, CHEM_MAX_TYPES)");
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(d.lo[k]) || !std::isfinite(d.hi[k])) return bad("non-finite bound");
    if (d.lo[k] > d.hi[k]) return bad("lo > hi");
  }
  if (d.interval < 1) return bad("interval < 1");
  if (d.mode < kRegionAll || d.mode > kRegionFraction) return bad("unknown mode");
  if ((d.mode == kRegionProb || d.mode == kRegionFraction) && !(d.value >= 0.0 && d.value <= 1.0)) return bad("value outside [0, 1]");
  if (d.mode == kRegionNum && d.num < 0) return bad("num < 0");
  if (!std::isfinite(d.new_mass) || !std::isfinite(d.new_q) || d.new_mass == 0.0) return bad("new_mass / new_q");
  return 0;
}

struct RegionCand { int32_t tag, type; uint32_t inbox, pad; };
struct RegionChange { int64_t step; int32_t tag, rule; };
struct RegionStat { int64_t step; int32_t rule, pad; int64_t candidates, changed; };

// the tags of `cand` (any order) that rule `rule` changes at `step`, ascending
inline std::vector<int32_t> region_pick(const chem_region_desc& d, int rule, int64_t step, std::vector<int32_t> cand) {
  std::sort(cand.begin(), cand.end());
  if (d.mode == kRegionAll) return cand;
  struct Key { uint32_t key; int32_t tag; };
  std::vector<Key> keys;
  std::vector<int32_t> out;
  for (int32_t t : cand) {
    uint32_t r[4];
    chem_philox::region_draw(d.seed, (uint64_t)step, (uint32_t)t, (uint32_t)rule, r);
    if (d.mode == kRegionProb) { if (chem_philox::u01(r[1]) < d.value) out.push_back(t); }
    else keys.push_back(Key{r[0], t});
  }
  if (d.mode == kRegionProb) return out;
  const size_t k = (size_t)region_quota(d.mode, d.value, d.num, (long long)cand.size(), 0);
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.key != b.key ? a.key < b.key : a.tag < b.tag; });
  for (size_t q = 0; q < k && q < keys.size(); ++q) out.push_back(keys[q].tag);
  std::sort(out.begin(), out.end());
  return out;
}

// One firing step: the due rules in insertion order over the records; a record changed by a rule carries its new type into
// the later ones.  Appends the changes (by rule, then tag) and one stats row per rule that changed something.
inline void region_fire(const std::vector<chem_region_desc>& rules, const std::vector<uint8_t>& enabled, int64_t step,
                        std::vector<RegionCand>& recs, std::vector<RegionChange>& changes, std::vector<RegionStat>& stats) {
  for (size_t k = 0; k < rules.size(); ++k) {
    const chem_region_desc& d = rules[k];
    if (!region_due(d, enabled[k] != 0, step)) continue;
    std::vector<int32_t> cand;
    for (const RegionCand& r : recs) if (r.type == d.target_type && ((r.inbox >> k) & 1u)) cand.push_back(r.tag);
    if (cand.empty()) continue;
    const std::vector<int32_t> hit = region_pick(d, (int)k, step, cand);
    if (hit.empty()) continue;
    for (RegionCand& r : recs) if (r.type == d.target_type && ((r.inbox >> k) & 1u) && std::binary_search(hit.begin(), hit.end(), r.tag)) r.type = d.new_type;
    for (int32_t t : hit) changes.push_back(RegionChange{step, t, (int32_t)k});
    stats.push_back(RegionStat{step, (int32_t)k, 0, (int64_t)cand.size(), (int64_t)hit.size()});
  }
}

}  // namespace chem
