// chem_react_host.hpp -- the pure host algorithms of the reaction cadence (CtxT::react_step, CtxT::atrp_step in
// chem_api.hip): set-up tables of the scan, the canonical order of the bond-forming events, the max_per_interval
// selection and the ATRP selection.  Plain C++ like chem_host.hpp: no device code, so that tests/host/reaction_harness.cpp
// checks them on the CPU.  Routines that touch device records are templated on the record type (md_kernels.hpp
// Candidate: int a, b, r; unsigned h; double d2).  The oracle keeps its own, separately written versions.
#pragma once
#include <cstring>
#include <utility>

#include "../../include/chem_philox.h"
#include "chem_host.hpp"

namespace chem {

// ReactionConstraintNeighbourState (chem_reaction_constraint), one per reaction row; role 0 = none
struct NbCons { int role = 0, nb_type = 0, min_state = 0, max_state = 0; };
// integrator.ATRPActivator reactive centre (chem_atrp_add_center)
struct AtrpCenter { int type, state, is_activator, new_type, delta_state; double new_mass, new_q; };

// RestrictReaction.define_connection: per-tag CSR of the allowed partners, both directions, from the
// (tag lo, tag hi) -> reaction bits map.  partner / mask hold at least one element (they are uploaded as they are).
struct RestrictCsr { std::vector<int> start, partner; std::vector<unsigned int> mask; };
inline RestrictCsr build_restrict_csr(const std::map<std::pair<int32_t, int32_t>, uint32_t>& restrict_map, int n) {
  RestrictCsr c;
  c.start.assign((size_t)n + 1, 0);
  for (auto& kv : restrict_map) { c.start[kv.first.first + 1]++; c.start[kv.first.second + 1]++; }
  for (int t = 0; t < n; ++t) c.start[t + 1] += c.start[t];
  c.partner.resize(c.start[n] ? c.start[n] : 1); c.mask.resize(c.partner.size());
  std::vector<int> cur(c.start.begin(), c.start.end() - 1);
  for (auto& kv : restrict_map) {
    c.partner[cur[kv.first.first]] = kv.first.second; c.mask[cur[kv.first.first]++] = kv.second;
    c.partner[cur[kv.first.second]] = kv.first.first; c.mask[cur[kv.first.second]++] = kv.second;
  }
  return c;
}

// Neighbour-state constraints, evaluated per particle from the bond graph and the current state and type mirrors (the
// graph lives on the host; candidates carrying a constraint are rare): bit q of word t is set when particle t has the
// constrained role's type of reaction q and a bonded neighbour of cs.nb_type with a state in [min_state, max_state).
inline std::vector<unsigned int> constraint_bits(const HostTopology& top, const std::vector<chem_reaction_desc>& reactions,
                                                 const std::vector<NbCons>& constraints) {
  std::vector<unsigned int> ok((size_t)top.n, 0u);
  for (size_t q = 0; q < constraints.size(); ++q) {
    const NbCons& cs = constraints[q];
    if (!cs.role) continue;
    const int own_type = cs.role == 1 ? reactions[q].type_1 : reactions[q].type_2;
    for (int32_t t = 0; t < (int32_t)top.n; ++t) {
      if (top.type[t] != own_type) continue;
      for (int32_t nb : top.graph[t]) if (top.type[nb] == cs.nb_type && top.state[nb] >= cs.min_state && top.state[nb] < cs.max_state) { ok[t] |= 1u << q; break; }
    }
  }
  return ok;
}

// canonical order of events: (min(a,b), max(a,b))
template <class Rec> inline uint64_t event_key(const Rec& p) { return ((uint64_t)(uint32_t)std::min(p.a, p.b) << 32) | (uint32_t)std::max(p.a, p.b); }

// Bond-forming events of one reaction step into canonical order.  A particle takes part in at most one event per
// reaction step, so min(a,b) alone is a unique key: LSD radix sort (3 x 11 bits) instead of a comparison sort of 10^5
// events; an input that breaks the premise is sorted by the full key.  `scratch` only grows (the caller keeps it: a
// fresh 6 MB vector per step is 1.5 ms of page faults).
template <class Rec> void sort_bond_events(std::vector<Rec>& bev, std::vector<Rec>& scratch) {
  const size_t m = bev.size();
  if (scratch.size() < m) scratch.resize(m);
  Rec* src = bev.data(); Rec* dst = scratch.data();
  for (int pass = 0; pass < 3; ++pass) {
    size_t cnt[2049] = {0};
    const int sh = 11 * pass;
    for (size_t k = 0; k < m; ++k) ++cnt[(((uint32_t)std::min(src[k].a, src[k].b) >> sh) & 2047u) + 1];
    for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
    for (size_t k = 0; k < m; ++k) dst[cnt[((uint32_t)std::min(src[k].a, src[k].b) >> sh) & 2047u]++] = src[k];
    std::swap(src, dst);
  }
  if (src != bev.data()) std::copy(src, src + m, bev.data());
  bool unique = true;
  for (size_t k = 1; k < m && unique; ++k) unique = std::min(bev[k - 1].a, bev[k - 1].b) != std::min(bev[k].a, bev[k].b);
  if (!unique) std::sort(bev.begin(), bev.end(), [](const Rec& p, const Rec& q) { return event_key(p) < event_key(q); });
}

// ChemicalReaction.max_per_interval (reaction_setup.py:426-427): of the accepted candidates (status 2) keep the
// max_per_interval of highest priority -- nearest: r^2 (compared as its bit pattern) then A's tag; random: pair hash then
// A's tag, as the oracle does -- and reject the others (status 0).  Returns whether any status changed.
template <class Rec> bool trim_accepted(const std::vector<Rec>& rec, std::vector<int>& status, int64_t max_per_interval, bool nearest) {
  std::vector<int> accd;
  for (size_t k = 0; k < status.size(); ++k) if (status[k] == 2) accd.push_back((int)k);
  if ((int64_t)accd.size() <= max_per_interval) return false;
  auto key = [&](int k) {
    unsigned long long bits;
    std::memcpy(&bits, &rec[k].d2, sizeof(bits));
    return std::make_pair(nearest ? bits : (unsigned long long)rec[k].h, rec[k].a);
  };
  std::sort(accd.begin(), accd.end(), [&](int p, int q) { return key(p) < key(q); });
  for (size_t k = (size_t)max_per_interval; k < accd.size(); ++k) status[accd[k]] = 0;
  return true;
}

// PostProcessRemoveNeighbourBond (chem_reaction_remove_bond; rule set: include/chem_mi355.h): which bonds the visits of one
// reaction step remove.  `reaction` of a rule and of an event is the row of the association table.  The selection reads the
// bond graph as it stands (this step's new bonds linked, nothing of this step removed yet) and `type0`, the types at the start
// of the step's association phase; it changes nothing.  Events come in canonical order; per event role 1 before role 2, rules
// in the order they were added; within one visit the bonds (p, q) by (tag p, tag q).  A bond found twice is reported for the
// first visit only.
struct NbRemoveRule { int reaction, invoke_on, anchor_type, nb_level, type_1, type_2, unexclude; };
struct AssocEvent { int32_t a, b; int reaction; };
struct RemovedBond { int32_t near, far; int reaction, unexclude; };
inline std::vector<RemovedBond> select_removals(const HostTopology& top, const std::vector<int32_t>& type0, const std::vector<chem_reaction_desc>& reactions,
                                                const std::vector<NbRemoveRule>& rules, const std::vector<AssocEvent>& events) {
  std::vector<RemovedBond> out;
  TupleSet found;
  std::unordered_map<int32_t, int> dist;
  std::vector<int32_t> frontier, next;
  for (const AssocEvent& e : events)
    for (int role = 1; role <= 2; ++role)
      for (const NbRemoveRule& rl : rules) {
        if (rl.reaction != e.reaction || !(rl.invoke_on & role)) continue;
        if ((role == 1 ? reactions[e.reaction].type_1 : reactions[e.reaction].type_2) != rl.anchor_type) continue;
        const int32_t anchor = role == 1 ? e.a : e.b;
        // breadth-first levels 0 .. nb_level; `frontier` ends as level nb_level - 1
        dist.clear(); dist[anchor] = 0; frontier.assign(1, anchor);
        for (int lvl = 1; lvl <= rl.nb_level; ++lvl) {
          next.clear();
          for (int32_t p : frontier) for (int32_t nb : top.graph[p]) if (dist.emplace(nb, lvl).second) next.push_back(nb);
          if (lvl < rl.nb_level) frontier.swap(next);
        }
        std::sort(frontier.begin(), frontier.end());
        for (int32_t p : frontier)
          for (int32_t q : top.graph[p]) {
            if (dist[q] != rl.nb_level) continue;
            const int tp = type0[p], tq = type0[q];
            if (!((tp == rl.type_1 && tq == rl.type_2) || (tp == rl.type_2 && tq == rl.type_1))) continue;
            if (!found.insert(HostTopology::pair_key(p, q))) continue;
            out.push_back(RemovedBond{p, q, e.reaction, rl.unexclude});
          }
      }
  return out;
}
// One removed bond per arity-2 list that holds it, lists in handle order: the batch HostTopology::remove_bonds takes and the
// records of chem_reaction_removed.
inline std::vector<HostTopology::BrokenBond> removals_by_list(const HostTopology& top, const std::vector<RemovedBond>& rem, std::vector<int>* reaction_of = nullptr) {
  std::vector<HostTopology::BrokenBond> bb;
  for (const RemovedBond& r : rem)
    for (size_t li = 0; li < top.lists.size(); ++li) {
      if (top.lists[li].arity != 2 || !top.lists[li].seen.contains(HostTopology::pair_key(r.near, r.far))) continue;
      bb.push_back(HostTopology::BrokenBond{r.near, r.far, (int32_t)li, r.unexclude});
      if (reaction_of) reaction_of->push_back(r.reaction);
    }
  return bb;
}

// One firing of the ATRPActivator (rule set: include/chem_mi355.h, chem_atrp_desc): pool draw (Philox stream keyed
// (seed, step, tag)), the num_particles smallest keys in (key, tag) order, then the acceptance loop with the catalyst
// bookkeeping.  Updates the type/mass/charge/state mirrors of `top` and the two ratios of `atrp`; the caller pushes
// `changes` to the device arrays.
struct AtrpOutcome { std::vector<HostTopology::PropChange> changes; chem_atrp_stats stats; bool types_changed; };
inline AtrpOutcome atrp_select(HostTopology& top, chem_atrp_desc& atrp, const std::vector<AtrpCenter>& centers, int64_t step) {
  struct Sel { uint32_t key; int32_t tag; uint32_t u; int center; };
  auto center_of = [&](int32_t t) {
    for (size_t c = 0; c < centers.size(); ++c) if (centers[c].type == top.type[t] && centers[c].state == top.state[t]) return (int)c;
    return -1;
  };
  std::vector<Sel> pool;
  int64_t ncand = 0;
  for (int32_t t = 0; t < (int32_t)top.n; ++t) {
    const int c = center_of(t);
    if (c >= 0) ++ncand;
    if (c < 0 && !atrp.select_from_all) continue;
    uint32_t r[4];
    chem_philox::atrp_draw(atrp.seed, (uint64_t)step, (uint32_t)t, r);
    pool.push_back(Sel{r[0], t, r[1], c});
  }
  auto less = [](const Sel& a, const Sel& b) { return a.key != b.key ? a.key < b.key : a.tag < b.tag; };
  if ((int64_t)pool.size() > atrp.num_particles) { std::nth_element(pool.begin(), pool.begin() + atrp.num_particles, pool.end(), less); pool.resize((size_t)atrp.num_particles); }
  std::sort(pool.begin(), pool.end(), less);
  const double dc = atrp.delta_catalyst / (double)atrp.num_particles;
  AtrpOutcome out{};
  chem_atrp_stats& st = out.stats;
  st.step = step; st.candidates = ncand; st.selected = (int64_t)pool.size();
  for (auto& sl : pool) {
    if (sl.center < 0) continue;
    const AtrpCenter& c = centers[sl.center];
    const double p = c.is_activator ? atrp.k_deactivate * atrp.ratio_deactivator : atrp.k_activate * atrp.ratio_activator;
    if (!(chem_philox::u01(sl.u) < p)) continue;
    const int32_t t = sl.tag;
    if (c.new_type >= 0 && c.new_type != top.type[t]) { top.type[t] = c.new_type; top.mass[t] = c.new_mass; top.q[t] = c.new_q; out.types_changed = true; }
    top.state[t] += c.delta_state;
    out.changes.push_back(HostTopology::PropChange{t, top.type[t], 1, top.state[t], top.mass[t], top.q[t]});
    if (c.is_activator) { const double m = std::min(dc, atrp.ratio_deactivator); atrp.ratio_deactivator -= m; atrp.ratio_activator += m; st.deactivated++; }
    else { const double m = std::min(dc, atrp.ratio_activator); atrp.ratio_activator -= m; atrp.ratio_deactivator += m; st.activated++; }
  }
  st.ratio_activator = atrp.ratio_activator; st.ratio_deactivator = atrp.ratio_deactivator;
  return out;
}

}  // namespace chem
