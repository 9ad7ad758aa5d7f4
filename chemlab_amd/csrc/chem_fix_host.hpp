// chem_fix_host.hpp -- FixDistances / ReleaseMolecule (chem_fix_create ff.): the pure host routines.  Rule set:
// include/chem_mi355.h ("fixed distances").  Plain C++ like chem_res_host.hpp: no device code, so that
// tests/host/fix_harness.cpp checks them on the CPU.
//
// A set holds its live entries (anchor tag, target tag, distance) in insertion order; every entry carries the insertion index
// `seq` it got when it was added (per set, never reused).  Releases remove entries and keep the order of the others; every
// release is logged as (step, set, anchor, target, cause), the records of one step ordered by (set, seq).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/chem_mi355.h"

namespace chem {

constexpr int kFixMaxSets = CHEM_MAX_FIX_SETS;
constexpr int kFixCauseReaction = 1, kFixCauseType = 2, kFixCauseJoined = 3, kFixCauseRefused = 4;

struct FixEntry { int32_t anchor, target; double dist; int64_t seq; };
// what becomes of a released target of type old_type (chem_fix_postprocess): new_type < 0 no property change, new_state < 0
// state kept, lambda < 0 resolution left alone
struct FixPost { int old_type, new_type; double new_mass, new_q; int new_state; double lambda; };
struct FixRule { int reaction, role, set, count; };      // chem_reaction_release: public reaction index, role 1 | 2
struct FixJoinRule { int reaction, role, set; double dist; };      // chem_reaction_join: public reaction index, anchor role 1 | 2
struct FixRecord { int64_t step; int32_t set, anchor, target, cause; int64_t seq; };
struct FixSet {
  int anchor_type = -1, target_type = -1;
  std::vector<FixEntry> ent;
  std::vector<FixPost> post;
  int64_t next_seq = 0;
};
// one reactant of a bond-forming event, in the order the releases are taken: events as chem_get_events reports them, role 1
// before role 2
struct FixReactant { int reaction, role; int32_t tag; };

struct FixState {
  std::vector<FixSet> sets;
  std::vector<FixRule> rules;
  std::vector<FixRecord> log;
  std::vector<FixJoinRule> joins;
  std::vector<FixRecord> join_log;                     // chem_fix_joins: cause 3 = joined, 4 = refused, in visit order
  std::unordered_set<int32_t> targets;                 // tags that are the target of a live entry
  std::unordered_map<int32_t, int> anchors;            // tag -> number of live entries it anchors
  bool any() const { for (const FixSet& s : sets) if (!s.ent.empty()) return true; return false; }
  int64_t count() const { int64_t c = 0; for (const FixSet& s : sets) c += (int64_t)s.ent.size(); return c; }

  // chem_fix_create; the handle or CHEM_ENOSPC
  int create(int anchor_type, int target_type) {
    if ((int)sets.size() >= kFixMaxSets) return CHEM_ENOSPC;
    FixSet s; s.anchor_type = anchor_type; s.target_type = target_type;
    sets.push_back(s);
    return (int)sets.size() - 1;
  }
  // chem_fix_add on tags (a tag < 0: unknown id).  All or nothing: 0, or CHEM_EINVAL with the reason in `why`.
  int add(int set, int64_t n, const int32_t* pairs, double dist, int64_t ntags, std::string& why) {
    if (set < 0 || set >= (int)sets.size()) { why = "unknown set"; return CHEM_EINVAL; }
    if (!(dist > 0.0) || !std::isfinite(dist)) { why = "the distance must be positive and finite"; return CHEM_EINVAL; }
    std::unordered_set<int32_t> new_t, new_a;
    for (int64_t k = 0; k < n; ++k) {
      const int32_t a = pairs[2 * k], t = pairs[2 * k + 1];
      if (a < 0 || t < 0 || a >= ntags || t >= ntags) { why = "unknown particle id"; return CHEM_EINVAL; }
      if (a == t) { why = "anchor and target are one particle"; return CHEM_EINVAL; }
      if (targets.count(t) || new_t.count(t)) { why = "a particle may be the target of one live entry only"; return CHEM_EINVAL; }
      if (anchors.count(t) || new_a.count(t)) { why = "a target may not be an anchor"; return CHEM_EINVAL; }
      if (targets.count(a) || new_t.count(a)) { why = "an anchor may not be a target"; return CHEM_EINVAL; }
      new_t.insert(t); new_a.insert(a);
    }
    FixSet& s = sets[set];
    for (int64_t k = 0; k < n; ++k) {
      const int32_t a = pairs[2 * k], t = pairs[2 * k + 1];
      s.ent.push_back(FixEntry{a, t, dist, s.next_seq++});
      targets.insert(t); ++anchors[a];
    }
    return 0;
  }
  // the post-process of `set` for a target of type `type`; nullptr: none
  const FixPost* post_for(int set, int type) const {
    for (const FixPost& p : sets[set].post) if (p.old_type == type) return &p;
    return nullptr;
  }
  void set_post(int set, const FixPost& p) {
    for (FixPost& q : sets[set].post) if (q.old_type == p.old_type) { q = p; return; }
    sets[set].post.push_back(p);
  }

  // ---- releases.  Both selections mark, then compact once per set (order kept), append the records of this step and sort
  // the step's records by (set, seq).  They return the released entries in log order of this call. ----
  std::vector<FixRecord> release_marked(std::vector<std::vector<char>>& mark, int64_t step, int cause) {
    std::vector<FixRecord> out;
    for (size_t si = 0; si < sets.size(); ++si) {
      FixSet& s = sets[si];
      if (mark[si].empty()) continue;
      size_t w = 0;
      for (size_t k = 0; k < s.ent.size(); ++k) {
        const FixEntry e = s.ent[k];
        if (mark[si][k]) {
          out.push_back(FixRecord{step, (int32_t)si, e.anchor, e.target, cause, e.seq});
          targets.erase(e.target);
          auto it = anchors.find(e.anchor);
          if (it != anchors.end() && --it->second == 0) anchors.erase(it);
        } else s.ent[w++] = e;
      }
      s.ent.resize(w);
    }
    if (!out.empty()) {
      log.insert(log.end(), out.begin(), out.end());
      size_t lo = log.size();
      while (lo > 0 && log[lo - 1].step == step) --lo;
      std::stable_sort(log.begin() + lo, log.end(), [](const FixRecord& p, const FixRecord& q) { return p.set != q.set ? p.set < q.set : p.seq < q.seq; });
    }
    return out;
  }
  // Release by a reaction: per reactant, per rule of its (reaction, role) in the order the rules were added, up to `count`
  // live entries of the rule's set anchored at the reactant, lowest insertion index first; fewer if fewer remain.
  std::vector<FixRecord> release_by_reaction(const std::vector<FixReactant>& reactants, int64_t step) {
    std::vector<std::vector<char>> mark(sets.size());
    if (rules.empty() || !any()) return {};
    bool hit = false;
    for (const FixReactant& r : reactants)
      for (const FixRule& rl : rules) {
        if (rl.reaction != r.reaction || rl.role != r.role || !anchors.count(r.tag)) continue;
        const FixSet& s = sets[rl.set];
        std::vector<char>& m = mark[rl.set];
        int left = rl.count;
        for (size_t k = 0; k < s.ent.size() && left > 0; ++k) {
          if (s.ent[k].anchor != r.tag) continue;
          if (m.empty()) m.assign(s.ent.size(), 0);
          if (!m[k]) { m[k] = 1; --left; hit = true; }
        }
      }
    if (!hit) return {};
    return release_marked(mark, step, kFixCauseReaction);
  }
  // Release by type: sets created with a type condition lose every entry whose anchor or target no longer has that type
  // (a condition of -1 on one side asks nothing of that side).
  std::vector<FixRecord> release_by_type(const std::vector<int32_t>& type, int64_t step) {
    std::vector<std::vector<char>> mark(sets.size());
    bool hit = false;
    for (size_t si = 0; si < sets.size(); ++si) {
      const FixSet& s = sets[si];
      if (s.anchor_type < 0 && s.target_type < 0) continue;
      for (size_t k = 0; k < s.ent.size(); ++k) {
        const bool off = (s.anchor_type >= 0 && type[s.ent[k].anchor] != s.anchor_type) || (s.target_type >= 0 && type[s.ent[k].target] != s.target_type);
        if (!off) continue;
        if (mark[si].empty()) mark[si].assign(s.ent.size(), 0);
        mark[si][k] = 1; hit = true;
      }
    }
    if (!hit) return {};
    return release_marked(mark, step, kFixCauseType);
  }
  // Join by a reaction (chem_reaction_join): per event (canonical order), per rule of its reaction in the order the rules were
  // added, the reactant in the rule's role becomes the anchor and the other one the target of a new entry of the rule's set.
  // A pair chem_fix_add would refuse adds nothing and is logged with cause 4.  Returns the new entries in visit order.
  struct JoinEvent { int reaction; int32_t a, b; };      // a: role 1, b: role 2
  std::vector<FixEntry> join_by_reaction(const std::vector<JoinEvent>& events, int64_t step, int64_t ntags) {
    std::vector<FixEntry> added;
    std::string why;
    for (const JoinEvent& e : events)
      for (const FixJoinRule& rl : joins) {
        if (rl.reaction != e.reaction) continue;
        const int32_t pair[2] = {rl.role == 1 ? e.a : e.b, rl.role == 1 ? e.b : e.a};
        const bool ok = add(rl.set, 1, pair, rl.dist, ntags, why) == 0;
        const int64_t seq = ok ? sets[rl.set].ent.back().seq : -1;
        join_log.push_back(FixRecord{step, (int32_t)rl.set, pair[0], pair[1], ok ? kFixCauseJoined : kFixCauseRefused, seq});
        if (ok) added.push_back(sets[rl.set].ent.back());
      }
    return added;
  }
  // the flat device order: every live entry, entries of one anchor consecutive (stable by anchor tag: sets and insertion
  // order decide among equals)
  std::vector<FixEntry> device_order() const {
    std::vector<FixEntry> all;
    for (const FixSet& s : sets) all.insert(all.end(), s.ent.begin(), s.ent.end());
    std::stable_sort(all.begin(), all.end(), [](const FixEntry& p, const FixEntry& q) { return p.anchor < q.anchor; });
    return all;
  }
};

}  // namespace chem
