// chem_ckpt_host.hpp -- checkpoint blobs (chem_checkpoint_save / chem_checkpoint_load): the writer, the reader, the fingerprint
// compare and the checksum.  Rule set: include/chem_mi355.h ("checkpoint").  Plain C++ like chem_fix_host.hpp: no device code,
// so that tests/host/checkpoint_harness.cpp checks them on the CPU.
//
// A blob holds the STATE of a context (CkptState: everything chem_run changes), not its configuration.  Layout, little endian,
// no alignment is assumed (every word is copied out):
//     header    u32 magic 'CHCK', u32 format version, u32 precision (32 | 64), u32 0
//     sections  in the fixed order of kCkptSections, each  u32 id, u32 0, u64 length, payload[length]
//     trailer   the section END: length 8, payload = u64 FNV-1a of every byte in front of that word
// An array is a u64 count followed by its elements; records are written field by field (no padding bytes, so equal states give
// equal bytes).  The first section is the fingerprint of the configuration the blob was written under (CkptFingerprint).
//
// ckpt_read validates the whole blob before it hands anything out, in this order: the header (magic, version, precision), the
// section walk (every id, every length against the bytes that are left: no read past nbytes), the checksum, the fingerprint
// against the context's, then every section's content (counts against the section, tags against the particle count, list
// entries against the list table, ...).  A refusal is CHEM_EINVAL with the reason in `why`; `out` is written only on success.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/chem_mi355.h"
#include "chem_fix_host.hpp"

namespace chem {

constexpr uint32_t kCkptMagic = 0x4B434843u;      // "CHCK"
constexpr uint32_t kCkptVersion = 1;
constexpr uint32_t kCkptEnd = 0x21444E45u;        // "END!"
enum CkptSection : uint32_t { CKPT_FINGERPRINT = 1, CKPT_CORE, CKPT_BAROSTAT, CKPT_PARTICLES, CKPT_RESOLUTION, CKPT_LISTS, CKPT_EXCLUSIONS,
                              CKPT_GRAPH, CKPT_FIX, CKPT_REMOVED, CKPT_EVENTS, CKPT_ATRP };
struct CkptSectionName { uint32_t id; const char* name; };
constexpr CkptSectionName kCkptSections[] = {
    {CKPT_FINGERPRINT, "fingerprint"}, {CKPT_CORE, "core"}, {CKPT_BAROSTAT, "barostat"}, {CKPT_PARTICLES, "particles"}, {CKPT_RESOLUTION, "resolution"},
    {CKPT_LISTS, "lists"}, {CKPT_EXCLUSIONS, "exclusions"}, {CKPT_GRAPH, "graph"}, {CKPT_FIX, "fix"}, {CKPT_REMOVED, "removed"}, {CKPT_EVENTS, "events"},
    {CKPT_ATRP, "atrp"}, {kCkptEnd, "end"}};
constexpr size_t kCkptSectionCount = sizeof(kCkptSections) / sizeof(kCkptSections[0]);
constexpr size_t kCkptHeaderBytes = 16, kCkptSectionHeaderBytes = 16;

inline uint64_t ckpt_checksum(const uint8_t* p, size_t n) {      // FNV-1a, 64 bit
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t k = 0; k < n; ++k) { h ^= p[k]; h *= 0x100000001b3ull; }
  return h;
}

// ---- the fingerprint: what a blob needs of the context it is loaded into -------------------------------------------------
struct CkptListKind { int32_t arity = 0, kind = 0, by_types = 0, hybrid = 0; };
struct CkptFingerprint {
  int32_t max_lists = CHEM_MAX_LISTS, max_types = CHEM_MAX_TYPES, max_reactions = CHEM_MAX_REACTIONS, max_pot_params = CHEM_MAX_POT_PARAMS,
          max_fix_sets = CHEM_MAX_FIX_SETS;
  std::vector<CkptListKind> lists;
  int32_t n_reactions = 0, n_dissociations = 0, n_fix_sets = 0, atrp_on = 0;
  int64_t npart = 0;
};
// the first field in which the blob's fingerprint differs from the context's, with both values; empty: they agree
inline std::string ckpt_fingerprint_diff(const CkptFingerprint& blob, const CkptFingerprint& ctx) {
  auto say = [](const std::string& field, long long b, long long c) { return field + " (blob " + std::to_string(b) + ", context " + std::to_string(c) + ")"; };
  if (blob.max_lists != ctx.max_lists) return say("CHEM_MAX_LISTS", blob.max_lists, ctx.max_lists);
  if (blob.max_types != ctx.max_types) return say("CHEM_MAX_TYPES", blob.max_types, ctx.max_types);
  if (blob.max_reactions != ctx.max_reactions) return say("CHEM_MAX_REACTIONS", blob.max_reactions, ctx.max_reactions);
  if (blob.max_pot_params != ctx.max_pot_params) return say("CHEM_MAX_POT_PARAMS", blob.max_pot_params, ctx.max_pot_params);
  if (blob.max_fix_sets != ctx.max_fix_sets) return say("CHEM_MAX_FIX_SETS", blob.max_fix_sets, ctx.max_fix_sets);
  if (blob.lists.size() != ctx.lists.size()) return say("list count", (long long)blob.lists.size(), (long long)ctx.lists.size());
  for (size_t l = 0; l < blob.lists.size(); ++l) {
    const CkptListKind &b = blob.lists[l], &c = ctx.lists[l];
    const std::string at = "list " + std::to_string(l) + " ";
    if (b.arity != c.arity) return say(at + "arity", b.arity, c.arity);
    if (b.kind != c.kind) return say(at + "kind", b.kind, c.kind);
    if (b.by_types != c.by_types) return say(at + "by_types", b.by_types, c.by_types);
    if (b.hybrid != c.hybrid) return say(at + "hybrid", b.hybrid, c.hybrid);
  }
  if (blob.n_reactions != ctx.n_reactions) return say("reaction count", blob.n_reactions, ctx.n_reactions);
  if (blob.n_dissociations != ctx.n_dissociations) return say("dissociation count", blob.n_dissociations, ctx.n_dissociations);
  if (blob.n_fix_sets != ctx.n_fix_sets) return say("fix-set count", blob.n_fix_sets, ctx.n_fix_sets);
  if (blob.atrp_on != ctx.atrp_on) return say("ATRP on", blob.atrp_on, ctx.atrp_on);
  if (blob.npart != ctx.npart) return say("particle count", blob.npart, ctx.npart);
  return std::string();
}

// ---- the state ------------------------------------------------------------------------------------------------------------
struct CkptRemoved { int64_t step = 0; int32_t near = 0, far = 0, list = 0, reaction = 0; };      // chem_reaction_removed, by tags
struct CkptState {
  // core
  int64_t step = 0; double L[3] = {0, 0, 0}; int32_t react_on = 0, ran = 0;
  // barostat: what chem_barostat_state_get shows and what the scalings since the last list build were charged to the lists
  int32_t baro_kind = 0; double baro_p_last = 0, pist_pe = 0, pist_eps = 0, pist_sv = 1, pist_mu = 1, baro_charge = 0, baro_charge_ref = 0;
  // particle table in tag order; pos and image as the device holds them (pos is not folded again), 3 per particle
  std::vector<int64_t> id; std::vector<int32_t> type, state, res_id, mol_id; std::vector<double> mass, q, pos, vel; std::vector<int32_t> image;
  // resolution stamps (all three empty while the context keeps none)
  std::vector<double> res_lambda0; std::vector<int64_t> res_s0; std::vector<int32_t> res_seen;
  // every list's entries in order (arity tags each), birth steps of a hybrid list
  struct List { std::vector<int32_t> ent; std::vector<int64_t> birth; };
  std::vector<List> lists;
  std::vector<int32_t> excl;       // excluded tag pairs in the order they were accepted
  std::vector<int32_t> graph;      // bonds of the topology manager's graph as tag pairs (a < b), by a, then b
  struct FixSetState { int64_t next_seq = 0; std::vector<FixEntry> ent; };
  std::vector<FixSetState> fix_sets; std::vector<FixRecord> fix_log, fix_joins;
  std::vector<CkptRemoved> removed;
  // event log: the records in arena order (r: row of the association table, ~row of the dissociation table) and the blocks
  std::vector<int32_t> ev_a, ev_b, ev_r; std::vector<double> ev_d2; std::vector<int8_t> ev_intra;
  std::vector<int64_t> ev_block_step; std::vector<uint64_t> ev_block_first;
  // ATRP: the catalyst ratios as the flips left them, one row per firing
  double atrp_ratio_activator = 0, atrp_ratio_deactivator = 0; std::vector<chem_atrp_stats> atrp_stats;
};

// ---- writer ---------------------------------------------------------------------------------------------------------------
struct CkptWriter {
  std::vector<uint8_t> b; size_t len_at = 0;
  template <class T> void put(T v) {
    static_assert(std::is_arithmetic<T>::value, "scalars only");
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
  }
  template <class T> void put_array(const std::vector<T>& v) {
    static_assert(std::is_arithmetic<T>::value, "scalars only");
    put<uint64_t>(v.size());
    const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
    if (!v.empty()) b.insert(b.end(), p, p + v.size() * sizeof(T));
  }
  void begin(uint32_t id) { put<uint32_t>(id); put<uint32_t>(0); len_at = b.size(); put<uint64_t>(0); }
  void end() { const uint64_t len = b.size() - len_at - 8; std::memcpy(&b[len_at], &len, 8); }
};

inline void ckpt_put_records(CkptWriter& w, const std::vector<FixRecord>& v) {
  w.put<uint64_t>(v.size());
  for (const FixRecord& r : v) { w.put(r.step); w.put(r.set); w.put(r.anchor); w.put(r.target); w.put(r.cause); w.put(r.seq); }
}

inline std::vector<uint8_t> ckpt_write(int precision, const CkptFingerprint& fp, const CkptState& s) {
  CkptWriter w;
  w.put<uint32_t>(kCkptMagic); w.put<uint32_t>(kCkptVersion); w.put<uint32_t>((uint32_t)precision); w.put<uint32_t>(0);
  w.begin(CKPT_FINGERPRINT);
  w.put(fp.max_lists); w.put(fp.max_types); w.put(fp.max_reactions); w.put(fp.max_pot_params); w.put(fp.max_fix_sets);
  w.put<int32_t>((int32_t)fp.lists.size());
  for (const CkptListKind& l : fp.lists) { w.put(l.arity); w.put(l.kind); w.put(l.by_types); w.put(l.hybrid); }
  w.put(fp.n_reactions); w.put(fp.n_dissociations); w.put(fp.n_fix_sets); w.put(fp.atrp_on); w.put(fp.npart);
  w.end();
  w.begin(CKPT_CORE);
  w.put(s.step); for (double l : s.L) w.put(l); w.put(s.react_on); w.put(s.ran);
  w.end();
  w.begin(CKPT_BAROSTAT);
  w.put(s.baro_kind); w.put(s.baro_p_last); w.put(s.pist_pe); w.put(s.pist_eps); w.put(s.pist_sv); w.put(s.pist_mu); w.put(s.baro_charge); w.put(s.baro_charge_ref);
  w.end();
  w.begin(CKPT_PARTICLES);
  w.put_array(s.id); w.put_array(s.type); w.put_array(s.state); w.put_array(s.res_id); w.put_array(s.mol_id); w.put_array(s.mass); w.put_array(s.q);
  w.put_array(s.pos); w.put_array(s.image); w.put_array(s.vel);
  w.end();
  w.begin(CKPT_RESOLUTION);
  w.put_array(s.res_lambda0); w.put_array(s.res_s0); w.put_array(s.res_seen);
  w.end();
  w.begin(CKPT_LISTS);
  w.put<uint64_t>(s.lists.size());
  for (const CkptState::List& l : s.lists) { w.put_array(l.ent); w.put_array(l.birth); }
  w.end();
  w.begin(CKPT_EXCLUSIONS); w.put_array(s.excl); w.end();
  w.begin(CKPT_GRAPH); w.put_array(s.graph); w.end();
  w.begin(CKPT_FIX);
  w.put<uint64_t>(s.fix_sets.size());
  for (const CkptState::FixSetState& f : s.fix_sets) {
    w.put(f.next_seq); w.put<uint64_t>(f.ent.size());
    for (const FixEntry& e : f.ent) { w.put(e.anchor); w.put(e.target); w.put(e.dist); w.put(e.seq); }
  }
  ckpt_put_records(w, s.fix_log); ckpt_put_records(w, s.fix_joins);
  w.end();
  w.begin(CKPT_REMOVED);
  w.put<uint64_t>(s.removed.size());
  for (const CkptRemoved& r : s.removed) { w.put(r.step); w.put(r.near); w.put(r.far); w.put(r.list); w.put(r.reaction); }
  w.end();
  w.begin(CKPT_EVENTS);
  w.put_array(s.ev_a); w.put_array(s.ev_b); w.put_array(s.ev_r); w.put_array(s.ev_d2); w.put_array(s.ev_intra); w.put_array(s.ev_block_step); w.put_array(s.ev_block_first);
  w.end();
  w.begin(CKPT_ATRP);
  w.put(s.atrp_ratio_activator); w.put(s.atrp_ratio_deactivator); w.put<uint64_t>(s.atrp_stats.size());
  for (const chem_atrp_stats& a : s.atrp_stats) { w.put(a.step); w.put(a.candidates); w.put(a.selected); w.put(a.activated); w.put(a.deactivated); w.put(a.ratio_activator); w.put(a.ratio_deactivator); }
  w.end();
  w.put<uint32_t>(kCkptEnd); w.put<uint32_t>(0); w.put<uint64_t>(8);      // (its length is known: the sum covers it)
  w.put<uint64_t>(ckpt_checksum(w.b.data(), w.b.size()));
  return std::move(w.b);
}

// ---- reader ---------------------------------------------------------------------------------------------------------------
// Reads inside [pos, lim) only; lim never lies behind the end of the blob.  The first failure sticks (`why`), every later get
// returns zeros and empty arrays.
struct CkptReader {
  const uint8_t* p = nullptr; size_t pos = 0, lim = 0; std::string why; const char* section = "";
  bool ok() const { return why.empty(); }
  void bad(const std::string& m) { if (why.empty()) why = std::string("section ") + section + ": " + m; }
  template <class T> T get() {
    T v{};
    if (!ok()) return v;
    if (lim - pos < sizeof(T)) { bad("shorter than its content"); return v; }
    std::memcpy(&v, p + pos, sizeof(T)); pos += sizeof(T);
    return v;
  }
  // a count of records of `bytes_each` bytes that still have to fit into the section
  uint64_t get_count(size_t bytes_each) {
    const uint64_t c = get<uint64_t>();
    if (!ok()) return 0;
    if (c > (lim - pos) / bytes_each) { bad("a count of " + std::to_string(c) + " overflows the section"); return 0; }
    return c;
  }
  template <class T> void get_array(std::vector<T>& v) {
    const uint64_t c = get_count(sizeof(T));
    v.resize((size_t)c);
    if (c) { std::memcpy(v.data(), p + pos, (size_t)c * sizeof(T)); pos += (size_t)c * sizeof(T); }
  }
  void expect(bool cond, const char* m) { if (!cond) bad(m); }
};

inline void ckpt_get_records(CkptReader& r, std::vector<FixRecord>& v) {
  const uint64_t c = r.get_count(32);
  v.resize((size_t)c);
  for (FixRecord& x : v) { x.step = r.get<int64_t>(); x.set = r.get<int32_t>(); x.anchor = r.get<int32_t>(); x.target = r.get<int32_t>(); x.cause = r.get<int32_t>(); x.seq = r.get<int64_t>(); }
}

// 0 and `out`, or CHEM_EINVAL and `why`.  `precision` and `ctx` are the loading context's.
inline int ckpt_read(const void* buf, int64_t nbytes, int precision, const CkptFingerprint& ctx, CkptState& out, std::string& why) {
  auto refuse = [&](const std::string& m) { why = "checkpoint: " + m; return CHEM_EINVAL; };
  if (!buf || nbytes < 0) return refuse("no blob");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  const size_t n = (size_t)nbytes;
  if (n < kCkptHeaderBytes) return refuse("truncated: " + std::to_string(n) + " bytes are less than a header");
  uint32_t hdr[4];
  std::memcpy(hdr, p, 16);
  if (hdr[0] != kCkptMagic) return refuse("bad magic: not a checkpoint blob");
  if (hdr[1] != kCkptVersion) return refuse("unknown format version " + std::to_string(hdr[1]) + " (this build reads version " + std::to_string(kCkptVersion) + ")");
  if (hdr[2] != (uint32_t)precision) return refuse("precision mismatch: the blob was written by a CHEM_PREC_F" + std::to_string(hdr[2]) + " context, this one is CHEM_PREC_F" + std::to_string(precision));
  // the section walk: every header and every length against the bytes that are left
  size_t start[kCkptSectionCount], len[kCkptSectionCount], pos = kCkptHeaderBytes;
  for (size_t k = 0; k < kCkptSectionCount; ++k) {
    const std::string name = kCkptSections[k].name;
    if (n - pos < kCkptSectionHeaderBytes) return refuse("truncated in front of section " + name);
    uint32_t id; uint64_t l;
    std::memcpy(&id, p + pos, 4); std::memcpy(&l, p + pos + 8, 8);
    if (id != kCkptSections[k].id) return refuse("corrupt: section " + name + " expected, found id " + std::to_string(id));
    pos += kCkptSectionHeaderBytes;
    if (l > n - pos) return refuse("truncated or corrupt: the length of section " + name + " (" + std::to_string(l) + ") is larger than the rest of the blob (" + std::to_string(n - pos) + ")");
    start[k] = pos; len[k] = (size_t)l; pos += (size_t)l;
  }
  if (pos != n) return refuse("corrupt: " + std::to_string(n - pos) + " bytes behind the last section");
  const size_t kend = kCkptSectionCount - 1;
  if (len[kend] != 8) return refuse("corrupt: the end section holds " + std::to_string(len[kend]) + " bytes instead of a checksum");
  uint64_t sum;
  std::memcpy(&sum, p + start[kend], 8);
  if (sum != ckpt_checksum(p, start[kend])) return refuse("checksum mismatch: the blob is corrupt");

  CkptReader r;
  r.p = p;
  auto open = [&](size_t k) { r.pos = start[k]; r.lim = start[k] + len[k]; r.section = kCkptSections[k].name; };
  auto close = [&]() { if (r.ok() && r.pos != r.lim) r.bad(std::to_string(r.lim - r.pos) + " bytes behind its content"); };
  size_t k = 0;
  // fingerprint
  CkptFingerprint fp;
  open(k++);
  fp.max_lists = r.get<int32_t>(); fp.max_types = r.get<int32_t>(); fp.max_reactions = r.get<int32_t>(); fp.max_pot_params = r.get<int32_t>(); fp.max_fix_sets = r.get<int32_t>();
  {
    const int32_t nl = r.get<int32_t>();
    if (r.ok() && (nl < 0 || (size_t)nl > (r.lim - r.pos) / 16)) r.bad("a list count of " + std::to_string(nl) + " overflows the section");
    fp.lists.resize(r.ok() ? (size_t)nl : 0);
    for (CkptListKind& l : fp.lists) { l.arity = r.get<int32_t>(); l.kind = r.get<int32_t>(); l.by_types = r.get<int32_t>(); l.hybrid = r.get<int32_t>(); }
  }
  fp.n_reactions = r.get<int32_t>(); fp.n_dissociations = r.get<int32_t>(); fp.n_fix_sets = r.get<int32_t>(); fp.atrp_on = r.get<int32_t>(); fp.npart = r.get<int64_t>();
  close();
  if (!r.ok()) return refuse(r.why);
  const std::string diff = ckpt_fingerprint_diff(fp, ctx);
  if (!diff.empty()) return refuse("the configuration differs from the one the blob was saved under: " + diff);
  const uint64_t np = (uint64_t)fp.npart;
  auto tag_ok = [&](int32_t t) { return t >= 0 && (uint64_t)t < np; };

  CkptState s;
  open(k++);      // core
  s.step = r.get<int64_t>(); for (double& l : s.L) l = r.get<double>(); s.react_on = r.get<int32_t>(); s.ran = r.get<int32_t>();
  close();
  r.expect(s.step >= 0, "negative step");
  for (double l : s.L) r.expect(std::isfinite(l) && l > 0, "box edge not positive and finite");
  open(k++);      // barostat
  s.baro_kind = r.get<int32_t>(); s.baro_p_last = r.get<double>(); s.pist_pe = r.get<double>(); s.pist_eps = r.get<double>(); s.pist_sv = r.get<double>(); s.pist_mu = r.get<double>();
  s.baro_charge = r.get<double>(); s.baro_charge_ref = r.get<double>();
  close();
  r.expect(s.baro_kind >= 0 && s.baro_kind <= 2, "unknown barostat kind");
  r.expect(std::isfinite(s.pist_pe) && std::isfinite(s.pist_sv) && std::isfinite(s.pist_mu) && s.pist_mu > 0, "piston state not finite");
  open(k++);      // particles
  r.get_array(s.id); r.get_array(s.type); r.get_array(s.state); r.get_array(s.res_id); r.get_array(s.mol_id); r.get_array(s.mass); r.get_array(s.q);
  r.get_array(s.pos); r.get_array(s.image); r.get_array(s.vel);
  close();
  if (r.ok()) {
    r.expect(s.id.size() == np && s.type.size() == np && s.state.size() == np && s.res_id.size() == np && s.mol_id.size() == np && s.mass.size() == np && s.q.size() == np &&
             s.pos.size() == 3 * np && s.image.size() == 3 * np && s.vel.size() == 3 * np, "array lengths do not match the particle count");
    for (size_t t = 0; r.ok() && t < s.id.size(); ++t) {
      r.expect(t == 0 || s.id[t] > s.id[t - 1], "particle ids not ascending");
      r.expect(s.type[t] >= 0 && s.type[t] < CHEM_MAX_TYPES, "particle type out of range");
      r.expect(std::isfinite(s.mass[t]) && s.mass[t] > 0 && std::isfinite(s.q[t]), "mass not positive or charge not finite");
      r.expect(tag_ok(s.mol_id[t]), "mol_id is not a particle");
      for (int d = 0; d < 3; ++d) r.expect(std::isfinite(s.pos[3 * t + d]) && std::isfinite(s.vel[3 * t + d]), "position or velocity not finite");
    }
  }
  open(k++);      // resolution
  r.get_array(s.res_lambda0); r.get_array(s.res_s0); r.get_array(s.res_seen);
  close();
  if (r.ok()) {
    r.expect(s.res_lambda0.size() == s.res_s0.size() && s.res_s0.size() == s.res_seen.size() && (s.res_lambda0.empty() || s.res_lambda0.size() == np), "stamp arrays do not match the particle count");
    for (size_t t = 0; r.ok() && t < s.res_lambda0.size(); ++t)
      r.expect(s.res_lambda0[t] >= 0.0 && s.res_lambda0[t] <= 1.0 && s.res_s0[t] >= 0 && s.res_s0[t] <= s.step && s.res_seen[t] >= 0 && s.res_seen[t] < CHEM_MAX_TYPES, "stamp out of range");
  }
  open(k++);      // lists
  {
    const uint64_t nl = r.get_count(16);
    if (r.ok() && nl != fp.lists.size()) r.bad("list count does not match the fingerprint");
    s.lists.resize(r.ok() ? (size_t)nl : 0);
    for (size_t li = 0; r.ok() && li < s.lists.size(); ++li) {
      CkptState::List& l = s.lists[li];
      r.get_array(l.ent); r.get_array(l.birth);
      if (!r.ok()) break;
      const CkptListKind& kd = fp.lists[li];
      r.expect(kd.arity >= 2 && kd.arity <= 4 && l.ent.size() % (size_t)kd.arity == 0, "entries are no multiple of the arity");
      r.expect(l.birth.size() == (kd.hybrid ? l.ent.size() / (size_t)kd.arity : 0), "birth steps do not match the entries");
      for (int32_t t : l.ent) if (!tag_ok(t)) { r.bad("entry names no particle"); break; }
      for (int64_t b : l.birth) if (b < 0 || b > s.step) { r.bad("birth step outside [0, step]"); break; }
    }
  }
  close();
  open(k++);      // exclusions
  r.get_array(s.excl);
  close();
  r.expect(s.excl.size() % 2 == 0, "odd number of tags");
  for (size_t e = 0; r.ok() && e + 1 < s.excl.size(); e += 2) r.expect(tag_ok(s.excl[e]) && tag_ok(s.excl[e + 1]) && s.excl[e] != s.excl[e + 1], "pair names no two particles");
  open(k++);      // graph
  r.get_array(s.graph);
  close();
  r.expect(s.graph.size() % 2 == 0, "odd number of tags");
  for (size_t e = 0; r.ok() && e + 1 < s.graph.size(); e += 2) r.expect(tag_ok(s.graph[e]) && tag_ok(s.graph[e + 1]) && s.graph[e] < s.graph[e + 1], "bond names no two particles in order");
  open(k++);      // fix
  {
    const uint64_t ns = r.get_count(16);
    if (r.ok() && ns != (uint64_t)fp.n_fix_sets) r.bad("set count does not match the fingerprint");
    s.fix_sets.resize(r.ok() ? (size_t)ns : 0);
    for (CkptState::FixSetState& f : s.fix_sets) {
      f.next_seq = r.get<int64_t>();
      const uint64_t ne = r.get_count(24);
      f.ent.resize((size_t)ne);
      for (FixEntry& e : f.ent) {
        e.anchor = r.get<int32_t>(); e.target = r.get<int32_t>(); e.dist = r.get<double>(); e.seq = r.get<int64_t>();
        r.expect(tag_ok(e.anchor) && tag_ok(e.target) && e.anchor != e.target && std::isfinite(e.dist) && e.dist > 0 && e.seq >= 0 && e.seq < f.next_seq, "entry out of range");
      }
    }
    ckpt_get_records(r, s.fix_log); ckpt_get_records(r, s.fix_joins);
    for (const std::vector<FixRecord>* v : {&s.fix_log, &s.fix_joins})
      for (const FixRecord& x : *v) r.expect(x.set >= 0 && x.set < fp.n_fix_sets && tag_ok(x.anchor) && tag_ok(x.target) && x.step >= 0 && x.step <= s.step, "record out of range");
  }
  close();
  open(k++);      // removed
  {
    const uint64_t nr = r.get_count(24);
    s.removed.resize((size_t)nr);
    for (CkptRemoved& x : s.removed) {
      x.step = r.get<int64_t>(); x.near = r.get<int32_t>(); x.far = r.get<int32_t>(); x.list = r.get<int32_t>(); x.reaction = r.get<int32_t>();
      r.expect(tag_ok(x.near) && tag_ok(x.far) && x.list >= 0 && (size_t)x.list < fp.lists.size() && x.step >= 0 && x.step <= s.step, "record out of range");
    }
  }
  close();
  open(k++);      // events
  r.get_array(s.ev_a); r.get_array(s.ev_b); r.get_array(s.ev_r); r.get_array(s.ev_d2); r.get_array(s.ev_intra); r.get_array(s.ev_block_step); r.get_array(s.ev_block_first);
  close();
  if (r.ok()) {
    const size_t ne = s.ev_a.size();
    r.expect(s.ev_b.size() == ne && s.ev_r.size() == ne && s.ev_d2.size() == ne && s.ev_intra.size() <= ne && s.ev_block_step.size() == s.ev_block_first.size(), "array lengths disagree");
    r.expect(ne == 0 || !s.ev_block_first.empty(), "records without a block");
    for (size_t e = 0; r.ok() && e < ne; ++e)
      r.expect(tag_ok(s.ev_a[e]) && tag_ok(s.ev_b[e]) && s.ev_r[e] >= -(int32_t)fp.n_dissociations && s.ev_r[e] < fp.n_reactions, "record out of range");
    for (size_t b = 0; r.ok() && b < s.ev_block_first.size(); ++b)
      r.expect(s.ev_block_first[b] <= ne && (b == 0 ? s.ev_block_first[b] == 0 : s.ev_block_first[b] >= s.ev_block_first[b - 1]) && s.ev_block_step[b] >= 0 && s.ev_block_step[b] <= s.step &&
               (b == 0 || s.ev_block_step[b] >= s.ev_block_step[b - 1]), "block out of order");
  }
  open(k++);      // atrp
  s.atrp_ratio_activator = r.get<double>(); s.atrp_ratio_deactivator = r.get<double>();
  {
    const uint64_t na = r.get_count(56);
    s.atrp_stats.resize((size_t)na);
    for (chem_atrp_stats& a : s.atrp_stats) {
      a.step = r.get<int64_t>(); a.candidates = r.get<int64_t>(); a.selected = r.get<int64_t>(); a.activated = r.get<int64_t>(); a.deactivated = r.get<int64_t>();
      a.ratio_activator = r.get<double>(); a.ratio_deactivator = r.get<double>();
    }
  }
  close();
  if (!r.ok()) return refuse(r.why);
  out = std::move(s);
  why.clear();
  return 0;
}

}  // namespace chem
