// Test harness (CPU only): drives the checkpoint writer and reader of chemlab_amd/csrc/chem_ckpt_host.hpp (ckpt_write, ckpt_read,
// the fingerprint compare, the checksum) from a plain-text script on stdin.  A program of its own, so that it can also be built
// with -fsanitize=address,undefined: every blob is read from a heap block of exactly its size, so a read past nbytes is a
// report, not luck.  Not part of the product library.
//   fp <npart> <reactions> <dissociations> <fix sets> <atrp> <nlists> {<arity> <kind> <by_types> <hybrid>}...   the context's fingerprint
//   fpset <field> <value>          one field of it: max_lists max_types max_reactions max_pot_params max_fix_sets nlists n_reactions
//                                  n_dissociations n_fix_sets atrp_on npart, or list.<i>.arity | kind | by_types | hybrid
//   prec <32 | 64>                 the context's precision (write and read)
//   synth <seed> <full | empty>    a synthetic state that fits the fingerprint: every section filled, or empty lists, no events, ...
//   write                          state -> blob; prints "wrote <bytes>"
//   hex                            prints "hex <blob>"
//   blob <hex>                     blob <- hex
//   read                           blob -> state through ckpt_read; prints "read 0", or "read <code> <reason>" (the state stays)
//   same                           prints "same 1" if the state equals the last synthetic one, field by field
//   sizes                          prints "sizes" and the element count of every part of the state
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include "../../chemlab_amd/csrc/chem_ckpt_host.hpp"
using namespace chem;

struct Rng {      // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  int64_t below(int64_t n) { return n > 0 ? (int64_t)(next() % (uint64_t)n) : 0; }
  double u() { return (double)(next() >> 11) / 9007199254740992.0; }
};

static CkptState synth(const CkptFingerprint& fp, uint64_t seed, bool full) {
  Rng g{seed};
  CkptState s;
  const int64_t n = fp.npart;
  s.step = full ? 1237 : 0; s.L[0] = 11.5; s.L[1] = 12.25 + g.u(); s.L[2] = 13.0 + g.u(); s.react_on = full; s.ran = full;
  if (full) { s.baro_kind = 2; s.baro_p_last = g.u(); s.pist_pe = g.u() - 0.5; s.pist_eps = s.pist_pe / 50.0; s.pist_sv = 1.0 - 1e-3 * g.u(); s.pist_mu = 1.0 + 1e-3 * g.u(); }
  for (int64_t t = 0; t < n; ++t) {
    s.id.push_back(10 + 3 * t); s.type.push_back((int32_t)g.below(CHEM_MAX_TYPES)); s.state.push_back((int32_t)g.below(5)); s.res_id.push_back((int32_t)g.below(1000));
    s.mol_id.push_back((int32_t)g.below(t + 1)); s.mass.push_back(0.5 + g.u()); s.q.push_back(g.u() - 0.5);
    for (int d = 0; d < 3; ++d) { s.pos.push_back(s.L[d] * (g.u() * 1.2 - 0.1)); s.image.push_back((int32_t)g.below(7) - 3); s.vel.push_back(g.u() - 0.5); }
  }
  if (full) for (int64_t t = 0; t < n; ++t) { s.res_lambda0.push_back(g.u()); s.res_s0.push_back(g.below(s.step + 1)); s.res_seen.push_back((int32_t)g.below(CHEM_MAX_TYPES)); }
  s.lists.resize(fp.lists.size());
  for (size_t l = 0; full && l < fp.lists.size(); ++l) {
    const int64_t ne = 3 + g.below(5);
    for (int64_t e = 0; e < ne * fp.lists[l].arity; ++e) s.lists[l].ent.push_back((int32_t)g.below(n));
    if (fp.lists[l].hybrid && fp.lists[l].arity == 2) for (int64_t e = 0; e < ne; ++e) s.lists[l].birth.push_back(g.below(s.step + 1));
  }
  auto pair = [&](std::vector<int32_t>& v, bool ordered) {
    int32_t a = (int32_t)g.below(n - 1), b = a + 1 + (int32_t)g.below(n - 1 - a);
    if (!ordered && (g.next() & 1)) std::swap(a, b);
    v.push_back(a); v.push_back(b);
  };
  if (full) for (int k = 0; k < 9; ++k) { pair(s.excl, false); pair(s.graph, true); }
  s.fix_sets.resize((size_t)fp.n_fix_sets);
  auto record = [&](int cause) {
    FixRecord r{};
    r.step = g.below(s.step + 1); r.set = (int32_t)g.below(fp.n_fix_sets); r.anchor = (int32_t)g.below(n); r.target = (int32_t)g.below(n); r.cause = cause; r.seq = cause == 4 ? -1 : g.below(20);
    return r;
  };
  if (full && fp.n_fix_sets > 0) {
    for (CkptState::FixSetState& f : s.fix_sets) {
      f.next_seq = 20;
      for (int k = 0; k < 4; ++k) { const int32_t a = (int32_t)g.below(n - 1); f.ent.push_back(FixEntry{a, a + 1, 0.5 + g.u(), (int64_t)(3 * k + g.below(3))}); }
    }
    for (int k = 0; k < 5; ++k) { s.fix_log.push_back(record(1 + (int)g.below(2))); s.fix_joins.push_back(record(3 + (int)g.below(2))); }
  }
  if (full && !fp.lists.empty())
    for (int k = 0; k < 6; ++k) s.removed.push_back(CkptRemoved{g.below(s.step + 1), (int32_t)g.below(n), (int32_t)g.below(n), (int32_t)g.below((int64_t)fp.lists.size()), (int32_t)g.below(4)});
  if (full && fp.n_reactions + fp.n_dissociations > 0) {
    int64_t at = 0;
    for (int b = 0; b < 4; ++b) {
      at += 1 + g.below(300);
      s.ev_block_step.push_back(at); s.ev_block_first.push_back(s.ev_a.size());
      for (int64_t e = 0, ne = g.below(6); e < ne; ++e) {
        s.ev_a.push_back((int32_t)g.below(n)); s.ev_b.push_back((int32_t)g.below(n));
        s.ev_r.push_back((int32_t)g.below(fp.n_reactions + fp.n_dissociations) - fp.n_dissociations); s.ev_d2.push_back(g.u());
      }
    }
    s.ev_a.push_back(0); s.ev_b.push_back(1); s.ev_r.push_back(fp.n_reactions > 0 ? 0 : -1); s.ev_d2.push_back(1.0);      // (at least one record)
    for (size_t e = 0; e + 1 < s.ev_a.size(); ++e) s.ev_intra.push_back((int8_t)(g.next() & 1));      // (the flags may lag the records)
  }
  if (full && fp.atrp_on) {
    s.atrp_ratio_activator = g.u(); s.atrp_ratio_deactivator = g.u();
    for (int k = 0; k < 3; ++k) s.atrp_stats.push_back(chem_atrp_stats{100 * (k + 1), g.below(50), g.below(20), g.below(5), g.below(5), g.u(), g.u()});
  }
  return s;
}

template <class T> static bool eq(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static bool eq_rec(const std::vector<FixRecord>& a, const std::vector<FixRecord>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k)
    if (a[k].step != b[k].step || a[k].set != b[k].set || a[k].anchor != b[k].anchor || a[k].target != b[k].target || a[k].cause != b[k].cause || a[k].seq != b[k].seq) return false;
  return true;
}
static bool bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool same(const CkptState& a, const CkptState& b) {
  bool ok = a.step == b.step && a.react_on == b.react_on && a.ran == b.ran && a.baro_kind == b.baro_kind;
  for (int d = 0; d < 3; ++d) ok = ok && bits(a.L[d], b.L[d]);
  ok = ok && bits(a.baro_p_last, b.baro_p_last) && bits(a.pist_pe, b.pist_pe) && bits(a.pist_eps, b.pist_eps) && bits(a.pist_sv, b.pist_sv) && bits(a.pist_mu, b.pist_mu) &&
       bits(a.baro_charge, b.baro_charge) && bits(a.baro_charge_ref, b.baro_charge_ref);
  ok = ok && eq(a.id, b.id) && eq(a.type, b.type) && eq(a.state, b.state) && eq(a.res_id, b.res_id) && eq(a.mol_id, b.mol_id) && eq(a.mass, b.mass) && eq(a.q, b.q) &&
       eq(a.pos, b.pos) && eq(a.image, b.image) && eq(a.vel, b.vel) && eq(a.res_lambda0, b.res_lambda0) && eq(a.res_s0, b.res_s0) && eq(a.res_seen, b.res_seen);
  ok = ok && a.lists.size() == b.lists.size();
  for (size_t l = 0; ok && l < a.lists.size(); ++l) ok = eq(a.lists[l].ent, b.lists[l].ent) && eq(a.lists[l].birth, b.lists[l].birth);
  ok = ok && eq(a.excl, b.excl) && eq(a.graph, b.graph) && a.fix_sets.size() == b.fix_sets.size();
  for (size_t f = 0; ok && f < a.fix_sets.size(); ++f) {
    ok = a.fix_sets[f].next_seq == b.fix_sets[f].next_seq && a.fix_sets[f].ent.size() == b.fix_sets[f].ent.size();
    for (size_t e = 0; ok && e < a.fix_sets[f].ent.size(); ++e) {
      const FixEntry &x = a.fix_sets[f].ent[e], &y = b.fix_sets[f].ent[e];
      ok = x.anchor == y.anchor && x.target == y.target && bits(x.dist, y.dist) && x.seq == y.seq;
    }
  }
  ok = ok && eq_rec(a.fix_log, b.fix_log) && eq_rec(a.fix_joins, b.fix_joins) && a.removed.size() == b.removed.size();
  for (size_t k = 0; ok && k < a.removed.size(); ++k) {
    const CkptRemoved &x = a.removed[k], &y = b.removed[k];
    ok = x.step == y.step && x.near == y.near && x.far == y.far && x.list == y.list && x.reaction == y.reaction;
  }
  ok = ok && eq(a.ev_a, b.ev_a) && eq(a.ev_b, b.ev_b) && eq(a.ev_r, b.ev_r) && eq(a.ev_d2, b.ev_d2) && eq(a.ev_intra, b.ev_intra) && eq(a.ev_block_step, b.ev_block_step) &&
       eq(a.ev_block_first, b.ev_block_first);
  ok = ok && bits(a.atrp_ratio_activator, b.atrp_ratio_activator) && bits(a.atrp_ratio_deactivator, b.atrp_ratio_deactivator) && a.atrp_stats.size() == b.atrp_stats.size();
  for (size_t k = 0; ok && k < a.atrp_stats.size(); ++k) {
    const chem_atrp_stats &x = a.atrp_stats[k], &y = b.atrp_stats[k];
    ok = x.step == y.step && x.candidates == y.candidates && x.selected == y.selected && x.activated == y.activated && x.deactivated == y.deactivated &&
         bits(x.ratio_activator, y.ratio_activator) && bits(x.ratio_deactivator, y.ratio_deactivator);
  }
  return ok;
}

int main() {
  CkptFingerprint fp;
  CkptState st, st0;
  std::vector<uint8_t> blob;
  int prec = 64;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd; is >> cmd;
    if (cmd == "fp") {
      fp = CkptFingerprint{};
      size_t nl = 0;
      is >> fp.npart >> fp.n_reactions >> fp.n_dissociations >> fp.n_fix_sets >> fp.atrp_on >> nl;
      fp.lists.resize(nl);
      for (CkptListKind& l : fp.lists) is >> l.arity >> l.kind >> l.by_types >> l.hybrid;
    }
    else if (cmd == "fpset") {
      std::string f; long long v; is >> f >> v;
      if (f == "max_lists") fp.max_lists = (int32_t)v; else if (f == "max_types") fp.max_types = (int32_t)v; else if (f == "max_reactions") fp.max_reactions = (int32_t)v;
      else if (f == "max_pot_params") fp.max_pot_params = (int32_t)v; else if (f == "max_fix_sets") fp.max_fix_sets = (int32_t)v; else if (f == "nlists") fp.lists.resize((size_t)v, CkptListKind{2, 1, 0, 0});
      else if (f == "n_reactions") fp.n_reactions = (int32_t)v; else if (f == "n_dissociations") fp.n_dissociations = (int32_t)v; else if (f == "n_fix_sets") fp.n_fix_sets = (int32_t)v;
      else if (f == "atrp_on") fp.atrp_on = (int32_t)v; else if (f == "npart") fp.npart = v;
      else if (f.rfind("list.", 0) == 0) {
        const size_t dot = f.find('.', 5);
        CkptListKind& l = fp.lists.at((size_t)std::stoul(f.substr(5, dot - 5)));
        const std::string m = f.substr(dot + 1);
        if (m == "arity") l.arity = (int32_t)v; else if (m == "kind") l.kind = (int32_t)v; else if (m == "by_types") l.by_types = (int32_t)v; else if (m == "hybrid") l.hybrid = (int32_t)v;
        else { printf("unknown field\n"); return 1; }
      }
      else { printf("unknown field\n"); return 1; }
    }
    else if (cmd == "prec") is >> prec;
    else if (cmd == "synth") { unsigned long long seed; std::string mode; is >> seed >> mode; st = synth(fp, seed, mode == "full"); st0 = st; }
    else if (cmd == "write") { blob = ckpt_write(prec, fp, st); printf("wrote %zu\n", blob.size()); }
    else if (cmd == "hex") { printf("hex "); for (uint8_t b : blob) printf("%02x", b); printf("\n"); }
    else if (cmd == "blob") {
      std::string h; is >> h;
      blob.clear();
      for (size_t k = 0; k + 1 < h.size(); k += 2) blob.push_back((uint8_t)std::stoul(h.substr(k, 2), nullptr, 16));
    }
    else if (cmd == "read") {
      std::unique_ptr<uint8_t[]> exact(new uint8_t[blob.size() ? blob.size() : 1]);      // exactly nbytes: the sanitizer sees any read beyond
      if (!blob.empty()) std::memcpy(exact.get(), blob.data(), blob.size());
      CkptState got; std::string why;
      const int rc = ckpt_read(exact.get(), (int64_t)blob.size(), prec, fp, got, why);
      if (rc == 0) { st = std::move(got); printf("read 0\n"); } else printf("read %d %s\n", rc, why.c_str());
      if ((rc != 0) != !why.empty()) { printf("refusal without a reason\n"); return 1; }
    }
    else if (cmd == "same") printf("same %d\n", same(st, st0) ? 1 : 0);
    else if (cmd == "sizes") {
      size_t ent = 0, birth = 0, fixe = 0;
      for (const auto& l : st.lists) { ent += l.ent.size(); birth += l.birth.size(); }
      for (const auto& f : st.fix_sets) fixe += f.ent.size();
      printf("sizes %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", st.id.size(), st.res_lambda0.size(), ent, birth, st.excl.size(), st.graph.size(), fixe, st.fix_log.size(),
             st.fix_joins.size(), st.removed.size(), st.ev_a.size(), st.ev_block_step.size(), st.atrp_stats.size());
    }
  }
  return 0;
}
