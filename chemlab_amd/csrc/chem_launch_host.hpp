// Which force kernel runs.  The pair-force kernels exist in a fixed set of instantiations -- lanes per
// particle, block size, MODE, ENERGY, DIAG -- and every option and registered feature narrows what may be launched.  This
// header is that rule, free of HIP: CtxT::launch_pair, CtxT::set_tile_lds_attr and the bonded tail of CtxT::compute_forces
// (chem_api.hip) call it and turn its answer into an instantiation in one place each; tests/host/launch_harness.cpp checks it
// on the CPU.  A new mode is registered here: a row in tile_variant_built / row_variant_built, its place in pair_plan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/chem_mi355.h"

namespace chem {

// ---- pair forces ----------------------------------------------------------------------------------------------------------
// MODE of the tile kernels: 0 general (linear tables), 1 LJ only, 2 one LJ parameter set, 3 general with cubic tables,
// 4 general + Coulomb, 5 general + resolution scaling, 6 general + capped pairs, 7 resolution + capped.
enum class PairFamily { tiles, rows };      // LDS-staged tiles (k_pair_tiles*) / one neighbour row per particle (k_pair_force*)
struct PairVariant {
  PairFamily family;
  int mode;        // tiles: 0..7; rows: 0 (the plain kernel, `cubic` says which build) or 4..7
  int tpp;         // lanes per particle
  int block;       // threads per block
  bool energy;     // the ENERGY instantiation (observe())
  bool diag;       // tiles: the DIAG instantiation (options debug_stamps / ablate)
  bool cubic;      // rows: the CUBIC instantiation
};

// The built set, tiles: what the library holds with its dynamic-LDS limit raised, and all that pair_plan may answer.
constexpr bool tile_variant_built(int mode, int tpp, int block, bool energy, bool diag) {
  const bool one_lane_512 = tpp == 1 && block == 512;
  if (mode >= 4 && mode <= 7) return one_lane_512 && !diag;      // one instantiation per ENERGY
  if (mode < 0 || mode > 3) return false;
  if (!(tpp == 1 || tpp == 2 || tpp == 4 || tpp == 8) || !(block == 256 || block == 512 || block == 1024)) return false;
  if (energy) return !diag && (mode == 0 || mode == 3);          // energies are evaluated by the general kernels only
  return !diag || one_lane_512;
}
// Instantiations the library carries beside the built set and launches from nowhere: the ENERGY builds of MODE 1 and 2 and
// of DIAG.  (The dispatch this header replaced named them under run-time tests.  They stay so that the device code stays
// what it was; they get no LDS limit and pair_plan never answers one.)
constexpr bool tile_variant_unlaunched(int mode, int tpp, int block, bool energy, bool diag) {
  return energy && !tile_variant_built(mode, tpp, block, true, diag) && tile_variant_built(mode, tpp, block, false, diag);
}
// ... rows: 256 threads, no DIAG; the feature kernels with four lanes per particle only
constexpr bool row_variant_built(int mode, int tpp, bool cubic) {
  if (mode == 4) return tpp == 4 && cubic;
  if (mode >= 5 && mode <= 7) return tpp == 4 && !cubic;
  return mode == 0 && (tpp == 1 || tpp == 2 || tpp == 4 || tpp == 8 || tpp == 16 || tpp == 32 || tpp == 64);
}
inline bool variant_built(const PairVariant& v) {
  if (v.family == PairFamily::tiles) return !v.cubic && tile_variant_built(v.mode, v.tpp, v.block, v.energy, v.diag);
  return !v.diag && v.block == 256 && row_variant_built(v.mode, v.tpp, v.cubic);
}
// f(const PairVariant&) for every member of the tile family's built set
template <class F> void for_each_tile_variant(F&& f) {
  for (int mode = 0; mode < 8; ++mode)
    for (int tpp : {1, 2, 4, 8})
      for (int block : {256, 512, 1024})
        for (int e = 0; e < 2; ++e)
          for (int d = 0; d < 2; ++d)
            if (tile_variant_built(mode, tpp, block, e != 0, d != 0)) f(PairVariant{PairFamily::tiles, mode, tpp, block, e != 0, d != 0, false});
}

// what CtxT knows when it is about to launch the pair forces
struct PairInput {
  bool use_tiles; int n;
  int opt_tpp, pair_bs;            // options tpp (0: automatic) and pair_block
  bool energy;
  bool coul, res, cap;             // a Coulomb pair is registered / a resolution pair is marked / a pair is capped
  bool lj_only, uniform_lj, cubic_tab;
  bool diag;                       // option debug_stamps or ablate
  int res_a, res_b, cap_a, cap_b;  // first marked / first capped type pair (first_res_pair, first_cap_pair): read by the refusals that name one
};

// lanes per particle
inline int pick_tpp(bool use_tiles, int n, int opt_tpp) {
  if (opt_tpp > 0) return use_tiles ? std::min(opt_tpp, 8) : opt_tpp;
  if (use_tiles) return 1;   // one lane per home particle at every size (measured 10k..1M particles after the ds_read_b128 fix: 125k particles 17.4 us against 20.6 with two lanes)
  return n >= 100000 ? 4 : (n >= 8000 ? 8 : 16);
}

enum class PairRefusal { none, tpp_limit, block_limit, res_next_to_coul, cap_next_to_coul, diag_feature, diag_shape };
struct PairPlan {
  int code;              // CHEM_OK: launch `v`; otherwise the error code of the refusal, its text from pair_refusal_text
  PairVariant v;
  PairRefusal why;
  int feature;           // refusals: 0 Coulomb, 1 resolution, 2 caps
  int a, b;              // refusals: the option's value, or the type pair
};

inline PairPlan pair_plan(const PairInput& in) {
  PairPlan p{CHEM_OK, PairVariant{in.use_tiles ? PairFamily::tiles : PairFamily::rows, 0, 1, 512, in.energy, false, false}, PairRefusal::none, 0, 0, 0};
  auto refuse = [&p](int code, PairRefusal why, int feature, int a, int b) { p.code = code; p.why = why; p.feature = feature; p.a = a; p.b = b; return p; };
  // the kernels with a Coulomb term, the resolution scaling or cap radii are built for one lane per particle and 512-thread
  // blocks, and the last two not next to the Coulomb term
  const bool on[3] = {in.coul, in.res, in.cap};
  for (int f = 0; f < 3; ++f) {
    if (!on[f]) continue;
    if (f == 1 && in.coul) return refuse(CHEM_ENOTIMPL, PairRefusal::res_next_to_coul, f, std::min(in.res_a, in.res_b), std::max(in.res_a, in.res_b));
    if (f == 2 && in.coul) return refuse(CHEM_ENOTIMPL, PairRefusal::cap_next_to_coul, f, in.cap_a, in.cap_b);
    if (in.opt_tpp > 1) return refuse(CHEM_EINVAL, PairRefusal::tpp_limit, f, in.opt_tpp, 0);
    if (in.pair_bs != 512) return refuse(CHEM_EINVAL, PairRefusal::block_limit, f, in.pair_bs, 0);
  }
  const int mode47 = in.coul ? 4 : in.res ? (in.cap ? 7 : 5) : in.cap ? 6 : 0;
  if (!in.use_tiles) {
    p.v.block = 256;
    if (mode47) { p.v.mode = mode47; p.v.tpp = 4; p.v.cubic = in.coul; }
    else { p.v.tpp = pick_tpp(false, in.n, in.opt_tpp); p.v.cubic = in.cubic_tab; }
    return p;
  }
  if (mode47) {      // (the diagnostics are refused on the ENERGY launch of these as well)
    if (in.diag) return refuse(CHEM_EINVAL, PairRefusal::diag_feature, in.coul ? 0 : in.res ? 1 : 2, 0, 0);
    p.v.mode = mode47;
    return p;
  }
  p.v.mode = in.energy ? (in.cubic_tab ? 3 : 0) : (in.uniform_lj ? 2 : (in.lj_only ? 1 : (in.cubic_tab ? 3 : 0)));
  p.v.tpp = pick_tpp(true, in.n, in.opt_tpp);
  p.v.block = in.pair_bs;
  if (in.diag && !in.energy) {      // diagnostics: one instantiation, one lane per particle, 512 threads
    if (p.v.tpp != 1 || in.pair_bs != 512) return refuse(CHEM_EINVAL, PairRefusal::diag_shape, 0, 0, 0);
    p.v.diag = true;
  }
  return p;
}

// the message of a refusal (built here, off the path of a launch)
inline std::string pair_refusal_text(const PairPlan& p) {
  static const char* const with[3] = {"with a Coulomb pair registered", "with a resolution pair marked", "with a capped pair registered"};
  static const char* const kernel[3] = {"with the Coulomb term", "with the resolution scaling", "with capped pairs"};
  const std::string pair = "(" + std::to_string(p.a) + "," + std::to_string(p.b) + ")";
  switch (p.why) {
    case PairRefusal::tpp_limit: return "option tpp = " + std::to_string(p.a) + ": " + with[p.feature] + " only tpp = 1 (or 0, automatic) is built";
    case PairRefusal::block_limit: return "option pair_block = " + std::to_string(p.a) + ": " + with[p.feature] + " only pair_block = 512 is built";
    case PairRefusal::res_next_to_coul: return "resolution-scaled type pair " + pair + " next to a registered Coulomb pair: the two terms are not served in one context";
    case PairRefusal::cap_next_to_coul: return "capped type pair " + pair + " next to a registered Coulomb pair: the two terms are not served in one context";
    case PairRefusal::diag_feature: return std::string("debug_stamps / ablate are not built for the force kernel ") + kernel[p.feature];
    case PairRefusal::diag_shape: return "debug_stamps / ablate need tpp=1 and pair_block=512";
    case PairRefusal::none: break;
  }
  return std::string();
}

// the first marked resolution pair: the first type with a mark and its first partner (mask[a] bit b: pair (a, b) is marked)
inline void first_res_pair(const uint32_t* mask, int& a, int& b) {
  for (a = 0; a < CHEM_MAX_TYPES && !mask[a]; ++a) {}
  for (b = 0; a < CHEM_MAX_TYPES && b < CHEM_MAX_TYPES && !((mask[a] >> b) & 1u); ++b) {}      // (no mark at all: a = CHEM_MAX_TYPES)
}
// the first capped pair (a <= b) in row order
inline void first_cap_pair(const double (*cap_rad)[CHEM_MAX_TYPES], int& a, int& b) {
  a = b = 0;
  for (int k = CHEM_MAX_TYPES * CHEM_MAX_TYPES; k-- > 0;)
    if (cap_rad[k / CHEM_MAX_TYPES][k % CHEM_MAX_TYPES] > 0 && k / CHEM_MAX_TYPES <= k % CHEM_MAX_TYPES) { a = k / CHEM_MAX_TYPES; b = k % CHEM_MAX_TYPES; }
}

// ---- bonded term behind the pair forces ----------------------------------------------------------------------------------------
enum class BondedLaunch { none, work_list, per_particle };   // nothing / owners of the work list (k_bonded_work*) / every particle (k_bonded*)
enum class BondedKind { plain, hybrid, charged };            // k_bonded(_work) / ..._hyb (lambda of hybrid entries) / ..._q (1-4 Coulomb list)
// the family of a context: a 1-4 Coulomb list takes the charged kernels (which carry the lambda code along), else a hybrid list the hybrid ones
constexpr BondedKind bonded_kind(bool has_coul14, bool has_hybrid) { return has_coul14 ? BondedKind::charged : has_hybrid ? BondedKind::hybrid : BondedKind::plain; }
struct BondedInput {
  long long nbent;           // bonded entries
  bool inline_bonds;         // CtxT::bonds_inline(): the force kernel has evaluated the harmonic bonds
  long long excl_over;       // particles with more exclusions than the force kernel holds slots for
  bool work_list;            // use_fused || dd_on: the last rebuild made the work list
  bool has_coul14, has_hybrid, bonds_only;
  int nb_owner;              // owners on the work list
};
struct BondedPlan {
  BondedLaunch launch; BondedKind kind;
  bool bonds_only;           // work list: the BONDS_ONLY instantiation
  bool inline_bonds;         // work list: it holds the owners with more than kBondSlots exclusions only
  int nown;                  // work list: owners to launch for
};
inline BondedPlan bonded_plan(const BondedInput& in) {
  BondedPlan p{BondedLaunch::none, BondedKind::plain, false, false, 0};
  if (in.nbent <= 0) return p;
  if (in.inline_bonds && in.excl_over == 0) return p;      // all of them were evaluated by the force kernel
  p.kind = bonded_kind(in.has_coul14, in.has_hybrid);
  if (!in.work_list) { p.launch = BondedLaunch::per_particle; return p; }
  p.launch = BondedLaunch::work_list;
  p.bonds_only = in.bonds_only;
  p.inline_bonds = in.inline_bonds;
  p.nown = in.inline_bonds ? (int)std::min<long long>(in.nb_owner, in.excl_over) : in.nb_owner;
  return p;
}
// Inline bonds keep a bonded partner's LDS slot in 16 bits (BondRec, md_kernels.hpp), kBondRecNone = no partner.  A staged tile of
// tile_cap slots numbers them 0 .. tile_cap - 1, so every slot a record can hold stays below the mark while tile_cap does not
// exceed it.  Beyond that CtxT::bonds_inline() answers no and the bonds go to the work list (BondedInput::inline_bonds = false),
// the route of every context the force kernel does not serve.
constexpr unsigned int kBondRecNone = 0xffffu;
constexpr bool bond_records_fit(long long tile_cap) { return tile_cap >= 0 && tile_cap <= (long long)kBondRecNone; }

}  // namespace chem
