// chem_api.hip -- context, run loop and the C ABI of libchem_mi355.so (include/chem_mi355.h).
//
// One context == one GPU.  chem_run() enqueues the whole velocity-Verlet loop on one HIP
// stream with no host round trip per step: the skin-triggered neighbour rebuild is decided on
// the device (k_rebuild_decide) and the rebuild chain early-exits when it is not needed.
// The host only synchronises at reaction steps (every `interval` steps) and at the end.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <thread>
#include <mutex>
#include <exception>
#include <tuple>
#include <type_traits>

#include "chem_comm.hpp"
#include "chem_geom_host.hpp"
#include "chem_idle_host.hpp"
#include "chem_launch_host.hpp"
#include "chem_tensor_host.hpp"
#include "chem_host.hpp"
#include "chem_react_host.hpp"
#include "chem_res_host.hpp"
#include "chem_fix_host.hpp"
#include "chem_region_host.hpp"
#include "chem_rdf_host.hpp"
#include "chem_sq_host.hpp"
#include "chem_ckpt_host.hpp"
#include "chem_tab_host.hpp"
#include "md_kernels.hpp"

namespace chem {

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      throw ChemError(CHEM_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));           \
  } while (0)

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// std::vector storage in pinned host memory: the device tables rebuilt at reaction steps (bonded and
// exclusion CSR, ~14 MB at 10^6 particles) are uploaded at PCIe speed instead of through the
// pageable-copy bounce buffers (2.5 ms -> 0.5 ms)
template <typename T> struct PinnedAlloc {
  using value_type = T;
  PinnedAlloc() = default;
  template <class U> PinnedAlloc(const PinnedAlloc<U>&) {}
  T* allocate(size_t n) { void* p = nullptr; if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc(); return (T*)p; }
  void deallocate(T* p, size_t) { (void)hipHostFree(p); }
  template <class U> bool operator==(const PinnedAlloc<U>&) const { return true; }
  template <class U> bool operator!=(const PinnedAlloc<U>&) const { return false; }
};
template <typename T> using PinnedVec = std::vector<T, PinnedAlloc<T>>;

template <typename T> struct DBuf {
  T* p = nullptr; size_t n = 0;
  void alloc(size_t count) {
    if (count <= n && p) return;
    free();
    HIPCHK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T)));
    n = count;
  }
  void free() { if (p) { (void)hipFree(p); p = nullptr; n = 0; } }
  ~DBuf() { free(); }
  template <class V> void upload(const V& h, hipStream_t s) {
    alloc(h.size());
    if (!h.empty()) HIPCHK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void download(std::vector<T>& h, size_t count, hipStream_t s) {
    h.resize(count);
    if (count) { HIPCHK(hipMemcpyAsync(h.data(), p, count * sizeof(T), hipMemcpyDeviceToHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
  }
};

static const bool g_trace = getenv("CHEM_TRACE") != nullptr;
static const bool g_dd_nopoll = getenv("CHEM_DD_NOPOLL") != nullptr;   // decomposed path: the host reads the decision with a blocking copy instead of polling
struct Trace {
  double t; const char* what;
  Trace(const char* w) : t(now_s()), what(w) {}
  void lap(const char* tag) { if (g_trace) { double n = now_s(); fprintf(stderr, "[chem trace] %s/%s %.3f ms\n", what, tag, 1e3 * (n - t)); t = n; } }
};

static inline int cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

// ---------------------------------------------------------------------------------------
struct Ctx {
  std::string err;
  int device = 0, prec = 32;
  double L[3] = {0, 0, 0}, rc = 0, skin = 0, dt = 0, cap_force = 0;
  int resc_kind = 0; double resc_kT = 0, resc_param = 0;   // Berendsen (1) / Isokinetic (2) velocity rescaling, StochasticVelocityRescaling (3)
  uint64_t svr_seed = 0;
  // Berendsen barostat (chem_barostat_berendsen; chem_baro_host.hpp): on while baro_tau > 0.  baro_keep: the forces in f4 are
  // those evaluated before the last scaling of a finished run, in the particle order of that evaluation -- the next chem_run
  // starts from them (what a longer run would have done) unless something re-sorted the particles or touched the system since.
  double baro_p0 = 0, baro_tau = 0; bool baro_keep = false;
  // what the scalings since the last list build (since the last rebuild of the reference rule) have been charged as displacement:
  // taken off the half skin every decision compares with (the same as adding it to the accumulated distance on the device)
  double baro_charge = 0, baro_charge_ref = 0; int baro_seen_builds = -1, baro_seen_ref = -1;
  double half_skin_eff() const { return std::max(0.5 * skin_eff() - baro_charge, 0.0); }
  double half_skin_ref() const { return std::max(0.5 * skin - baro_charge_ref, 0.0); }
  // Langevin piston (chem_barostat_langevin): on while pist_w > 0; never together with the Berendsen barostat.  pist_pe is the
  // host's copy of the piston momentum the device keeps (pist_pe_upload: the device's word has to be written first), pist_sv and
  // pist_mu the factors of the next step as the device computed them at the last kick.
  double pist_w = 0, pist_gamma = 0, pist_kT = 0; uint64_t pist_seed = 0;
  double pist_pe = 0, pist_eps = 0, pist_sv = 1, pist_mu = 1, baro_p_last = 0; bool pist_pe_upload = false, pist_mu_upload = false;
  bool piston_on() const { return pist_w > 0; }
  bool baro_on() const { return baro_tau > 0 || pist_w > 0; }
  const char* baro_name() const { return piston_on() ? "Langevin" : "Berendsen"; }
  void baro_forget() {      // a barostat goes off: nothing of it stays (lists that scalings have aged are built again first)
    if (baro_charge > 0 || baro_charge_ref > 0) resort = true;
    baro_keep = false; baro_charge = baro_charge_ref = 0; baro_seen_builds = baro_seen_ref = -1; baro_p_last = 0;
  }
  HostTopology top;
  std::vector<double> pos0, vel0;  // staged particle data (tag order) until first upload
  // Checkpoints (chem_checkpoint_save / chem_checkpoint_load; chem_ckpt_host.hpp).  img0: staged image counters of a restored
  // state -- while it is not empty, pos0 holds the device's own coordinates, which the upload takes as they are (no fold, no
  // count).  ckpt_pull: the device's particle data and chemical states into pos0 / vel0 / img0 and the mirrors; ckpt_reset: what
  // the typed context derives from the host data is forgotten.  Between them save and load put the same host data in place and
  // raise every dirty flag, so both contexts go on through one code path.
  std::vector<int32_t> img0;
  virtual void ckpt_pull() = 0;
  virtual void ckpt_reset() = 0;
  int64_t tm_base_rebuilds = 0, tm_base_list_rebuilds = 0;      // the device's counters start again with every upload of the particles
  int ntypes = 1;
  HostPairPot pp[CHEM_MAX_TYPES][CHEM_MAX_TYPES];
  // Truncated Coulomb term (chem_nb_coulomb): one (prefactor, rc) for every registered type pair, a symmetric type-pair bit mask
  double coul_k = 0, coul_rc = 0; uint32_t coul_mask[CHEM_MAX_TYPES] = {}; bool coul_dirty = false;
  bool coul_on() const { for (uint32_t m : coul_mask) if (m) return true; return false; }
  // the by-tag charge array is alive: a non-bonded Coulomb pair is registered or a 1-4 Coulomb list (CHEM_POT_COULOMB_BOND) exists.
  // Asked wherever charges are kept current; the pair kernel's mode, LDS plan and option limits follow coul_on() alone.
  bool charges_on() const { return coul_on() || top.any_coulomb_bond(); }
  double coul_epot = 0, coul_virial = 0;   // of the last energy evaluation (observe)
  // Per-particle resolution lambda (chem_nb_resolution, chem_resolution_rate, chem_set_resolution; chem_res_host.hpp): the
  // stamps by tag and the rates by type live on the host (`res`), marked type pairs in a symmetric bit mask with their caps.
  // The device copies (stamps, rates, mask, caps) exist only while a type pair is marked (res_pairs_on): lambda moves no force
  // otherwise.  res_rules: public reaction index -> lambda set on the role-1 / role-2 particle of every event (< 0: none).
  ResState res; uint32_t res_mask[CHEM_MAX_TYPES] = {}; double res_fmax[CHEM_MAX_TYPES][CHEM_MAX_TYPES] = {}; bool res_dirty = false;
  std::map<int, std::array<double, 2>> res_rules;
  bool res_pairs_on() const { for (uint32_t m : res_mask) if (m) return true; return false; }
  // Capped pairs (chem_nb_cap): the cap radius of every capped type pair, symmetric, 0 = none.  The device copy (the squares, in
  // the kernels' precision) exists only while a type pair is capped (caps_on); the capped force kernels are launched only then.
  double cap_rad[CHEM_MAX_TYPES][CHEM_MAX_TYPES] = {}; bool cap_dirty = false;
  bool caps_on() const { for (const auto& row : cap_rad) for (double c : row) if (c > 0) return true; return false; }
  // the force kernel stages one extra word per slot (charge or lambda): LDS plan, kernel choice and option limits follow it
  bool slot_word_on() const { return coul_on() || res_pairs_on(); }
  // type changes have to be seen when they happen (re-stamping) and events looked at (res_rules)
  bool res_tracking() const { return (res.on() && res.any_rate()) || !res_rules.empty(); }
  virtual void res_push(const std::vector<int32_t>& tags) = 0;      // stamps of these tags -> device (if the copy is alive)
  // Fixed distances (chem_fix_create ff.; chem_fix_host.hpp): sets, entries, release rules and the log live on the host; the
  // device holds the flat entry array only while a live entry exists (fix_dirty: rewritten at the next flush_host_state).
  FixState fix; bool fix_dirty = false;
  bool ran = false;      // chem_run has been called since chem_set_particles (chem_add_particles is refused then)
  // releases have to be looked for at every reaction / ATRP step: a rule, or a typed set, with entries to act on
  bool fix_tracking() const {
    if (!fix.any()) return false;
    if (!fix.rules.empty()) return true;
    for (const FixSet& s : fix.sets) if (!s.ent.empty() && (s.anchor_type >= 0 || s.target_type >= 0)) return true;
    return false;
  }
  virtual int fix_after_reactions(bool events) = 0;       // release by reaction (this step's events) and by type; the number released
  virtual void add_particles_prepare() = 0;                // positions and velocities back into pos0 / vel0 (tag order)
  bool lang = false; double kT = 0, gamma = 0; uint64_t lang_seed = 0; uint32_t lang_tmask = 0;
  bool react_init = false, react_on = false;
  int interval = 0, nearest = 1, max_per_interval = 0; uint64_t react_seed = 0;
  std::vector<chem_reaction_desc> reactions;
  // Dissociation reactions (chem_dissociation_add) live beside the association table -- they occupy no row of ReactSet or of
  // the role words -- but share its public index space: pub_map[public] = row of `reactions` (>= 0) or ~row of `dissociations`.
  std::vector<chem_dissociation_desc> dissociations;
  std::vector<int> pub_map, assoc_pub, diss_pub;
  int assoc_row(int pub) const { return pub >= 0 && pub < (int)pub_map.size() && pub_map[pub] >= 0 ? pub_map[pub] : -1; }
  int public_index(int arena_r) const { return arena_r >= 0 ? assoc_pub[arena_r] : diss_pub[~arena_r]; }
  std::vector<chem_nb_change> nb_rules;   // PostProcessChangeNeighboursProperty (chem_reaction_neighbour_change)
  // Reverse reactions: PostProcessRemoveNeighbourBond (chem_reaction_remove_bond; rules keyed by the row of `reactions`, the log
  // by tags and the public index) and PostProcessJoinParticles (chem_reaction_join: fix.joins).  Both act in reverse_step().
  std::vector<NbRemoveRule> rm_rules;
  struct RemovedRec { int64_t step; int32_t near, far, list, reaction; };
  std::vector<RemovedRec> removed_log;
  bool reverse_on() const { return !rm_rules.empty() || !fix.joins.empty(); }
  // RestrictReaction.define_connection (chem_reaction_restrict): (tag lo, tag hi) -> reaction bits; CSR rebuilt when it changed
  std::map<std::pair<int32_t, int32_t>, uint32_t> restrict_map; uint32_t restricted_mask = 0; bool restrict_dirty = false;
  std::vector<NbCons> constraints;   // ReactionConstraintNeighbourState (chem_reaction_constraint)
  // integrator.ATRPActivator (chem_atrp_init; reaction_post_process.py:380-426)
  bool atrp_on = false; chem_atrp_desc atrp{}; std::vector<AtrpCenter> atrp_centers; std::vector<chem_atrp_stats> atrp_stats;
  // Region rules (chem_region_add; chem_region_host.hpp): descriptors and switches live on the host and travel to the scan
  // kernel by value; the logs hold tags.  region_keep: a rule changed something at the step the last run ended on -- the stored
  // forces (resets included) are the ones the next run starts from, and the list build it asked for comes behind the next drift,
  // as in an uninterrupted run -- unless something has touched the system or re-sorted the particles since.
  std::vector<chem_region_desc> regions; std::vector<uint8_t> region_enabled;
  std::vector<RegionChange> region_log; std::vector<RegionStat> region_stats;
  int64_t region_firings = 0, region_syncs = 0, region_counted = 0; bool region_keep = false;
  bool region_any() const { for (uint8_t e : region_enabled) if (e) return true; return false; }
  bool region_due_at(int64_t s) const { for (size_t k = 0; k < regions.size(); ++k) if (region_due(regions[k], region_enabled[k] != 0, s)) return true; return false; }
  std::vector<chem_event> events;   // expanded, canonical order (filled lazily from the arena by chem_get_events)
  // event arena: SoA copy of the device records of every reaction step, appended in device order (amortised growth:
  // fresh vectors per step cost their page faults every time -- 4 ms for 2.8e5 events); blocks = (step, first index).
  // The host's type/mass/charge mirrors are brought up to date from it lazily (sync_type_mirrors): chemical states and
  // types live on the device, the mirrors are only read by typed lists, tuple spawning and read-back paths.
  struct EventArena {
    std::vector<int32_t> a, b, r; std::vector<double> d2; std::vector<int8_t> intra;
    std::vector<std::pair<int64_t, size_t>> blocks; size_t mirror_pos = 0, expanded_blocks = 0;
    size_t size() const { return a.size(); }
    void clear() { a.clear(); b.clear(); r.clear(); d2.clear(); intra.clear(); blocks.clear(); mirror_pos = 0; expanded_blocks = 0; }
  } arena;
  int opt_intra_inter = 0;   // classify every event as intra-/inter-cluster at event time (ar.save_intra_inter_counter)
  // records of one reaction step (device order) -> arena; runs on the bookkeeping thread beside the MD steps unless the
  // host needs the type mirrors within the reaction step itself
  template <class Rec> void append_events(const Rec* ev, size_t m, int64_t at_step, const std::vector<int8_t>& intra_flags) {
    EventArena& A = arena;
    const size_t n0 = A.size();
    A.blocks.emplace_back(at_step, n0);
    A.a.resize(n0 + m); A.b.resize(n0 + m); A.r.resize(n0 + m); A.d2.resize(n0 + m);
    if (!intra_flags.empty()) { A.intra.resize(n0 + m); std::copy(intra_flags.begin(), intra_flags.end(), A.intra.begin() + n0); }
    for (size_t k = 0; k < m; ++k) { A.a[n0 + k] = ev[k].a; A.b[n0 + k] = ev[k].b; A.r[n0 + k] = ev[k].r; A.d2[n0 + k] = ev[k].d2; }
  }
  void sync_type_mirrors() {
    for (size_t k = arena.mirror_pos; k < arena.size(); ++k) {
      if (arena.r[k] < 0) continue;      // (a dissociation event: diss_step brought the mirrors up to date itself)
      const chem_reaction_desc& d = reactions[arena.r[k]];
      const int32_t ea = arena.a[k], eb = arena.b[k];
      // (the charge follows the device's rule, k_react_apply_q: set wherever the reaction names a new type, also where the type stays)
      if (d.new_type_1 >= 0) { if (d.new_type_1 != top.type[ea]) { top.type[ea] = d.new_type_1; top.mass[ea] = d.new_mass_1; top.q[ea] = d.new_q_1; } else top.q[ea] = d.new_q_1; }
      if (d.new_type_2 >= 0) { if (d.new_type_2 != top.type[eb]) { top.type[eb] = d.new_type_2; top.mass[eb] = d.new_mass_2; top.q[eb] = d.new_q_2; } else top.q[eb] = d.new_q_2; }
    }
    arena.mirror_pos = arena.size();
  }
  int64_t step = 0;
  bool resort = true;
  bool geom_dirty = true, particles_dirty = true, pair_dirty = true, bonded_dirty = true, excl_dirty = true, labels_dirty = true;
  int nl_capacity_user = 0;
  int opt_tpp = 0;          // 0 = automatic
  int opt_time_pair = 0;    // HIP-event timing of every N-th pair-force launch (0 = off)
  int64_t pair_launch_no = 0;
  int opt_fuse = 1;         // fused integrate2+integrate1
  int opt_lpt = 1;          // descriptors of the fused rebuild in largest-tile-first order per XCD range (force launch tail)
  bool opt_dd_fold = true;   // decomposed path: block maxima folded by atomics of the integrate kernel (no fold launch per step)
  int opt_dd_merge = 1;     // decomposed path: displacement fold in the integrate kernel, decision in the force kernel (no one-block launches)
  bool opt_dd_fastx = true;  // decomposed path: excluded partners located as slots by the standalone list kernel (ghost copies through gtag)
  int opt_ablate_list = 0;  // diagnostics (with debug_stamps): parts of the list build left out, see tools/rebuild_stamps.py
                            // (1 tables + staging only, 3 no peel, 5 exclusions ignored, 4 home particles behind the first pass of 512 skipped: the lists are incomplete)
  int opt_bond_slots_kernel = 0; // bond pass, single domain: 0 the fused rebuild's idle tail records the bonded partners' slots, 1 k_bond_slots behind every neighbour launch
  int opt_coop_overflow = 1; // list build: the home particles behind a tile's last full pass of 512 are swept by nine lanes each (dev_nlist_tile_f32)
  int opt_row_order = 1;    // fused rebuild: a tile's force-list rows stored by length, the shortest in the last pass (chem_roworder_host.hpp); 0 = natural order
  int opt_tiles = 1;        // LDS-tiled list/force kernels when the cell grid allows
  int opt_fused = 1;        // rebuild chain as one persistent launch with grid barriers (single domain, tiles)
  int pair_guard = 0;       // 256 while the force kernels are launched speculatively (decomposed path)
  int pair_subset = 0;      // 0 all tiles, 1 interior tiles of the slab, 2 its two boundary tile layers
  int opt_overlap = -1;     // decomposed path: interior forces while the halo exchange is in flight (-1: automatic, by slab size)
  hipStream_t cstream = nullptr; hipEvent_t ev_fold = nullptr, ev_halo = nullptr;
  int opt_criterion = 0;     // 1: rebuild when max |x - x(last build)| > skin/2 ; 0: reference's accumulated per-step maxima
  // Internal list skin (>= the workload's skin): cells, tiles and the 16-bit force list are built for rc + skin_list and live
  // until the accumulated displacement exceeds skin_list / 2.  Forces do not depend on it (exact cutoff in the force kernel);
  // the reported rebuild count stays the reference rule's (DevCtl::ref_rebuilds).  opt_list_skin: < 0 automatic, 0 off
  // (= the workload's skin), > 0 explicit.  Only the fused single-domain tile path uses it.
  double opt_list_skin = -1.0, skin_list = 0.0;
  double skin_eff() const { return skin_list > skin ? skin_list : skin; }
  int opt_ablate = 0;        // diagnostic only: 1 = pair kernel stops after staging, 2 = skips staging
  int opt_skip_inactive = 1; // force list omits type pairs without a potential
  int opt_bonds_inline = 1;  // harmonic 2-body bonds evaluated by the force kernel from its staged image (when the host can prove it applicable)
  int opt_tile_split = 0;    // narrow tiles at the end of every tile row (chem_geom_host.hpp plan_tiles): 0 off, nb * 10 + w
  int opt_bucket_cap = 0;    // testing: bucket rows of the fused rebuild narrower than 64 (provokes the mid-run overflow recovery)
  int64_t halts_recovered = 0;
  // Neighbour launch only on steps that can need a rebuild (single domain, fused rebuild, accumulated criterion; DESIGN.md
  // section 5, chem_idle_host.hpp).  skip_idle: 0 a launch on every step, 1 the rule, 2 testing -- no launch the host did not
  // ask for itself, so that every regular rebuild stops the run and is redone.  idle_lag: the host enqueues step s once the
  // device has published step s - lag (bounded look-ahead); idle_kappa: allowance on the published per-step displacement.
  // (defaults from the sweep of profiles/skip_idle.txt)
  int opt_skip_idle = 1, opt_idle_lag = 1; double opt_idle_kappa = 1.25;
  int64_t idle_skipped = 0, idle_wrong = 0, idle_timeouts = 0;
  // which steps of the running call went without the launch, from step skip_log_base on: a stop takes the steps enqueued behind
  // it (they left at once and are redone) out of idle_skipped again; cleared wherever the host has seen the device without a stop
  std::vector<bool> skip_log; int64_t skip_log_base = 0;
  void skip_log_add(bool skipped) {
    const int64_t at = step - skip_log_base;
    if (at < 0) { skip_log.clear(); skip_log_base = step; }
    else skip_log.resize((size_t)at, false);
    skip_log.push_back(skipped);
    if (skipped) ++idle_skipped;
  }
  void skip_log_stop(int64_t halt_step) {      // the run stopped at halt_step: nothing from there on was a step
    const int64_t at = std::max<int64_t>(halt_step - skip_log_base, 0);
    for (size_t k = (size_t)at; k < skip_log.size(); ++k) if (skip_log[k]) --idle_skipped;
    if ((size_t)at < skip_log.size()) skip_log.resize((size_t)at);
  }
  void skip_log_confirm() { skip_log.clear(); skip_log_base = step; }
  // slab domain decomposition (chem_comm_init)
  bool dd_on = false; int P = 1, rk = 0;
  std::unique_ptr<Transport> tr;
  chem_timers tm{};
  virtual ~Ctx() {}
  virtual void run(int64_t nsteps) = 0;
  virtual int64_t get_state(int what, void* out, int64_t cap) = 0;
  virtual void observe(chem_obs* out) = 0;
  virtual void pressure(chem_pressure* out) = 0;
  virtual void pressure_tensor(chem_pressure_tensor* out) = 0;
  // Radial distribution functions (chem_rdf_*; rule set: include/chem_mi355.h, host rules: chem_rdf_host.hpp).  The configuration
  // lives here, the accumulators on the device (allocated by rdf_configure only); neither is part of a checkpoint.  every > 0:
  // chem_run takes a frame behind the force launch of every step s with s % every == 0.
  struct RdfConf { bool on = false; double r_max = 0; int nbins = 0, npairs = 0, split = 0, every = 0; int32_t tp[2 * CHEM_RDF_MAX_PAIRS] = {}; } rdf;
  virtual void rdf_configure() = 0;      // accumulators for rdf (zeroed), or freed where it is off
  virtual void rdf_sample() = 0;
  virtual void rdf_get(chem_rdf_result* out, uint64_t* counts, int64_t cap) = 0;
  virtual void rdf_reset() = 0;
  // Static structure factor (chem_sq_*; rule set: include/chem_mi355.h, host rules: chem_sq_host.hpp): as above, configuration here,
  // accumulators and scratch on the device (allocated by sq_configure and the first plan only), neither in a checkpoint.
  struct SqConf { bool on = false; int nmax = 0, npairs = 0, every = 0; int32_t tp[2 * CHEM_SQ_MAX_PAIRS] = {}; } sq;
  virtual void sq_configure() = 0;
  virtual void sq_sample() = 0;
  virtual void sq_get(chem_sq_result* out, double* sums, int64_t cap) = 0;
  virtual void sq_reset() = 0;
  virtual double sq_time_frames(int frames) = 0;      // chem_debug_sq_frame_ms
  virtual int64_t verlet_pairs(int64_t* out, int64_t cap) = 0;
  virtual void modify_particle(int tag, int what, double value) = 0;
  virtual int res_apply_completions() = 0;
  virtual void sync() = 0;
  virtual void refresh_timers() {}
  virtual void set_pair_bs(int) {}
  virtual void set_bond_pass(bool) {}
  virtual int64_t debug_dump(long long*, int64_t) { return 0; }
  virtual void debug_enable(int) {}
  virtual int64_t debug_dump_rebuild(long long*, int64_t) { return 0; }
  virtual int64_t debug_force_list(int, int32_t*, int64_t) { return -1; }
  virtual int64_t debug_row_order(int, int32_t*, int64_t) { return -1; }
  virtual void debug_tiles(int32_t* out) = 0;
  virtual void debug_acc(double* out) = 0;
  virtual void join_async() {}
};

// ---- from a plan of chem_launch_host.hpp to an instantiation ---------------------------------------------------------------
template <int V> using Int = std::integral_constant<int, V>;
// a run-time value as a compile-time one: f(Int<V>) for the V among Vs that v equals; false where none does (or f says so)
template <int... Vs, class F> bool pick_among(int v, F&& f) { return ((v == Vs && f(Int<Vs>{})) || ...); }

// f(kernel, Int<MODE>) for the tile kernel of a variant.  What this can name is the header's built set (and what the header
// lists as carried along is instantiated), so set_tile_lds_attr has prepared whatever launch_pair can launch.
template <typename R, class F> void with_tile_kernel(const PairVariant& v, F&& f) {
  const bool found = variant_built(v) && pick_among<0, 1>(v.energy, [&](auto E_) {
    constexpr bool E = decltype(E_)::value != 0;
    switch (v.mode) {
      case 4: f(&k_pair_tiles_q<R, E>, Int<4>{}); return true;
      case 5: f(&k_pair_tiles_res<R, E>, Int<5>{}); return true;
      case 6: f(&k_pair_tiles_cap<R, E>, Int<6>{}); return true;
      case 7: f(&k_pair_tiles_rescap<R, E>, Int<7>{}); return true;
    }
    return pick_among<0, 1, 2, 3>(v.mode, [&](auto M_) { return pick_among<1, 2, 4, 8>(v.tpp, [&](auto T_) {
      return pick_among<256, 512, 1024>(v.block, [&](auto B_) { return pick_among<0, 1>(v.diag, [&](auto D_) {
        constexpr int M = decltype(M_)::value, T = decltype(T_)::value, B = decltype(B_)::value;
        constexpr bool D = decltype(D_)::value != 0;
        if constexpr (tile_variant_built(M, T, B, E, D)) { f(&k_pair_tiles<R, T, E, B, M, D>, M_); return true; }
        else { if constexpr (tile_variant_unlaunched(M, T, B, E, D)) (void)&k_pair_tiles<R, T, E, B, M, D>; return false; }
      }); });
    }); });
  });
  if (!found) throw ChemError(CHEM_ESTATE, "internal: no pair-force kernel is built for the planned variant");
}
// ... and for the row kernel of a variant
template <typename R, class F> void with_row_kernel(const PairVariant& v, F&& f) {
  const bool found = variant_built(v) && pick_among<0, 1>(v.energy, [&](auto E_) {
    constexpr bool E = decltype(E_)::value != 0;
    switch (v.mode) {
      case 4: f(&k_pair_force<R, 4, E, true, true>, Int<4>{}); return true;
      case 5: f(&k_pair_force_res<R, 4, E>, Int<5>{}); return true;
      case 6: f(&k_pair_force_cap<R, 4, E>, Int<6>{}); return true;
      case 7: f(&k_pair_force_rescap<R, 4, E>, Int<7>{}); return true;
    }
    return pick_among<1, 2, 4, 8, 16, 32, 64>(v.tpp, [&](auto T_) { return pick_among<0, 1>(v.cubic, [&](auto C_) {
      f(&k_pair_force<R, decltype(T_)::value, E, decltype(C_)::value != 0>, Int<0>{}); return true;
    }); });
  });
  if (!found) throw ChemError(CHEM_ESTATE, "internal: no pair-force kernel is built for the planned variant");
}

template <typename R> struct CtxT : Ctx {
  using V4 = Vec4<R>;
  int pair_bs = 512;
  bool lj_only = true;
  bool cubic_tab = false;   // a type pair of kind 3 exists: the general-mode force kernels are launched in their CUBIC instantiation
  bool state_mirror_stale = false;   // top.state lags the device after reaction steps
  int tile_cap = 0;       // LDS slots of one staged tile (dynamic LDS)
  static size_t tile_lds_bytes(int cap_) { return (size_t)(cap_ + 5) * sizeof(V4) + 16; }
  size_t tile_lds_bytes() const { return tile_lds_bytes(tile_cap); }
  // force kernel: fp64 stages 24-byte slots + type bytes (two workgroups per CU instead of one)
  // (with a Coulomb pair registered: + one charge word per slot behind the image, k_pair_tiles MODE 4)
  static size_t pair_lds_bytes(int cap_, bool coul = false) { return coul ? coul_img_bytes<R>(cap_) : (sizeof(R) == 8 ? (size_t)(cap_ + 5) * 25 + 64 : tile_lds_bytes(cap_)); }
  size_t pair_lds_bytes() const { return pair_lds_bytes(tile_cap, slot_word_on()); }
  // the list build has its own layout of the same block (fp32: SoA groups + type masks + slice boundaries)
  // (fp64 builds use the fp32 list image too -- the force list may be a superset -- and need their own 32-byte-per-slot
  //  image only where the exact int32 rows are built)
  static constexpr size_t kTileLdsBudget = 150 * 1024;   // of 160 KB per CU: the rest is the kernels' static __shared__ (tile tables, scan scratch)
  // reaction scan: the staged image + 4 bytes per slot of role words (k_react_roles)
  size_t scan_lds_bytes() const { return scan_roles_offset(tile_cap, sizeof(V4)) + (size_t)(tile_cap + 1) * sizeof(unsigned int); }
  bool scan_roles_staged() const { return scan_lds_bytes() <= kTileLdsBudget; }      // (otherwise the scan reads the role words from global memory)
  // what a tile of cap_ slots asks of the LDS, over every kernel that stages one (asked before tile_cap is set or grown)
  // (extra: static LDS a force-kernel mode adds beyond what kTileLdsBudget leaves room for -- the staged force caps of MODE 5,
  //  the staged cap radii of MODE 6, both in MODE 7)
  static size_t tile_lds_need(int cap_, bool coul, size_t extra = 0) { return std::max(std::max(tile_lds_bytes(cap_), pair_lds_bytes(cap_, coul) + extra), list_lds_need(cap_, true)); }
  size_t res_lds_extra() const { return ((res_pairs_on() ? 1 : 0) + (caps_on() ? 1 : 0)) * sizeof(R) * kMaxTypes * kMaxTypes; }
  static size_t list_lds_need(int cap_, bool exact_rows) {
    const size_t lb = list_lds_bytes(cap_, kMaxTypes);
    return (sizeof(R) == 4 || exact_rows) ? std::max(tile_lds_bytes(cap_), lb) : lb;
  }
  size_t list_lds_need(bool exact_rows = true) const { return list_lds_need(tile_cap, exact_rows); }
  // ---- position codec on the host (md_kernels.hpp "position codec"): fp32 build = int32 fixed point, fp64 build = reals
  static constexpr bool kFixed = sizeof(R) == 4;
  double q_scale(int d) const { return L[d] / 2147483648.0; }
  R enc_pos(double x, int d) const {      // x already folded into [0, L)
    if constexpr (kFixed) { const int32_t q = (int32_t)(long long)std::llrint((x - 0.5 * L[d]) / q_scale(d)); R r; std::memcpy(&r, &q, 4); return r; }
    else return (R)x;
  }
  double dec_pos(R v, int d) const {
    if constexpr (kFixed) { int32_t q; std::memcpy(&q, &v, 4); return (double)q * q_scale(d) + 0.5 * L[d]; }
    else return (double)v;
  }
  R enc_shift(double boxes, int d) const {   // periodic shift of +-1 box length (slab ghost layers)
    if constexpr (kFixed) { const uint32_t q = boxes != 0.0 ? 0x80000000u : 0u; R r; std::memcpy(&r, &q, 4); return r; }
    else return (R)(boxes * L[d]);
  }
  static double fold_coord(double x, double Ld) { double s = std::floor(x / Ld); x -= s * Ld; if (x >= Ld) x -= Ld; if (x < 0) x = 0; return x; }
  PosScale<R> pos_scale() const {
    PosScale<R> ps{};
    for (int d = 0; d < 3; ++d) { ps.s[d] = (R)q_scale(d); ps.inv[d] = (R)(1.0 / q_scale(d)); }
    return ps;
  }
  hipStream_t stream = nullptr;
  int n = 0;
  DBuf<V4> x4, v4, f4, x4o, v4o, tab, x0;
  DBuf<int> tag, tago, rtag, state, res_id, mol_id;
  DBuf<int4> img4, img4o;
  DBuf<int> cell_cnt, cell_start, cell_of, slot_of, perm, cell_sub;
  // fused rebuild (single domain, tiles): segment scans + grid barrier state
  DBuf<int> cell_loc, seg_tot, tile_n, tile_loc, tseg_tot, cell_n, bucket; int bcap = 0; DBuf<GridBar> gbar;
  DBuf<int> tile_cnt, tile_off;   // reaction scan on tiles: candidates per tile, their offsets
  DBuf<int> tile_need;            // ... and the candidates every tile found, whether its region held them or not
  DBuf<unsigned int> scan_role;   // ... and the role bits of every particle slot (k_react_roles)
  DBuf<int4> bwork, bj; int nb_owner = 0; bool bwork_dirty = true;   // bonded work list (see dev_bonded_prep)
  // Inline bonds: all bonded terms are 2-body bonds of ONE harmonic parameter set and the exclusion set is exactly the bond
  // set (chain-growth systems) -> the LDS slots of the excluded partners, which the list build locates anyway, ARE the bonded
  // partners: it writes them out (BondRecs, md_kernels.hpp), the force kernel evaluates the bonds from its staged image, the per-step bonded
  // launch disappears.  Particles with more than kBondSlots (8) exclusions stay with the work list (then launched for them alone).
  // Decided on the host from what it knows exactly (bonds_inline()).
  DBuf<BondRec> brec0, brec1; bool harmonic_only = false, bonds_excluded = false;      // (one 8-byte word per particle each: partners 1-4, partners 5-8)
  BondRecs bond_recs(size_t np) {      // the two arrays, grown to np particles (every list build rewrites them)
    if (brec0.n < np) { brec0.alloc(np + 1024); brec1.alloc(np + 1024); }
    return BondRecs{brec0.p, brec1.p};
  }
  std::vector<uint8_t> excl_deg; size_t excl_deg_upto = 0; int64_t excl_over = 0;   // particles with more than kBondSlots (8) exclusions: their bonds stay with the work-list kernel
  void update_excl_deg() {
    if (excl_deg.size() != (size_t)top.n) { excl_deg.assign((size_t)top.n, 0); excl_deg_upto = 0; excl_over = 0; }
    if (excl_deg_upto > top.excl_log.size()) { std::fill(excl_deg.begin(), excl_deg.end(), 0); excl_deg_upto = 0; excl_over = 0; }
    for (; excl_deg_upto < top.excl_log.size(); ++excl_deg_upto) {
      const auto& e = top.excl_log[excl_deg_upto];
      for (int32_t t : {e.first, e.second}) { if (excl_deg[t] < 255) { ++excl_deg[t]; if (excl_deg[t] == kBondSlots + 1) ++excl_over; } }
    }
  }
  double inline_K = 0, inline_r0 = 0;
  // ... and where no particle has more than kBondSlots of them (single domain, fused rebuild), the list build does not look at
  // the exclusions at all: the rebuild's idle tail (slabs: k_bond_slots behind the list launch) records the partner slots, the force kernel takes the partners'
  // pair term out of its sums again (k_pair_tiles bond_mode 2).  Option bond_pass = 0: the list build removes the pairs itself.
  bool opt_bond_pass = true;
  void set_bond_pass(bool v) override { opt_bond_pass = v; }
  bool bond_by_pass() { return opt_bond_pass && ((use_fused && !dd_on) || (dd_on && use_tiles && opt_dd_fastx)) && bonds_inline() && excl_over == 0; }
  bool bonds_inline() {
    if (!opt_bonds_inline || !(use_fused || (dd_on && use_tiles)) || nbent <= 0 || !harmonic_only || !bonds_excluded) return false;
    if (coul_on()) return false;      // (the epilogue takes the partner's pair term out through pair_accum, which knows no charges)
    if (res_pairs_on()) return false;      // (nor any lambda)
    if (caps_on()) return false;      // (nor any cap radius)
    if (top.any_hybrid()) return false;      // (the force kernel knows one K, one r0 and no lambda: a hybrid list is never evaluated there)
    // (a 1-4 Coulomb list with parameters is a second slot, so harmonic_only already rules it out; one without parameters does
    //  nothing but would pass that proof -- inline bonds stay off next to any Coulomb term, so ask directly)
    if (top.any_coulomb_bond()) return false;
    if (!bond_records_fit(tile_cap)) return false;      // (a slot of the staged tile must fit the record's 16 bits)
    // the exclusion set must BE the bond set (bonds are a subset: bonds_excluded; both are duplicate-free): equal counts
    size_t nb2 = 0;
    for (const auto& l : top.lists) if (l.arity == 2) nb2 += (size_t)l.size();
    if (nb2 != top.excl_log.size()) return false;
    update_excl_deg();
    return true;
  }
  int fused_grid = 0, fused_grid_diag = 0, fused_par = 0, seg_shift = 0, tseg_shift = 0; bool use_fused = false;
  DBuf<int> nlist, nn, nnh;
  DBuf<unsigned short> nl16;
  // row order (option row_order): the staging regions of the fused rebuild's workgroups.  (Which home a stored row belongs to
  // is written into nnh by every list build, so the option may change between two builds.)
  DBuf<unsigned short> stage16; DBuf<int> stage_cnt; int stage_cap = 0;
  bool row_on() const { return row_order_on(opt_row_order, use_fused, use_tiles, dd_on, S); }
  void ensure_row_order() {
    if (!row_on()) return;
    stage_cap = row_stage_cap(n, box.ncell, HX * HY * HZ, tile_cap);
    stage16.alloc((size_t)fused_grid * stage_cap * S); stage_cnt.alloc((size_t)fused_grid * stage_cap);
  }
  DBuf<TileLDS<R>> tdesc;
  DBuf<long long> dbgbuf, wgst; bool dbg_on = false;
  Candidate* pin_ev = nullptr; size_t pin_ev_cap = 0;   // pinned host staging for reaction events
  // cluster labels of a reaction step are merged on a host thread beside the following MD steps;
  // joined (and uploaded) before the next reaction scan and before any other API call
  std::thread label_thr; bool labels_pending = false; std::exception_ptr label_err;
  std::vector<std::pair<int32_t, int32_t>> label_bonds; std::vector<int32_t> label_touched;
  std::vector<int> label_seen_lists;      // bonded list of every bond in label_bonds whose de-duplication key the thread still has to insert
  void join_async() override {
    join_thread();
    sync_type_mirrors();      // any API call other than chem_run sees current type/mass/charge mirrors
  }
  // the bookkeeping thread of the last reaction step (event log, bond graph, cluster labels, exclusion rows); the
  // reaction step itself joins only this -- replaying the type mirrors there would cost the 2-3 ms it just saved
  void join_thread() {
    if (label_thr.joinable()) label_thr.join();
    if (label_err) { std::exception_ptr e = label_err; label_err = nullptr; labels_pending = false; std::rethrow_exception(e); }
    if (labels_pending) {
      res_id.upload(top.res_id, stream); mol_id.upload(top.mol_id, stream);
      HIPCHK(hipStreamSynchronize(stream));
      labels_pending = false;
    }
  }
  // ---- slab decomposition state: reals live at [G, G+n), lower ghosts right-aligned in front of
  // them, upper ghosts behind; cap = allocated particles
  int nglob = 0, lower = 0, upper = 0, nzg = 0, z0 = 0, ncz = 0;
  int G = 0, nglo = 0, ngup = 0, cap = 0, mcap = 0;
  DBuf<unsigned char> mig[4];          // send down, send up, recv from upper, recv from lower
  DBuf<int> lcnt_dn, lcnt_up, gcnt_lo, gcnt_up;
  int halo_dn_off = 0, halo_dn_cnt = 0, halo_up_off = 0, halo_up_cnt = 0;   // slices of the own boundary layers
  DBuf<double> redbuf;                 // small device buffer for cross-rank reductions
  DBuf<Candidate> cand_loc; DBuf<int> cnt_all;   // reaction candidates before the all-gather
  int acap() const { return dd_on ? cap : n; }
  int64_t dd_rebuilds = 0, dd_direct_rebuilds = 0;   // slab rebuilds: all of them / those the host called for itself (rebuild_now)
  int* hflag = nullptr; int* hflag_dev = nullptr; int hticket = 0;   // pinned decision word + ticket
  DBuf<double> dd_vals;
  DBuf<unsigned long long> foldmax;    // decomposed path: atomic fold of the step's displacement maxima (kFoldSlots words, md_kernels.hpp)
  bool fold_on() const { return dd_merged() && opt_dd_fold; }
  // (allocated here if need be: the first drift of a context runs before its first dd_step_sync, and a launch without the words
  //  would leave that step's displacement out of the accumulated distance)
  // Single domain, fused rebuild, accumulated criterion: the same fold, two sets of words by the parity of the step's decision
  // (its launch -- k_rebuild_fused or the force kernel -- reads one and clears the other)
  // (skip_idle 0 is the launch on every step as it was: block maxima, no atomics, nothing published)
  bool fold_sd() const { return use_fused && !dd_on && opt_criterion == 0 && opt_skip_idle != 0; }
  unsigned long long* fold_arg() {
    if (fold_sd()) { ensure_hflag(); return foldmax.p + fused_par * kFoldSlots; }
    if (!(dd_on && fold_on())) return nullptr;
    ensure_hflag(); return foldmax.p;
  }
  // the published state of the device and the host's generation of it (chem_idle_host.hpp)
  int hint_gen = 1; int64_t hint_gen_step = 0;      // hint_gen_step: first step enqueued under this generation
  IdleHint* hint_host() { return reinterpret_cast<IdleHint*>(hflag + 64); }
  IdleHint* hint_dev() { return reinterpret_cast<IdleHint*>(hflag_dev + 64); }
  void hint_invalidate() { ++hint_gen; hint_gen_step = step; }
  IdleHint hint_read() {
    IdleHint h{}; h.step = -1;
    if (!hflag) return h;
    const volatile IdleHint* v = hint_host();
    const long long s1 = v->step;
    std::atomic_thread_fence(std::memory_order_acquire);
    h.acc = v->acc; h.d = v->d; h.gen = v->gen; h.halted = v->halted;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (v->step == s1) h.step = s1;
    return h;
  }
  bool skip_applies() const { return opt_skip_idle && fold_sd() && !want32 && !dbg_on && !baro_on(); }

  DBuf<int> gtag;                      // slab: index of a tag's ghost copy on this rank (-1: none)
  DBuf<Box<R>> box_dev; Box<R> box_dev_host; bool box_dev_valid = false;   // device copy of the box for the standalone list kernel
  int S = 0;
  bool use_tiles = false, want32 = false;   // int32 list only built on demand (reaction steps, diagnostics)
  ActMask act{}; UniLJ uni{}; bool uniform_lj = false; bool all_active = false;
  int ntiles = 0;
  DBuf<int> excl_start, excl_list; int has_excl = 0;
  DBuf<int> bstart; DBuf<BondedEntry> bent; DBuf<BondedParam> bpar; int64_t nbent = 0; bool bonds_only = false;
  // hybrid pair lists (chem_list_set_hybrid): (lambda0, rate) per parameter slot; has_hybrid selects the k_bonded*_hyb kernels.
  // has_coul14: a 1-4 Coulomb list exists -> the k_bonded*_q kernels (charges by tag, lambda code included)
  // force_step_off: 1 while the run loop evaluates the forces of the step it is about to complete (positions of step + 1)
  DBuf<double2> bhyb; bool has_hybrid = false, has_coul14 = false; int64_t force_step_off = 0;
  std::vector<std::array<double, 2>> stage_hyb;
  HybridArgs hybrid_args() const { return HybridArgs{bhyb.p, (long long)(step + force_step_off)}; }
  DBuf<PairCore<R>> pcore; DBuf<PairExt<R>> pext;
  DBuf<DevCtl> ctl;
  DBuf<unsigned long long> blockmax;
  int dd_par = 0; DecideArgs pair_da{};   // decomposed path: parity of the accumulated distance, decision arguments of the force launch
  DBuf<double> eout, ekout, elist;
  // reactions
  DBuf<Candidate> cand, evout; int cand_cap = 0;
  DBuf<int> st0, st1, asA, asB, evcount;
  DBuf<unsigned long long> best1, best2;
  DBuf<ReactSet> rs_dev;
  DBuf<int> conn_start, conn_partner; DBuf<unsigned int> conn_mask, cons_ok;
  Box<R> box{}; BoxD boxd{};
  bool device_ready = false;
  // per-kernel HIP-event samples of the timed region (option time_pair_kernel = N: every N-th step)
  std::vector<hipEvent_t> ev;  // pool, used in pairs
  size_t ev_used = 0;
  std::vector<int> ev_kind;    // kind of sample k (events 2k, 2k+1): 0 pair, 1 neighbour kernel, 2 integrate, 3 bonded
  bool timed_step = false;
  // A sampled step brackets the force kernel and ONE of the other per-step kernels (rotating) with events: the records between
  // the launches cost ~3 us each, and eight of them on every sampled step showed in short timed regions
  int timed_extra = 1;
  void tbeg(int kind) { if (timed_step && (kind == 0 || kind == timed_extra) && ev_used + 2 <= ev.size()) { HIPCHK(hipEventRecord(ev[ev_used], stream)); ev_kind.push_back(kind); } }
  void tend() { if (timed_step && ev_used + 2 <= ev.size() && ev_kind.size() == ev_used / 2 + 1) { HIPCHK(hipEventRecord(ev[ev_used + 1], stream)); ev_used += 2; } }

  CtxT() { HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); }
  ~CtxT() override {
    if (label_thr.joinable()) label_thr.join();
    if (stream) (void)hipStreamSynchronize(stream);   // nothing may still write the pinned words or the buffers
    tr.reset();
    for (auto e : ev) (void)hipEventDestroy(e);
    if (pin_ev) (void)hipHostFree(pin_ev);
    if (hflag) (void)hipHostFree(hflag);
    if (baro_pin) (void)hipHostFree(baro_pin);
    if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); (void)hipEventDestroy(ev_fold); (void)hipEventDestroy(ev_halo); }
    if (stream) (void)hipStreamDestroy(stream);
  }
  void sync() override { HIPCHK(hipStreamSynchronize(stream)); }

  // ---- uploads ------------------------------------------------------------------------
  void setup_box() {
    const CellGrid cg = cell_grid(L, rc + skin_eff());
    const int* nc = cg.nc; const bool cells = cg.cells;
    for (int d = 0; d < 3; ++d) {
      box.L[d] = (R)L[d]; box.invL[d] = (R)(1.0 / L[d]);
      box.nc[d] = nc[d];
      box.cell_inv[d] = (R)((cells ? nc[d] : 1) / L[d]);
      boxd.L[d] = L[d]; boxd.invL[d] = 1.0 / L[d];
      box.qs[d] = boxd.qs[d] = q_scale(d); box.qh[d] = boxd.qh[d] = 0.5 * L[d];
      box.qsf[d] = (R)q_scale(d); box.qinvf[d] = (R)(1.0 / q_scale(d));
    }
    box.ncell = cells ? nc[0] * nc[1] * nc[2] : 1;
    box.xs_nb = 1 << 20; box.xs_w = 1;      // (all tiles HX wide until the tile plan says otherwise)
    box.zghost = 0; box.z0g = 0; box.nzg = cells ? nc[2] : 1; box.shz_lo = 0; box.shz_hi = 0;
    if (dd_on) {
      const SlabLayers sl = slab_layers(cg, P, rk);
      nzg = sl.nzg; ncz = sl.ncz; z0 = sl.z0; lower = sl.lower; upper = sl.upper;
      box.zghost = 1; box.z0g = z0; box.nzg = nzg; box.nc[2] = ncz + 2;
      box.ncell = nc[0] * nc[1] * (ncz + 2);
      box.shz_lo = enc_shift(z0 == 0 ? -1.0 : 0.0, 2);
      box.shz_hi = enc_shift(z0 + ncz == nzg ? 1.0 : 0.0, 2);
    }
  }

  double pick_list_skin() const {
    return chem::pick_list_skin(L, rc, skin, opt_list_skin, opt_criterion, opt_tiles != 0, opt_fused != 0, dd_on, P, dd_on ? nglob : n);
  }
  void debug_acc(double* out) override { const DevCtl h = read_ctl(); out[0] = h.acc_ref; out[1] = h.acc_maxdist; }
  void debug_tiles(int32_t* out) override {
    if (geom_dirty) setup_geometry();
    const int ntx = use_tiles ? tile_ntx(box.nc[0], box.xs_nb, box.xs_w) : 0;
    out[0] = ntiles; out[1] = box.nc[0]; out[2] = use_tiles ? tile_nbx(box.nc[0], box.xs_nb) : 0; out[3] = box.xs_w;
    out[4] = ntx ? ntiles / ntx : 0; out[5] = tile_cap;
  }
  // cells, neighbour-list capacity and everything else that depends on box/cutoff/skin (the rules: chem_geom_host.hpp)
  void setup_geometry() {
    skin_list = pick_list_skin();
    setup_geometry_once();
    if (skin_list > 0 && !use_fused && !dd_on) { skin_list = 0.0; setup_geometry_once(); }   // the wider skin only pays on the fused tile path
    baro_replan_pending = false;
  }
  void setup_geometry_once() {
    setup_box();
    cell_cnt.alloc(box.ncell + 1); cell_start.alloc(box.ncell + 1); cell_sub.alloc(box.ncell + 2);
    HIPCHK(hipMemsetAsync(cell_cnt.p, 0, sizeof(int) * (box.ncell + 1), stream));
    S = row_stride(L, rc + skin_eff(), dd_on ? nglob : n, nl_capacity_user);
    const TilePlan tp = plan_tiles(box.nc[0], box.nc[1], dd_on ? ncz : box.nc[2], dd_on ? nzg : box.nc[2], dd_on ? nglob : n, dd_on, opt_tiles != 0,
                                   opt_tile_split, [coul = slot_word_on(), extra = res_lds_extra()](int c) { return tile_lds_need(c, coul, extra); }, kTileLdsBudget);
    use_tiles = tp.use_tiles; box.xs_nb = tp.xs_nb; box.xs_w = tp.xs_w; ntiles = tp.ntiles;
    if (tp.tile_cap) { tile_cap = tp.tile_cap; if (use_tiles) set_tile_lds_attr(); }      // (a grid without tiles leaves the last capacity as it was)
    alloc_lists();
    setup_fused();
    setup_tile_order();
    HIPCHK(hipStreamSynchronize(stream));
    geom_dirty = false; resort = true; hint_invalidate();
  }

  // Fused rebuild kernel: the grid must be co-resident (grid barriers), so it is sized from the
  // occupancy of the kernel itself on this device.
  void setup_fused() {
    use_fused = false;
    if (!opt_fused || !use_tiles || dd_on) return;
    const void* fn = reinterpret_cast<const void*>(&k_rebuild_fused<R, 512>);
    // (a block the device refuses leaves the fused launch off -- the unfused chain takes over -- instead of failing the set-up)
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)list_lds_need()) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rebuild_fused<R, 512, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)list_lds_need()) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 512, list_lds_need(false)) != hipSuccess || per_cu < 1) return;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    int g = std::min(per_cu * prop.multiProcessorCount, 1024) / 8 * 8;
    if (g < 8) return;
    fused_grid = g;
    // the diagnostic instantiation (stamps, int32 rows) has its own resource usage and, in fp64, the larger LDS block
    int per_cu_d = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, reinterpret_cast<const void*>(&k_rebuild_fused<R, 512, true>), 512, list_lds_need(true)) != hipSuccess || per_cu_d < 1) return;
    fused_grid_diag = std::min(std::min(per_cu_d * prop.multiProcessorCount, 1024) / 8 * 8, fused_grid);
    if (fused_grid_diag < 8) return;
    // cell segments: 64 cells (the prefix inside a segment is one wave reduction in the sort phase), more when that
    // would give more than 1024 segments; tile segments: <= 1024 of them
    seg_shift = segment_shift(box.ncell, 6, 1024); tseg_shift = segment_shift(ntiles, 0, 1024);
    cell_loc.alloc(box.ncell + 1); seg_tot.alloc(1024); tile_n.alloc(ntiles + 1); tile_loc.alloc(ntiles + 1); tseg_tot.alloc(1024);
    // bucket rows of the binning pass: 64 members per cell = what one wave sorts (the LDS tiles already require a mean
    // cell occupancy far below that); a fuller cell raises ctl->bucket_overflow and the unfused chain takes over
    cell_n.alloc(box.ncell + 1);
    bcap = opt_bucket_cap > 0 ? std::min(opt_bucket_cap, 64) : 64;
    bucket.alloc((size_t)box.ncell * bcap);
    HIPCHK(hipMemsetAsync(bucket.p, 0, sizeof(int) * (size_t)box.ncell * bcap, stream));   // (the sort phase reads whole rows: entries must always be valid indices)
    if (!gbar.p) { gbar.alloc(1); HIPCHK(hipMemsetAsync(gbar.p, 0, sizeof(GridBar), stream)); }
    HIPCHK(hipMemsetAsync(seg_tot.p, 0, sizeof(int) * 1024, stream));
    use_fused = true;
    ensure_row_order();
  }
  DBuf<int> tile_pos, tile_ord;
  void setup_tile_order() {
    TileOrder o = use_tiles && !dd_on ? tile_order(box.nc, box.xs_nb, box.xs_w, ntiles) : TileOrder{};
    if (o.ord.empty()) { tile_pos.free(); tile_ord.free(); return; }
    // (two copies each: the rebuild kernel double-buffers them by the parity of its rebuild count and rewrites them from the home counts)
    for (std::vector<int>* v : {&o.pos, &o.ord}) { v->resize(2 * (size_t)ntiles); std::copy_n(v->begin(), ntiles, v->begin() + ntiles); }
    tile_pos.upload(o.pos, stream); tile_ord.upload(o.ord, stream);
  }
  void launch_rebuild_fused(bool publish = false) {      // publish: a step's decision in run() -- tells the host where the device stands
    FusedArgs<R> a{};
    a.n = n; a.ncell = box.ncell; a.ntiles = ntiles; a.CAP = tile_cap; a.S = S; a.has_excl = has_excl; a.criterion = opt_criterion;
    a.par = fused_par; a.seg_shift = seg_shift; a.tseg_shift = tseg_shift; a.nblk = cdiv(n, kIntPerBlock); a.want32 = want32 ? 1 : 0; a.ntypes = ntypes; a.ablate = dbg_on ? opt_ablate_list : 0; a.coop = opt_coop_overflow;
    a.half_skin = half_skin_eff(); a.rl2 = (R)((rc + skin_eff()) * (rc + skin_eff()));
    a.half_skin_ref = half_skin_ref(); a.rl2_rows = (R)((rc + skin) * (rc + skin));
    a.istep = step;
    a.x4 = x4.p; a.v4 = v4.p; a.x4o = x4o.p; a.v4o = v4o.p; a.x0 = opt_criterion ? x0.p : nullptr;      // (reference positions: only the displacement criterion reads them -- 16 MB of writes per rebuild otherwise)
    a.tag = tag.p; a.tago = tago.p; a.rtag = rtag.p; a.img4 = img4.p; a.img4o = img4o.p;
    a.cell_cnt = cell_cnt.p; a.cell_of = cell_of.p; a.slot_of = slot_of.p; a.cell_start = cell_start.p; a.cell_loc = cell_loc.p;
    a.cell_sub = cell_sub.p; a.cell_n = cell_n.p; a.bucket = bucket.p; a.bcap = bcap; a.btot = seg_tot.p; a.perm = perm.p; a.tn = tile_n.p; a.tloc = tile_loc.p; a.tbtot = tseg_tot.p;
    a.tile_pos = opt_lpt ? tile_pos.p : nullptr; a.tile_ord = opt_lpt ? tile_ord.p : nullptr;
    a.desc = tdesc.p; a.excl_start = excl_start.p; a.excl_list = excl_list.p; a.nl16 = nl16.p; a.nnh = nnh.p; a.nlist = nlist.p; a.nn = nn.p;
    a.blockmax = blockmax.p; a.ctl = ctl.p; a.gb = gbar.p; a.box = box; a.act = act;
    if (row_on()) {
      ensure_row_order();
      a.stage16 = stage16.p; a.stage_cnt = stage_cnt.p; a.stage_cap = stage_cap;
      a.row_P = std::max(pair_bs / std::max(pick_tpp(), 1), 64);
    }
    a.wgst = dbg_on && wgst.p ? wgst.p : nullptr;
    a.bstart = bstart.p; a.bent = bent.p; a.bwork = bwork.p; a.bj = bj.p; a.nbent = (int)std::min<int64_t>(nbent, 1 << 30);
    a.fold = fold_sd() ? (ensure_hflag(), foldmax.p) : nullptr;
    a.hint = publish && fold_sd() ? hint_dev() : nullptr; a.gen = hint_gen;
    a.bslots = BondRecs{}; a.bond_pass = 0;
    if (bonds_inline() && !(sizeof(R) == 8 && want32)) {   // (the exact fp64 builder of the int32 rows locates no slots: ensure_list32 rebuilds again)
      a.bslots = bond_recs((size_t)n);
      a.bond_pass = (bond_by_pass() && !want32) ? (opt_bond_slots_kernel ? 2 : 1) : 0;    // (the int32 rows must leave the excluded pairs out: ensure_list32 rebuilds again behind them)
      if (excl_over == 0) a.nbent = 0;                      // no work list needed; otherwise it holds the owners with > kBondSlots exclusions only
    }
    if (dbg_on || want32) hipLaunchKernelGGL((k_rebuild_fused<R, 512, true>), dim3(fused_grid_diag), dim3(512), list_lds_need(true), stream, a);
    else hipLaunchKernelGGL((k_rebuild_fused<R, 512>), dim3(fused_grid), dim3(512), list_lds_need(false), stream, a);
    if (a.bond_pass == 2)      // (leaves at once unless the launch in front of it has rebuilt: DevCtl::need_rebuild)
      hipLaunchKernelGGL((k_bond_slots<R>), dim3(ntiles), dim3(256), 0, stream, ntiles, (const TileLDS<R>*)tdesc.p, (const int*)tag.p, (const int*)excl_start.p,
                         (const int*)excl_list.p, (const int*)rtag.p, (const int*)nullptr, 0, 0x7fffffff, (const V4*)x4.p, box, a.bslots, ctl.p);
    fused_par ^= 1;
  }

  void set_tile_lds_attr() {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nlist_tiles<R, 512>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)list_lds_need()));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_react_scan_tiles<R, 512>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(scan_roles_staged() ? scan_lds_bytes() : tile_lds_bytes())));
    // every force kernel a plan can name (chem_launch_host.hpp); MODE 4..7 while their feature is on: the image + the charge
    // words (4), + the lambda words (5, 7: same layout), the image alone (6)
    const bool on47[4] = {coul_on(), res_pairs_on(), caps_on() && !res_pairs_on(), caps_on() && res_pairs_on()};
    for_each_tile_variant([&](const PairVariant& v) {
      if (v.mode >= 4 && !on47[v.mode - 4]) return;
      const int bytes = (int)(v.mode >= 4 ? pair_lds_bytes() : tile_lds_bytes());
      with_tile_kernel<R>(v, [&](auto kern, auto) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes)); });
    });
  }

  void alloc_lists() {
    nlist.free(); nl16.free();
    const size_t ac = (size_t)acap();
    nlist.alloc(ac * S);
    nnh.alloc(ac);
    if (use_tiles) { nl16.alloc(ac * S); HIPCHK(hipMemsetAsync(nl16.p, 0, ac * S * 2, stream)); tdesc.alloc(ntiles); }
    // the energy launch of the tile path writes three words per TILE: a sparse box has more tiles than the particle count
    // behind upload_particles' size allows for (57 particles in 2197 tiles: observe() wrote past the end, tests/test_gpu_geometry.py)
    eout.alloc(3 * std::max((size_t)cdiv((long long)ac * 64, 256), (size_t)ntiles) + 8);
    tm.nlist_capacity = S;
    ensure_row_order();
  }

  void upload_particles() {
    nglob = (int)top.n;
    n = nglob; G = 0; nglo = ngup = 0; cap = nglob;
    std::vector<V4> hx, hv; std::vector<int> ht; std::vector<int4> hi;
    const bool raw = !img0.empty();      // a restored state: coordinates and image counters as the device held them
    if (dd_on) {
      if (raw) throw ChemError(CHEM_ENOTIMPL, "a context that holds a restored checkpoint cannot be decomposed: a gap of the decomposed path");
      skin_list = pick_list_skin();   // (the slab bounds below must be those of the geometry set up afterwards)
      setup_box();   // slab bounds (z0, ncz, nzg)
      const SlabCaps sc = slab_capacities(nglob, nzg, ncz);
      G = sc.G; mcap = sc.mcap; cap = sc.cap;
      hx.assign(cap, V4{}); hv.assign(cap, V4{}); ht.assign(cap, 0); hi.assign(cap, make_int4(0, 0, 0, 0));
      int k = G;
      for (int t = 0; t < nglob; ++t) {
        const SlabCoord zc = slab_layer_of(pos0[3 * t + 2], L[2], nzg);
        const double z = zc.z, s = zc.s;
        if (zc.layer < z0 || zc.layer >= z0 + ncz) continue;
        if (k >= cap - G) throw ChemError(CHEM_ENOSPC, "domain decomposition: slab holds more particles than the allocated capacity");
        // (x and y are folded by the first binning pass in the fp64 build; the fixed-point encoding wants them in the box now)
        const double fx_ = kFixed ? fold_coord(pos0[3 * t], L[0]) : pos0[3 * t], fy_ = kFixed ? fold_coord(pos0[3 * t + 1], L[1]) : pos0[3 * t + 1];
        hx[k].x = enc_pos(fx_, 0); hx[k].y = enc_pos(fy_, 1); hx[k].z = enc_pos(z, 2); hx[k].w = (R)top.type[t];
        if (kFixed) { hi[k].x = (int)std::llrint((pos0[3 * t] - fx_) / L[0]); hi[k].y = (int)std::llrint((pos0[3 * t + 1] - fy_) / L[1]); }
        hv[k].x = (R)vel0[3 * t]; hv[k].y = (R)vel0[3 * t + 1]; hv[k].z = (R)vel0[3 * t + 2]; hv[k].w = (R)top.mass[t];
        ht[k] = t; hi[k].z = (int)s;
        ++k;
      }
      n = k - G;
    } else {
      hx.resize(n); hv.resize(n); ht.resize(n); hi.assign(n, make_int4(0, 0, 0, 0));
      for (int t = 0; t < n; ++t) {
        if constexpr (kFixed) {   // folded on the host, images counted (the fp64 build leaves that to the first binning pass)
          for (int d = 0; d < 3; ++d) {
            const double x = pos0[3 * t + d], xf = raw ? x : fold_coord(x, L[d]);
            (&hx[t].x)[d] = enc_pos(xf, d); (&hi[t].x)[d] = raw ? img0[3 * t + d] : (int)std::llrint((x - xf) / L[d]);
          }
        } else {
          hx[t].x = (R)pos0[3 * t]; hx[t].y = (R)pos0[3 * t + 1]; hx[t].z = (R)pos0[3 * t + 2];
          if (raw) { hi[t].x = img0[3 * t]; hi[t].y = img0[3 * t + 1]; hi[t].z = img0[3 * t + 2]; }
        }
        hx[t].w = (R)top.type[t];
        hv[t].x = (R)vel0[3 * t]; hv[t].y = (R)vel0[3 * t + 1]; hv[t].z = (R)vel0[3 * t + 2]; hv[t].w = (R)top.mass[t];
        ht[t] = t;
      }
    }
    const int ac = acap();
    x4.upload(hx, stream); v4.upload(hv, stream); tag.upload(ht, stream); img4.upload(hi, stream);
    {
      std::vector<int> hr(nglob, -1);
      for (int k = 0; k < n; ++k) hr[ht[G + k]] = G + k;
      rtag.upload(hr, stream);
    }
    f4.alloc(ac); x4o.alloc(ac); v4o.alloc(ac); tago.alloc(ac); img4o.alloc(ac); x0.alloc(ac);
    HIPCHK(hipMemcpyAsync(x0.p, x4.p, sizeof(V4) * ac, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipMemsetAsync(f4.p, 0, sizeof(V4) * ac, stream));
    cell_of.alloc(ac); slot_of.alloc(ac); perm.alloc(ac); nn.alloc(ac);
    HIPCHK(hipMemsetAsync(nn.p, 0, sizeof(int) * ac, stream));
    ctl.alloc(1);
    HIPCHK(hipMemsetAsync(ctl.p, 0, sizeof(DevCtl), stream));
    blockmax.alloc(cdiv(ac, 256));
    HIPCHK(hipMemsetAsync(blockmax.p, 0, sizeof(unsigned long long) * cdiv(ac, 256), stream));
    eout.alloc(3 * (size_t)cdiv((long long)ac * 64, 256) + 8);
    ekout.alloc(4 * (size_t)cdiv(ac, 256) + 8);
    elist.alloc(CHEM_MAX_LISTS);
    redbuf.alloc(64);
    state.alloc(nglob); res_id.alloc(nglob); mol_id.alloc(nglob);
    if (dd_on) {
      const size_t mb = mig_bytes();
      for (int k = 0; k < 4; ++k) { mig[k].alloc(mb); HIPCHK(hipMemsetAsync(mig[k].p, 0, mb, stream)); }
    }
    HIPCHK(hipStreamSynchronize(stream));
    pos0.clear(); pos0.shrink_to_fit(); vel0.clear(); vel0.shrink_to_fit(); img0.clear(); img0.shrink_to_fit();
    particles_dirty = false; labels_dirty = true; geom_dirty = true; resort = true; device_ready = true;
  }

  // migration buffer layout: [count, pad x3][x4 x mcap][v4 x mcap][img4 x mcap][tag x mcap]
  size_t mig_bytes() const { return 16 + (size_t)mcap * (2 * sizeof(V4) + sizeof(int4) + sizeof(int)); }
  MigBuf<R> mig_view(int k) {
    unsigned char* b = mig[k].p;
    MigBuf<R> m;
    m.count = reinterpret_cast<int*>(b);
    m.x = reinterpret_cast<V4*>(b + 16);
    m.v = m.x + mcap;
    m.img = reinterpret_cast<int4*>(m.v + mcap);
    m.tag = reinterpret_cast<int*>(m.img + mcap);
    m.cap = mcap;
    return m;
  }

  // top.state lags the device after reaction steps: bring it up to date where the host is about to read it
  void refresh_state_mirror(bool force = false) {
    if (!force && !state_mirror_stale) return;
    std::vector<int> hs; state.download(hs, nglob, stream); top.state.assign(hs.begin(), hs.end()); state_mirror_stale = false;
  }

  void upload_labels() {
    refresh_state_mirror();
    state.upload(top.state, stream); res_id.upload(top.res_id, stream); mol_id.upload(top.mol_id, stream);
    HIPCHK(hipStreamSynchronize(stream));
    labels_dirty = false;
  }

  void upload_pair() {
    int nt = 1;
    for (int t : top.type) nt = std::max(nt, t + 1);
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = 0; b < CHEM_MAX_TYPES; ++b) if (pp[a][b].kind) nt = std::max(nt, std::max(a, b) + 1);
    for (auto& r : reactions) { nt = std::max(nt, std::max(r.new_type_1, r.new_type_2) + 1); }
    for (auto& r : dissociations) { nt = std::max(nt, std::max(r.new_type_1, r.new_type_2) + 1); }
    for (auto& r : nb_rules) nt = std::max(nt, r.new_type + 1);
    for (auto& c : atrp_centers) nt = std::max(nt, std::max(c.type, c.new_type) + 1);
    for (auto& r : regions) nt = std::max(nt, std::max(r.target_type, r.new_type) + 1);
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) if (coul_mask[a]) nt = std::max(nt, a + 1);
    for (const ResRate& r : res.rate) if (r.alpha > 0.0) nt = std::max(nt, r.new_type + 1);
    for (const FixSet& fs : fix.sets) for (const FixPost& fp : fs.post) nt = std::max(nt, fp.new_type + 1);
    ntypes = nt;
    std::vector<PairCore<R>> hc((size_t)nt * nt);
    std::vector<PairExt<R>> he((size_t)nt * nt);
    std::vector<V4> htab;
    bool cubic = false;
    for (int a = 0; a < nt; ++a) for (int b = 0; b < nt; ++b) {
      const HostPairPot& p = pp[a][b];
      PairCore<R> c{(R)-1, 0, 0, 0}; PairExt<R> e{0, 0, 0, 0, 0, 0, 0, 0};
      if (p.kind == 1) {
        const double s6 = std::pow(p.sig, 6), s12 = s6 * s6;
        c.rc2 = (R)(p.rc * p.rc); c.lj1 = (R)(48.0 * p.eps * s12); c.lj2 = (R)(24.0 * p.eps * s6); c.kind = (R)1;
        e.e1 = (R)(4.0 * p.eps * s12); e.e2 = (R)(4.0 * p.eps * s6); e.shift = (R)p.shift;
      } else if (p.kind == 2 && p.itype != TAB_LINEAR) {      // spline kinds: two rows of coefficients per interval
        c.rc2 = (R)(p.rc * p.rc); c.kind = (R)3; cubic = true;
        e.r0 = (R)p.r0; e.inv_dr = (R)(1.0 / p.dr); e.toff = (int)htab.size(); e.nrow = (int)p.e.size();
        const std::vector<double> co = pack_pair_rows(p.e.data(), p.f.data(), p.e.size(), p.itype);
        for (size_t k = 0; k < co.size(); k += 4) {
          V4 row; row.x = (R)co[k]; row.y = (R)co[k + 1]; row.z = (R)co[k + 2]; row.w = (R)co[k + 3];
          htab.push_back(row);
        }
      } else if (p.kind == 2) {
        c.rc2 = (R)(p.rc * p.rc); c.kind = (R)2;
        e.r0 = (R)p.r0; e.inv_dr = (R)(1.0 / p.dr); e.toff = (int)htab.size(); e.nrow = (int)p.e.size();
        for (size_t k = 0; k < p.e.size(); ++k) {
          const double fk = p.f[k], ek = p.e[k];
          const double fn = k + 1 < p.f.size() ? p.f[k + 1] : fk, en = k + 1 < p.e.size() ? p.e[k + 1] : ek;
          V4 row; row.x = (R)fk; row.y = (R)(fn - fk); row.z = (R)ek; row.w = (R)(en - ek);
          htab.push_back(row);
        }
      }
      hc[(size_t)a * nt + b] = c; he[(size_t)a * nt + b] = e;
    }
    lj_only = htab.empty();
    cubic_tab = cubic;
    // type pairs with a potential; uniform LJ = every active pair shares one parameter set
    std::memset(&act, 0, sizeof(act));
    uniform_lj = lj_only;
    const HostPairPot* first = nullptr;
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = 0; b < CHEM_MAX_TYPES; ++b) {
      const HostPairPot& p = pp[a][b];
      if (!opt_skip_inactive || p.kind || ((coul_mask[a] >> b) & 1u)) act.row[a] |= 1u << b;   // (a pair may carry the Coulomb term alone)
      if (p.kind == 1) {
        if (!first) first = &p;
        else if (p.eps != first->eps || p.sig != first->sig || p.rc != first->rc) uniform_lj = false;
      }
    }
    if (!opt_skip_inactive || !first) uniform_lj = false;
    if (slot_word_on() || caps_on()) { uniform_lj = false; lj_only = false; }
    // a re-sent potential keeps its cap: the radius must still lie inside the cutoff it has now
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = a; b < CHEM_MAX_TYPES; ++b)
      if (cap_rad[a][b] > 0 && pp[a][b].kind != 0 && !(cap_rad[a][b] < pp[a][b].rc))
        throw ChemError(CHEM_EINVAL, "capped type pair (" + std::to_string(a) + "," + std::to_string(b) + "): cap radius " + std::to_string(cap_rad[a][b]) +
                                     " is not inside the cutoff " + std::to_string(pp[a][b].rc) + " of the potential the pair carries now");
    all_active = true;   // every pair of types in use carries a potential: the list build skips the per-hit type filter
    for (int a = 0; a < nt; ++a) for (int b = 0; b < nt; ++b) if (!((act.row[a] >> b) & 1u)) all_active = false;
    if (uniform_lj) {
      const double s6 = std::pow(first->sig, 6), s12 = s6 * s6;
      uni.drc2 = first->rc * first->rc; uni.dlj1 = 48.0 * first->eps * s12; uni.dlj2 = 24.0 * first->eps * s6;
      uni.rc2 = (float)uni.drc2; uni.lj1 = (float)uni.dlj1; uni.lj2 = (float)uni.dlj2;
    }
    resort = true;   // the force list depends on the type-pair mask
    pcore.upload(hc, stream); pext.upload(he, stream); tab.upload(htab, stream);
    HIPCHK(hipStreamSynchronize(stream));
    pair_dirty = false;
  }

  // Charges by tag and the type-pair mask of the Coulomb term: allocated and kept up to date (k_react_apply, k_apply_props,
  // modify_particle) only while a Coulomb pair is registered or a 1-4 Coulomb list exists (charges_on); every rank of a
  // decomposition holds all of them.
  DBuf<R> qtag; DBuf<unsigned int> cmask_dev; DBuf<double> eoutq;
  R* qtag_arg() { return charges_on() ? qtag.p : nullptr; }
  void upload_coul() {
    coul_dirty = false;
    if (!charges_on()) { HIPCHK(hipStreamSynchronize(stream)); qtag.free(); cmask_dev.free(); eoutq.free(); return; }      // the array exists only while somebody reads it
    std::vector<R> hq((size_t)top.n);
    for (size_t t = 0; t < hq.size(); ++t) hq[t] = (R)top.q[t];
    std::vector<unsigned int> hm(coul_mask, coul_mask + CHEM_MAX_TYPES);
    qtag.upload(hq, stream); cmask_dev.upload(hm, stream);
    HIPCHK(hipStreamSynchronize(stream));
  }
  CoulArgs<R> coul_args(size_t nblocks) {
    if (eoutq.n < 2 * nblocks + 8) eoutq.alloc(2 * nblocks + 8);
    return CoulArgs<R>{qtag.p, tag.p, cmask_dev.p, eoutq.p, (R)coul_k, (R)(coul_rc * coul_rc)};
  }

  // Resolution: stamps by tag (lambda0, s0), rates by type, the mask of marked type pairs and their caps -- allocated only
  // while a type pair is marked; every rank of a decomposition holds all of them (the set-up calls are the same on every rank).
  DBuf<double2> rstamp; DBuf<double> ralpha; DBuf<unsigned int> rmask_dev; DBuf<R> rfmax;
  void upload_res() {
    res_dirty = false;
    if (!res_pairs_on()) { HIPCHK(hipStreamSynchronize(stream)); rstamp.free(); ralpha.free(); rmask_dev.free(); rfmax.free(); return; }
    std::vector<double2> hs((size_t)top.n, double2{1.0, 0.0});
    if (res.on()) for (size_t t = 0; t < hs.size(); ++t) hs[t] = double2{res.lambda0[t], (double)res.s0[t]};
    std::vector<double> ha(CHEM_MAX_TYPES);
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) ha[a] = res.rate[a].alpha;
    std::vector<unsigned int> hm(res_mask, res_mask + CHEM_MAX_TYPES);
    std::vector<R> hf((size_t)CHEM_MAX_TYPES * CHEM_MAX_TYPES);
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = 0; b < CHEM_MAX_TYPES; ++b) hf[(size_t)a * CHEM_MAX_TYPES + b] = (R)res_fmax[a][b];
    rstamp.upload(hs, stream); ralpha.upload(ha, stream); rmask_dev.upload(hm, stream); rfmax.upload(hf, stream);
    HIPCHK(hipStreamSynchronize(stream));
  }
  void res_push(const std::vector<int32_t>& tags) override {
    if (tags.empty() || res_dirty || !rstamp.p || !device_ready || particles_dirty) { if (!tags.empty()) res_dirty = true; return; }
    if (tags.size() > 16) { upload_res(); return; }      // (the stamps are not contiguous: beyond a few, one copy of all of them is cheaper)
    std::vector<double2> stage(tags.size());
    for (size_t k = 0; k < tags.size(); ++k) { const int32_t t = tags[k]; stage[k] = double2{res.lambda0[t], (double)res.s0[t]}; HIPCHK(hipMemcpyAsync(rstamp.p + t, &stage[k], sizeof(double2), hipMemcpyHostToDevice, stream)); }
    HIPCHK(hipStreamSynchronize(stream));
  }
  // Capped pairs: the squared cap radii by type pair -- allocated only while a type pair is capped; type-pair data, the same on
  // every rank of a decomposition.
  DBuf<R> capc2;
  void upload_cap() {
    cap_dirty = false;
    if (!caps_on()) { HIPCHK(hipStreamSynchronize(stream)); capc2.free(); return; }
    std::vector<R> hc((size_t)CHEM_MAX_TYPES * CHEM_MAX_TYPES);
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = 0; b < CHEM_MAX_TYPES; ++b) hc[(size_t)a * CHEM_MAX_TYPES + b] = (R)(cap_rad[a][b] * cap_rad[a][b]);
    capc2.upload(hc, stream);
    HIPCHK(hipStreamSynchronize(stream));
  }
  CapArgs<R> cap_args() const { return CapArgs<R>{capc2.p}; }
  ResArgs<R> res_args() const { return ResArgs<R>{rstamp.p, ralpha.p, tag.p, rmask_dev.p, rfmax.p, (long long)(step + force_step_off)}; }
  // Completion (chem_resolution_rate with a property change): every particle whose lambda reached 1 at the current step gets
  // its new type, mass, charge and state by the route of chem_modify_particle, and a stamp (1, step) under the new type.
  int res_apply_completions() override {
    const std::vector<ResCompletion> done = res.completions_at(step);
    if (done.empty()) return 0;
    join_async();      // the mirrors are written below
    std::vector<int32_t> tags;
    for (const ResCompletion& c : done) {
      const int32_t t = c.tag;
      top.type[t] = c.new_type; top.mass[t] = c.new_mass; top.q[t] = c.new_q;
      modify_particle(t, CHEM_STATE_TYPE, (double)c.new_type); modify_particle(t, CHEM_STATE_MASS, c.new_mass); modify_particle(t, CHEM_STATE_CHARGE, c.new_q);
      if (c.new_state >= 0) { top.state[t] = c.new_state; modify_particle(t, CHEM_STATE_STATE, (double)c.new_state); }
      res.stamp(t, 1.0, step); res.seen[t] = c.new_type; tags.push_back(t);
    }
    pair_dirty = true; bonded_dirty = true; resort = true;
    res_push(tags);
    return (int)done.size();
  }
  // Behind the reaction cadence of a step (dissociation, association, ATRP): types that changed are re-stamped, then the
  // lambda rules of the reactions (chem_reaction_set_resolution) act on this step's events, in arena order.
  void res_after_reactions() {
    join_async();      // the event log and the type mirrors of this step are complete
    res.ensure(top.type);
    std::vector<int32_t> changed;
    res.restamp_type_changes(top.type, step, changed);
    if (!res_rules.empty())
      for (size_t bk = arena.blocks.size(); bk-- > 0 && arena.blocks[bk].first == step;) {
        const size_t lo = arena.blocks[bk].second, hi = bk + 1 < arena.blocks.size() ? arena.blocks[bk + 1].second : arena.size();
        for (size_t k = lo; k < hi; ++k) {
          const auto it = res_rules.find(public_index(arena.r[k]));
          if (it == res_rules.end()) continue;
          if (it->second[0] >= 0.0) { res.stamp(arena.a[k], it->second[0], step); changed.push_back(arena.a[k]); }
          if (it->second[1] >= 0.0) { res.stamp(arena.b[k], it->second[1], step); changed.push_back(arena.b[k]); }
        }
      }
    res_push(changed);
  }

  // ---- fixed distances (chem_fix_add; rule set: include/chem_mi355.h, host routines: chem_fix_host.hpp) ----
  // The flat entry array is rewritten by the host at an add or a release only (both sit behind a synchronisation); it is freed
  // with the last entry, and a context without entries launches exactly what it launched before.
  DBuf<FixEnt<R>> fix_dev; int fix_n = 0;
  void upload_fix() {
    fix_dirty = false;
    const std::vector<FixEntry> all = fix.device_order();
    HIPCHK(hipStreamSynchronize(stream));
    fix_n = (int)all.size();
    if (all.empty()) { fix_dev.free(); return; }
    std::vector<FixEnt<R>> h(all.size());
    for (size_t k = 0; k < all.size(); ++k) { h[k] = FixEnt<R>{}; h[k].a = all[k].anchor; h[k].t = all[k].target; h[k].d = (R)all[k].dist; }
    fix_dev.upload(h, stream);
    HIPCHK(hipStreamSynchronize(stream));
  }
  void launch_fix() {
    if (fix_n <= 0) return;
    FixGeom<R> g{};
    for (int d = 0; d < 3; ++d) { g.L[d] = (R)L[d]; g.invL[d] = (R)(1.0 / L[d]); }
    hipLaunchKernelGGL((k_fix_distances<R>), dim3(cdiv(fix_n, 256)), dim3(256), 0, stream, fix_n, fix_dev.p, rtag.p, nglob, x4.p, v4.p, g, pos_scale(), (const DevCtl*)ctl.p);
  }
  // What a release does to its target: the post-process of the set that matches the target's current type, by the route of
  // the other host-decided property changes (mirrors, k_apply_props, charges), then the lambda stamp; the lists are rebuilt.
  int fix_apply_releases(const std::vector<FixRecord>& rel) {
    if (rel.empty()) return 0;
    const bool on_device = device_ready && !particles_dirty;      // (otherwise the mirrors alone: everything is uploaded later)
    std::vector<HostTopology::PropChange> chg;
    std::vector<std::pair<int32_t, double>> stamps;
    for (const FixRecord& r : rel) {
      const int32_t t = r.target;
      const FixPost* p = fix.post_for(r.set, top.type[t]);
      if (!p) continue;
      if (p->new_type >= 0) { top.type[t] = p->new_type; top.mass[t] = p->new_mass; top.q[t] = p->new_q; }
      if (p->new_state >= 0 && (!on_device || !state_mirror_stale)) top.state[t] = p->new_state;
      if (p->new_type >= 0 || p->new_state >= 0) chg.push_back(HostTopology::PropChange{t, top.type[t], p->new_state >= 0 ? 1 : 0, p->new_state >= 0 ? p->new_state : 0, top.mass[t], top.q[t]});
      if (p->lambda >= 0.0) stamps.emplace_back(t, p->lambda);
    }
    if (on_device) apply_prop_changes(chg);
    std::vector<int32_t> changed;
    if (res.on() || !stamps.empty()) {
      res.ensure(top.type);
      res.restamp_type_changes(top.type, step, changed);      // (re-stamped under the old type's rate first)
      for (const auto& s : stamps) { res.stamp((size_t)s.first, s.second, step); changed.push_back(s.first); }
      res_push(changed);
    }
    fix_dirty = true;
    if (!on_device) return (int)rel.size();
    if (!chg.empty() && any_typed_list()) upload_bonded(false);
    upload_fix();
    request_rebuild();      // the target's displacement was never tracked, and its new type pair may bring it onto the lists
    return (int)rel.size();
  }
  int fix_after_reactions(bool events) override {
    int nrel = 0;
    join_async();      // the event log and the type mirrors of this step are complete
    if (events && !fix.rules.empty()) {
      // this step's association events that formed a bond, in the order chem_get_events reports them: (min id, max id)
      struct Ev { int32_t a, b; int r; };
      std::vector<Ev> evs;
      for (size_t bk = arena.blocks.size(); bk-- > 0 && arena.blocks[bk].first == step;) {
        const size_t lo = arena.blocks[bk].second, hi = bk + 1 < arena.blocks.size() ? arena.blocks[bk + 1].second : arena.size();
        for (size_t k = lo; k < hi; ++k) if (arena.r[k] >= 0 && !reactions[arena.r[k]].is_virtual) evs.push_back(Ev{arena.a[k], arena.b[k], public_index(arena.r[k])});
      }
      std::sort(evs.begin(), evs.end(), [](const Ev& p, const Ev& q) { return std::make_pair(std::min(p.a, p.b), std::max(p.a, p.b)) < std::make_pair(std::min(q.a, q.b), std::max(q.a, q.b)); });
      std::vector<FixReactant> rc;
      for (const Ev& e : evs) { rc.push_back(FixReactant{e.r, 1, e.a}); rc.push_back(FixReactant{e.r, 2, e.b}); }
      nrel += fix_apply_releases(fix.release_by_reaction(rc, step));
    }
    nrel += fix_apply_releases(fix.release_by_type(top.type, step));
    return nrel;
  }
  // chem_add_particles after the first upload: the particle data goes back to the staging arrays (unfolded positions, so that
  // the images are counted again), everything per-tag is uploaded afresh with the larger set
  void add_particles_prepare() override {
    if (particles_dirty) return;
    const int64_t n0 = top.n;
    std::vector<double> p((size_t)3 * n0), v((size_t)3 * n0);
    get_state(CHEM_STATE_POS_UNFOLDED, p.data(), 3 * n0);
    get_state(CHEM_STATE_VEL, v.data(), 3 * n0);
    refresh_state_mirror();
    pos0 = std::move(p); vel0 = std::move(v);
    particles_dirty = true;
  }
  // Checkpoint: the particle data as the device holds it (coordinates not folded again, image counters beside them), so that
  // the upload that follows puts back exactly these words; chemical states into the mirror (types, masses, charges and labels
  // are current after join_async).  A context whose state is staged already (loaded or saved, not run since) has nothing to pull.
  void ckpt_count_builds() { const DevCtl h = read_ctl(); tm_base_rebuilds += h.ref_rebuilds; tm_base_list_rebuilds += h.rebuild_count; }
  void ckpt_pull() override {
    if (particles_dirty && !img0.empty()) return;
    flush_host_state();      // (a context that never ran: positions are folded and counted once, by the upload's own rule)
    HIPCHK(hipStreamSynchronize(stream));
    ckpt_count_builds();
    std::vector<int> ht; std::vector<V4> hx, hv; std::vector<int4> hi;
    tag.download(ht, (size_t)n, stream); x4.download(hx, (size_t)n, stream); v4.download(hv, (size_t)n, stream); img4.download(hi, (size_t)n, stream);
    pos0.assign((size_t)3 * n, 0.0); vel0.assign((size_t)3 * n, 0.0); img0.assign((size_t)3 * n, 0);
    for (int i = 0; i < n; ++i) {
      const size_t t = (size_t)ht[i];
      if (t >= (size_t)n) throw ChemError(CHEM_ESTATE, "internal: checkpoint found a tag outside the particle set");
      pos0[3 * t] = dec_pos(hx[i].x, 0); pos0[3 * t + 1] = dec_pos(hx[i].y, 1); pos0[3 * t + 2] = dec_pos(hx[i].z, 2);
      vel0[3 * t] = (double)hv[i].x; vel0[3 * t + 1] = (double)hv[i].y; vel0[3 * t + 2] = (double)hv[i].z;
      img0[3 * t] = hi[i].x; img0[3 * t + 1] = hi[i].y; img0[3 * t + 2] = hi[i].z;
    }
    refresh_state_mirror(true);
    particles_dirty = true;
  }
  void ckpt_reset() override {
    if (stream) HIPCHK(hipStreamSynchronize(stream));
    if (device_ready && !particles_dirty) ckpt_count_builds();      // (a load into a context that has run)
    state_mirror_stale = false; baro_replan_pending = false; react_tables_reserved = false;
    excl_deg.clear(); excl_deg_upto = 0; excl_over = 0;
    box_dev_valid = false;
  }

  // ---- per-tag CSR tables built on the device from flat, append-only arrays (md_kernels.hpp "Per-tag CSR tables") ----
  DBuf<int4> fent; DBuf<int> flist, eslot, bkey, tcnt, tcounts, type_tag; DBuf<SlotKey> skeys; DBuf<int2> epairs;
  size_t fent_n = 0, epairs_n = 0; std::vector<size_t> list_uploaded; int nslot = 0;
  DBuf<double2> btab_rows; DBuf<double4> btab_info; size_t btab_uploaded = 0;
  BTab btab_view() const { return BTab{btab_rows.p, btab_info.p}; }
  void upload_bond_tables() {
    if (btab_uploaded == top.btables.size()) return;
    std::vector<double2> rows; std::vector<double4> info;
    for (const HostBondTable& t : top.btables) {
      info.push_back(make_double4((double)rows.size(), t.itype == TAB_LINEAR ? (double)t.e.size() : -(double)t.e.size(), t.r0, 1.0 / t.dr));   // (sign: BTab)
      if (t.itype == TAB_LINEAR) for (size_t k = 0; k < t.e.size(); ++k) rows.push_back(make_double2(t.e[k], t.f[k]));
      else {
        const std::vector<double> co = pack_bond_rows(t.e.data(), t.f.data(), t.e.size(), t.itype);
        for (size_t k = 0; k < co.size(); k += 2) rows.push_back(make_double2(co[k], co[k + 1]));
      }
    }
    btab_rows.upload(rows, stream); btab_info.upload(info, stream);
    HIPCHK(hipStreamSynchronize(stream));
    btab_uploaded = top.btables.size();
  }
  template <typename T> static void grow(DBuf<T>& b, size_t used, size_t need, hipStream_t st) {   // keeps the first `used` elements
    if (need <= b.n) return;
    DBuf<T> nb; nb.alloc(std::max(need, b.n * 2 + 1024));
    if (used) HIPCHK(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    std::swap(b.p, nb.p); std::swap(b.n, nb.n);
  }
  DBuf<int> scan_tot;
  void scan_counts(int n, int* cnt, int* start) {
    const int nb = cdiv(n, kScanItems);
    scan_tot.alloc(std::max(nb, 1));
    hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(1024), 0, stream, n, cnt, start, scan_tot.p);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(1024), 0, stream, nb, scan_tot.p, n, start);
    hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(1024), 0, stream, n, (const int*)scan_tot.p, start);
  }
  // full = true: every tuple of every list again (set-up, parameter changes); false: only what the lists gained
  // since the last call (reaction steps).  Parameter slots are re-resolved against the current particle types on
  // the device either way.
  // wait = false: everything is only enqueued (reaction step: the host goes on with its own bookkeeping meanwhile);
  // the table sizes the host needs (entry and owner counts) are upper bounds from the flat arrays, the kernels
  // themselves read the exact figures from device memory
  size_t fent_members = 0;     // sum of arity * HostList::entry_width over the flat tuples
  std::vector<HBondedParam> stage_hp; std::vector<HostTopology::HSlotKey> stage_hk;
  PinnedVec<int4> stage_ne; PinnedVec<int> stage_nl; PinnedVec<int2> stage_ep;   // pinned: a pageable async copy blocks for ~0.1 ms
  void upload_bonded(bool full = true, bool wait = true) {
    upload_bond_tables();
    // (host staging lives in members: with wait = false the copies may still be in flight when this returns)
    std::vector<HBondedParam>& hp = stage_hp; std::vector<HostTopology::HSlotKey>& hk = stage_hk;
    top.build_params(hp, hk);
    static_assert(sizeof(HBondedParam) == sizeof(BondedParam) && sizeof(HostTopology::HSlotKey) == sizeof(SlotKey), "layout");
    nslot = (int)hp.size();
    // analytic pair terms only (the chain-growth systems): the per-step kernel without the angle / dihedral / table code
    bonds_only = nslot > 0;
    for (const auto& q : hp) bonds_only &= q.arity == 2 && (q.kind == CHEM_POT_HARMONIC || q.kind == CHEM_POT_FENE || q.kind == CHEM_POT_FENE_LJ || q.kind == CHEM_POT_LJ_BOND || q.kind == CHEM_POT_COULOMB_BOND);
    harmonic_only = nslot == 1 && hp[0].arity == 2 && hp[0].kind == CHEM_POT_HARMONIC;      // ONE harmonic parameter set (kernel arguments of the force launch)
    if (harmonic_only) { inline_K = hp[0].p[0]; inline_r0 = hp[0].p[1]; }
    if (full && harmonic_only) {
      // every listed pair must be an excluded pair (ChemLab's DynamicExcludeList observes the bond lists; a caller of the C ABI
      // need not): checked once against the host's exclusion rows; bonds made by reactions are excluded by construction
      bonds_excluded = true;
      for (const auto& l : top.lists) {
        if (l.arity != 2) continue;
        for (size_t e = 0; e < (size_t)l.size() && bonds_excluded; ++e) {
          const int32_t a_ = l.ent[2 * e], b_ = l.ent[2 * e + 1];
          bonds_excluded = std::binary_search(top.excl[a_].begin(), top.excl[a_].end(), b_);
        }
      }
    }
    bpar.alloc(std::max<size_t>(hp.size(), 1)); skeys.alloc(std::max<size_t>(hk.size(), 1));
    has_hybrid = top.any_hybrid();
    has_coul14 = top.any_coulomb_bond();
    if ((has_hybrid || has_coul14) && nslot) {      // (the _q kernels carry the lambda code: (1, 0) for slots that are not hybrid)
      static_assert(sizeof(std::array<double, 2>) == sizeof(double2), "layout");
      top.hybrid_params(hp, stage_hyb);
      bhyb.alloc(stage_hyb.size());
      HIPCHK(hipMemcpyAsync(bhyb.p, stage_hyb.data(), stage_hyb.size() * sizeof(double2), hipMemcpyHostToDevice, stream));
    }
    if (nslot) {
      HIPCHK(hipMemcpyAsync(bpar.p, hp.data(), hp.size() * sizeof(BondedParam), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(skeys.p, hk.data(), hk.size() * sizeof(SlotKey), hipMemcpyHostToDevice, stream));
    }
    if (full || list_uploaded.size() != top.lists.size()) { fent_n = 0; fent_members = 0; list_uploaded.assign(top.lists.size(), 0); }
    PinnedVec<int4>& ne = stage_ne; PinnedVec<int>& nl = stage_nl;
    ne.clear(); nl.clear();
    bool typed = false;
    for (size_t li = 0; li < top.lists.size(); ++li) {
      const HostList& l = top.lists[li];
      typed |= l.by_types != 0;
      const size_t have = (size_t)l.size();
      for (size_t e = list_uploaded[li]; e < have; ++e) {
        const int32_t* t = &l.ent[e * l.arity];
        int z = l.arity > 2 ? t[2] : -1;
        if (l.hybrid) {      // the birth step travels in the unused third tag (BondedEntry::t2) of a pair,
          if (l.birth[e] < 0 || l.birth[e] > 0x7fffffff) throw ChemError(CHEM_ESTATE, "hybrid list: birth step beyond 2^31 - 1");
          if (l.arity == 2) z = encode_birth(l.birth[e]);
        }
        ne.push_back(make_int4(t[0], t[1], z, l.arity > 3 ? t[3] : -1)); nl.push_back((int)li);
        // of a triple or quadruple in a second flat record that belongs to no list (k_bt_count passes it by, k_bt_fill reads it)
        if (l.hybrid && l.arity > 2) { ne.push_back(make_int4(encode_birth(l.birth[e]), -1, -1, -1)); nl.push_back(-1); }
      }
      fent_members += (have - list_uploaded[li]) * (size_t)(l.arity * l.entry_width());
      list_uploaded[li] = have;
    }
    grow(fent, fent_n, fent_n + ne.size(), stream); grow(flist, fent_n, fent_n + ne.size(), stream);
    if (!ne.empty()) {
      HIPCHK(hipMemcpyAsync(fent.p + fent_n, ne.data(), ne.size() * sizeof(int4), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(flist.p + fent_n, nl.data(), nl.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      fent_n += ne.size();
    }
    const int nt = nglob > 0 ? nglob : (int)top.n;
    if (tcnt.n < (size_t)nt + 1) { tcnt.alloc((size_t)nt + 1); HIPCHK(hipMemsetAsync(tcnt.p, 0, sizeof(int) * ((size_t)nt + 1), stream)); }
    bstart.alloc((size_t)nt + 1); tcounts.alloc(2);
    if (typed) type_tag.upload(top.type, stream);      // typed lists: the host keeps the type mirrors current (react_step)
    HIPCHK(hipMemsetAsync(tcounts.p, 0, 2 * sizeof(int), stream));
    const size_t ub = (fent_n && nslot) ? fent_members : 0;      // upper bound of the entry count (tuples without parameters drop out)
    if (ub) {
      const int ne_i = (int)fent_n;
      if (eslot.n < fent_n) eslot.alloc(fent_n + fent_n / 2 + 1024);          // (amortised: these grow at every reaction step)
      if (bent.n < ub) { bent.alloc(ub + ub / 2 + 1024); bkey.alloc(ub + ub / 2 + 1024); }
      hipLaunchKernelGGL((k_bt_count<R>), dim3(cdiv(ne_i, 256)), dim3(256), 0, stream, ne_i, fent.p, flist.p, nslot, skeys.p, x4.p, rtag.p,
                         typed ? (const int*)type_tag.p : (const int*)nullptr, eslot.p, tcnt.p);
      scan_counts(nt, tcnt.p, bstart.p);
      hipLaunchKernelGGL(k_bt_fill, dim3(cdiv(ne_i, 256)), dim3(256), 0, stream, ne_i, fent.p, eslot.p, skeys.p, bstart.p, tcnt.p, bent.p, bkey.p);
      hipLaunchKernelGGL(k_bt_sort, dim3(cdiv(nt, 256)), dim3(256), 0, stream, nt, bstart.p, tcnt.p, bent.p, bkey.p, tcounts.p);
    } else HIPCHK(hipMemsetAsync(bstart.p, 0, sizeof(int) * ((size_t)nt + 1), stream));
    nbent = (int64_t)ub; nb_owner = (int)std::min<size_t>((size_t)nt, ub);
    if (bwork.n < (size_t)std::max(nb_owner, 1)) bwork.alloc((size_t)nb_owner + nb_owner / 2 + 1024);
    if (bj.n < (size_t)std::max<int64_t>(nbent, 1)) bj.alloc((size_t)nbent + nbent / 2 + 1024);
    bwork_dirty = true;
    bonded_dirty = false;
    if (wait) HIPCHK(hipStreamSynchronize(stream));
  }

  // Reaction steps append to these tables; their first growth (device reallocation + copy, pinned reallocation of the
  // staging vectors: milliseconds each) is paid here, once, when a run with reactions starts -- sized for one bond
  // per particle, beyond that they grow geometrically as before.
  bool react_tables_reserved = false;
  std::vector<Candidate> bond_ev;       // bond-forming events of a reaction step in canonical order
  std::vector<Candidate> radix_tmp;     // scratch of the event sort (kept: a fresh 6 MB vector per step is 1.5 ms of page faults)
  void reserve_reaction_tables() {
    if (react_tables_reserved) return;
    react_tables_reserved = true;
    const size_t nt = (size_t)(nglob > 0 ? nglob : (int)top.n);
    const size_t per = top.spawns_tuples() ? (top.any_hybrid() ? 8 : 4) : 1;      // flat records a new bond may add (itself + spawned angles / dihedrals, two each in a hybrid list)
    for (auto& d : reactions) if (!d.is_virtual && d.bond_list >= 0 && d.bond_list < (int)top.lists.size()) {
      HostList& l = top.lists[d.bond_list];
      l.seen.reserve(l.seen.used + nt); l.ent.reserve(l.ent.size() + 2 * nt);
    }
    radix_tmp.reserve(nt / 2 + 1024); bond_ev.reserve(nt / 2 + 1024);
    stage_ne.reserve(nt / 2 * per + 1024); stage_nl.reserve(nt / 2 * per + 1024); stage_ep.reserve(nt / 2 * per + 1024);
    grow(fent, fent_n, fent_n + nt * per, stream); grow(flist, fent_n, fent_n + nt * per, stream);
    grow(epairs, epairs_n, epairs_n + nt * per, stream);
    const size_t ub = fent_members + 2 * nt * per;
    if (eslot.n < fent_n + nt * per) eslot.alloc(fent_n + nt * per);
    if (bent.n < ub) { DBuf<BondedEntry> nb_; nb_.alloc(ub); if (nbent > 0) HIPCHK(hipMemcpyAsync(nb_.p, bent.p, (size_t)nbent * sizeof(BondedEntry), hipMemcpyDeviceToDevice, stream));
                       HIPCHK(hipStreamSynchronize(stream)); std::swap(bent.p, nb_.p); std::swap(bent.n, nb_.n); bkey.alloc(ub); }
    if (bwork.n < nt) { bwork.alloc(nt); bwork_dirty = true; }
    if (bj.n < ub) { bj.alloc(ub); bwork_dirty = true; }
    if (excl_list.n < 3 * (epairs_n + nt * per) + 1024) {
      DBuf<int> nl_; nl_.alloc(3 * (epairs_n + nt * per) + 1024);
      if (epairs_n) HIPCHK(hipMemcpyAsync(nl_.p, excl_list.p, std::min(excl_list.n, 2 * epairs_n) * sizeof(int), hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream)); std::swap(excl_list.p, nl_.p); std::swap(excl_list.n, nl_.n);
    }
  }

  void upload_excl(bool full = true, bool wait = true) {
    if (full) epairs_n = 0;
    const size_t have = top.excl_log.size();
    const size_t add = have - epairs_n;
    grow(epairs, epairs_n, have, stream);
    static_assert(sizeof(std::pair<int32_t, int32_t>) == sizeof(int2), "layout");
    if (add) {
      stage_ep.resize(add);
      std::memcpy(stage_ep.data(), top.excl_log.data() + epairs_n, add * sizeof(int2));
      HIPCHK(hipMemcpyAsync(epairs.p + epairs_n, stage_ep.data(), add * sizeof(int2), hipMemcpyHostToDevice, stream));
    }
    epairs_n = have;
    const int nt = nglob > 0 ? nglob : (int)top.n;
    if (tcnt.n < (size_t)nt + 1) { tcnt.alloc((size_t)nt + 1); HIPCHK(hipMemsetAsync(tcnt.p, 0, sizeof(int) * ((size_t)nt + 1), stream)); }
    excl_start.alloc((size_t)nt + 1);
    if (excl_list.n < std::max<size_t>(2 * have, 1)) excl_list.alloc(3 * have + 1024);
    if (have) {
      const int m = (int)have;
      hipLaunchKernelGGL(k_ex_count, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, epairs.p, tcnt.p);
      scan_counts(nt, tcnt.p, excl_start.p);
      hipLaunchKernelGGL(k_ex_fill, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, epairs.p, excl_start.p, tcnt.p, excl_list.p);
      hipLaunchKernelGGL(k_ex_sort, dim3(cdiv(nt, 256)), dim3(256), 0, stream, nt, excl_start.p, tcnt.p, excl_list.p);
    } else HIPCHK(hipMemsetAsync(excl_start.p, 0, sizeof(int) * ((size_t)nt + 1), stream));
    if (wait) HIPCHK(hipStreamSynchronize(stream));
    has_excl = have ? 1 : 0;
    excl_dirty = false; resort = true;
  }

  void flush_host_state() {
    if (top.n <= 0 || !(L[0] > 0) || !(rc > 0)) throw ChemError(CHEM_ESTATE, "system incomplete: need box, cutoff and particles");
    if (particles_dirty) upload_particles();
    if (geom_dirty) setup_geometry();
    if (labels_dirty) upload_labels();
    if (pair_dirty) upload_pair();
    if (coul_dirty) upload_coul();
    if (res_dirty) upload_res();
    if (cap_dirty) upload_cap();
    if (fix_dirty) upload_fix();
    if (bonded_dirty) upload_bonded();
    if (excl_dirty) upload_excl();
  }

  // ---- rebuild chain (every kernel early-exits unless ctl->need_rebuild) ---------------
  // Grids are capped ("persistent" grid-stride kernels) so that the early-exit launches of the
  // steps that do not rebuild cost ~2 us each instead of a full-size dispatch.
  void launch_sort_chain(int i0, int npart) {
    const int nb = std::max(1, std::min(cdiv(npart, 256), 2048));
    DevCtl* c = ctl.p;
    MigBuf<R> mdn{}, mup{};
    if (dd_on) { mdn = mig_view(0); mup = mig_view(1); }
    hipLaunchKernelGGL(k_bin<R>, dim3(nb), dim3(256), 0, stream, i0, npart, x4.p, v4.p, tag.p, img4.p, box, cell_cnt.p, cell_of.p, slot_of.p, mdn, mup, c);
  }
  void launch_list_chain() {
    DevCtl* c = ctl.p;
    const R rl2 = (R)((rc + skin_eff()) * (rc + skin_eff())), rl2_rows = (R)((rc + skin) * (rc + skin));   // (they differ on the tile path only)
    if (use_tiles) {
      BondRecs bs{}, record{};      // inline bonds (decomposed path: the standalone list kernel records the partner slots ...)
      int list_excl = has_excl;
      if (dd_on && bonds_inline()) {
        bs = bond_recs((size_t)acap());
        // (... unless the bond pass is on: the list build ignores the exclusions = bonds, k_bond_slots behind it records the
        //  partner slots and every force launch takes the partners' pair term out again, as on the fused path)
        if (bond_by_pass() && !want32) { record = bs; bs = BondRecs{}; list_excl = 0; }
      }
      hipLaunchKernelGGL((k_tile_desc<R>), dim3(std::min(ntiles, 2048)), dim3(128), 0, stream, ntiles, tile_cap, cell_start.p, box, tdesc.p, c, (const int*)cell_sub.p);
      hipLaunchKernelGGL((k_tile_scan<R>), dim3(1), dim3(1024), 0, stream, ntiles, tdesc.p, c);
      // slabs: the excluded partners of a particle are located as slots like on the fused path (ghost copies through gtag) --
      // without it every hit of a particle with exclusions paid a tag gather and a row scan (late stage: this launch 0.36 -> 1.59 ms)
      const Box<R>* bxp = nullptr;
      if (dd_on && has_excl && opt_dd_fastx && gtag.p && !(bond_by_pass() && !want32)) {
        if (!box_dev.p) box_dev.alloc(1);
        if (!box_dev_valid || std::memcmp(&box, &box_dev_host, sizeof(box)) != 0) {
          std::memcpy(&box_dev_host, &box, sizeof(box)); box_dev_valid = true;
          HIPCHK(hipMemcpyAsync(box_dev.p, &box_dev_host, sizeof(box), hipMemcpyHostToDevice, stream));
        }
        bxp = box_dev.p;
      }
      hipLaunchKernelGGL((k_nlist_tiles<R, 512>), dim3(ntiles), dim3(512), list_lds_need(want32), stream, ntiles, tile_cap, x4.p, tag.p, tdesc.p, rl2,
                         excl_start.p, excl_list.p, list_excl, act, ntypes, nl16.p, S, nnh.p, want32 ? nlist.p : (int*)nullptr, S, nn.p, c, rl2_rows, bs,
                         bxp, (const int*)rtag.p, (const int*)gtag.p, G, G + n, opt_coop_overflow);
      if (record)
        hipLaunchKernelGGL((k_bond_slots<R>), dim3(ntiles), dim3(256), 0, stream, ntiles, (const TileLDS<R>*)tdesc.p, (const int*)tag.p, (const int*)excl_start.p,
                           (const int*)excl_list.p, (const int*)rtag.p, (const int*)gtag.p, G, G + n, (const V4*)x4.p, box, record, c);
    } else if (box.nc[0] > 0)
      hipLaunchKernelGGL((k_nlist_cells<R, 1536>), dim3(std::min(box.ncell, 2560)), dim3(256), 0, stream, n, x4.p, tag.p, cell_start.p, box, rl2,
                         excl_start.p, excl_list.p, has_excl, nlist.p, nn.p, S, c);
    else
      hipLaunchKernelGGL(k_nlist_brute<R>, dim3(cdiv(n, 4)), dim3(256), 0, stream, n, x4.p, tag.p, box, rl2, excl_start.p,
                         excl_list.p, has_excl, nlist.p, nn.p, S, c);
  }
  // the binned particles [base, base + count) into cell order, the sorted copies of the cells [c_first, c_last) back in place
  void launch_cell_sort(int base, int count, int c_first, int c_last) {
    DevCtl* c = ctl.p;
    const int nb = std::max(1, std::min(cdiv(count, 256), 2048));
    hipLaunchKernelGGL(k_scan_cells, dim3(1), dim3(1024), 0, stream, box.ncell, base, cell_cnt.p, cell_start.p, c);
    hipLaunchKernelGGL(k_place, dim3(nb), dim3(256), 0, stream, base, count, cell_of.p, slot_of.p, cell_start.p, perm.p, c);
    hipLaunchKernelGGL(k_sort_gather<R>, dim3(std::min(cdiv(box.ncell, 4), 2048)), dim3(256), 0, stream, box.ncell, cell_start.p, perm.p,
                       x4.p, v4.p, tag.p, img4.p, x4o.p, v4o.p, tago.p, img4o.p, c, box, cell_sub.p);
    if (dd_on) {
      // what a slab clears before the sorted copies come back: the tag maps, and the sub-bin words of the two ghost layers
      // (filled by the neighbours' particles afterwards: no sub-bin information for their cells)
      const int nxy = box.nc[0] * box.nc[1];
      if (gtag.n < (size_t)nglob) gtag.alloc(nglob);
      hipLaunchKernelGGL(k_dd_clear, dim3(cdiv(std::max(nglob, nxy), 256)), dim3(256), 0, stream, rtag.p, gtag.p, nglob, cell_sub.p, cell_sub.p + (size_t)(ncz + 1) * nxy, nxy);
    }
    hipLaunchKernelGGL(k_copyback<R>, dim3(nb), dim3(256), 0, stream, cell_start.p, c_first, c_last, x4o.p, v4o.p, tago.p, img4o.p, x4.p, v4.p, tag.p, img4.p, rtag.p, x0.p, c);
  }
  void launch_rebuild_chain() {   // single domain
    launch_sort_chain(0, n);
    launch_cell_sort(0, n, 0, box.ncell);
    launch_list_chain();
  }

  void decide_and_rebuild(bool publish = false) {
    if (use_fused) { tbeg(1); launch_rebuild_fused(publish); tend(); return; }
    hipLaunchKernelGGL(k_rebuild_decide<R>, dim3(1), dim3(1024), 0, stream, ctl.p, blockmax.p, cdiv(n, kIntPerBlock), half_skin_eff(), opt_criterion, 3, (const double*)nullptr, 0, (volatile int*)nullptr, 0, half_skin_ref());
    launch_rebuild_chain();
  }

  // ---- slab decomposition ---------------------------------------------------------------
  void ensure_hflag() {
    if (hflag) return;
    HIPCHK(hipHostMalloc((void**)&hflag, 4096, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(hflag, 0, 4096);
    HIPCHK(hipHostGetDevicePointer((void**)&hflag_dev, hflag, 0));
    dd_vals.alloc(64 * kFoldSlots);
    foldmax.alloc(2 * kFoldSlots);
    HIPCHK(hipMemsetAsync(foldmax.p, 0, 2 * kFoldSlots * sizeof(unsigned long long), stream));
    hint_host()->step = -1;
  }
  void poll_ticket(volatile int* word, int ticket, const char* what) {
    long long spins = 0;
    while (*word != ticket) {
      if ((++spins & 0xfffff) == 0 && hipStreamQuery(stream) != hipErrorNotReady) {   // stream drained or failed: re-check once, then give up
        if (*word == ticket) break;
        HIPCHK(hipStreamSynchronize(stream));
        if (*word != ticket) throw ChemError(CHEM_EDEVICE, std::string(what) + " never arrived from the device");
      }
    }
  }
  // up to 8 device integers with one poll instead of one blocking copy each
  int collect_ticket = 0;
  void collect_ints(std::initializer_list<const int*> src, int* out) {
    ensure_hflag();
    CollectArgs a{}; a.n = 0;
    for (const int* p : src) a.src[a.n++] = p;
    const int ticket = ++collect_ticket;
    hipLaunchKernelGGL(k_collect_ints, dim3(1), dim3(64), 0, stream, a, (volatile int*)(hflag_dev + 16), ticket);
    poll_ticket(hflag + 16, ticket, "slab rebuild counters");
    for (int k = 0; k < a.n; ++k) out[k] = hflag[17 + k];
  }
  void set_need_rebuild_async(int v) { HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&ctl.p->need_rebuild, v, 1, stream)); }

  int read_int(const int* dev) {
    int v = 0;
    HIPCHK(hipMemcpyAsync(&v, dev, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return v;
  }

  // Host-synchronous rebuild of one slab: migrate leavers to the z-neighbours, sort the reals,
  // exchange the boundary layers as ghosts (contiguous slices of the cell-sorted arrays), rebuild
  // cells/tiles/lists.  Every rank enters together (the trigger is a cross-rank maximum).
  void rebuild_dd() {
    Trace trd("dd");
    const int nxy = box.nc[0] * box.nc[1];
    // (need_rebuild on, force_rebuild off: the request is being served; migration headers cleared)
    hipLaunchKernelGGL(k_dd_begin, dim3(1), dim3(64), 0, stream, ctl.p, reinterpret_cast<int*>(mig[0].p), reinterpret_cast<int*>(mig[1].p));
    // 1. bin the reals; leavers go to the migration buffers
    launch_sort_chain(G, n);
    // 2. migration exchange (fixed-capacity buffers, count in the header)
    tr->exchange(mig[0].p, mig_bytes(), mig[1].p, mig_bytes(), mig[2].p, mig_bytes(), mig[3].p, mig_bytes(), lower, upper, stream);
    int cnt2[2];
    collect_ints({reinterpret_cast<const int*>(mig[2].p), reinterpret_cast<const int*>(mig[3].p)}, cnt2);
    const int from_up = cnt2[0], from_lo = cnt2[1];
    trd.lap("bin+migrate+poll");
    if (from_up > mcap || from_lo > mcap) throw ChemError(CHEM_ENOSPC, "domain decomposition: migration buffer overflow");
    if (G + n + from_lo + from_up > cap - G) throw ChemError(CHEM_ENOSPC, "domain decomposition: slab capacity exceeded by arrivals");
    // 3. arrivals behind the current reals, then bin them too (they are in their own slab now)
    if (from_lo) hipLaunchKernelGGL(k_append_arrivals<R>, dim3(cdiv(from_lo, 256)), dim3(256), 0, stream, mig_view(3), from_lo, G + n, x4.p, v4.p, tag.p, img4.p);
    if (from_up) hipLaunchKernelGGL(k_append_arrivals<R>, dim3(cdiv(from_up, 256)), dim3(256), 0, stream, mig_view(2), from_up, G + n + from_lo, x4.p, v4.p, tag.p, img4.p);
    const int npend = n + from_lo + from_up;
    HIPCHK(hipMemsetAsync(mig[0].p, 0, 16, stream)); HIPCHK(hipMemsetAsync(mig[1].p, 0, 16, stream));
    if (from_lo + from_up) launch_sort_chain(G + n, from_lo + from_up);
    // 4. sort the reals into [G, G + n_new): the own (non-ghost) cell layers
    launch_cell_sort(G, npend, nxy, (ncz + 1) * nxy);
    // 5. boundary-layer counts to the neighbours
    lcnt_dn.alloc(nxy + 1); lcnt_up.alloc(nxy + 1); gcnt_lo.alloc(nxy + 1); gcnt_up.alloc(nxy + 1);
    hipLaunchKernelGGL(k_layer_counts, dim3(cdiv(nxy + 1, 256)), dim3(256), 0, stream, nxy, ncz, cell_start.p, lcnt_dn.p, lcnt_up.p);
    tr->exchange(lcnt_dn.p, (nxy + 1) * sizeof(int), lcnt_up.p, (nxy + 1) * sizeof(int), gcnt_up.p, (nxy + 1) * sizeof(int), gcnt_lo.p,
                 (nxy + 1) * sizeof(int), lower, upper, stream);
    int c7[7];
    collect_ints({cell_start.p + (size_t)(ncz + 1) * nxy, reinterpret_cast<const int*>(mig[0].p), reinterpret_cast<const int*>(mig[1].p),
                  lcnt_dn.p + nxy, lcnt_up.p + nxy, gcnt_lo.p + nxy, gcnt_up.p + nxy}, c7);
    trd.lap("sort+counts+poll");
    n = c7[0] - G;
    if (c7[1] || c7[2]) throw ChemError(CHEM_ESTATE, "domain decomposition: a migrated particle left its new slab immediately");
    halo_dn_off = G; halo_dn_cnt = c7[3];
    halo_up_cnt = c7[4]; halo_up_off = G + n - halo_up_cnt;
    nglo = c7[5]; ngup = c7[6];
    if (nglo > G || G + n + ngup > cap) throw ChemError(CHEM_ENOSPC, "domain decomposition: ghost layer exceeds the reserved capacity");
    // 6. ghost particles: contiguous slices, received in place (lower ghosts right-aligned in front of the reals)
    tr->exchange2(halo_msg(),
                  Transport::Msg{tag.p + halo_dn_off, halo_dn_cnt * sizeof(int), tag.p + halo_up_off, halo_up_cnt * sizeof(int), tag.p + G + n, ngup * sizeof(int),
                                 tag.p + G - nglo, nglo * sizeof(int)}, lower, upper, stream);
    hipLaunchKernelGGL(k_ghost_cells, dim3(1), dim3(1024), 0, stream, nxy, ncz, gcnt_lo.p, gcnt_up.p, cell_start.p);
    if (nglo + ngup) hipLaunchKernelGGL(k_ghost_rtag, dim3(cdiv(nglo + ngup, 256)), dim3(256), 0, stream, G - nglo, nglo, G + n, ngup, tag.p, rtag.p, gtag.p);
    // 7. tiles + lists over the own layers.  A stencil beyond the LDS tile capacity or a row beyond its stride is a LOCAL matter
    //    (both capacities are per rank, no collective depends on them): grow and build the lists again, here, instead of
    //    carrying the flag to the end of the call and failing there (tests/test_gpu_sweep.py: a trimer melt at rho = 0.3
    //    outgrew the capacity estimated from its first configuration in the middle of a run)
    for (int attempt = 0; attempt < 4; ++attempt) {
      launch_list_chain();
      if (!use_tiles) break;
      int ov[2];
      collect_ints({&ctl.p->stage_overflow, &ctl.p->nl_overflow}, ov);
      if (!ov[0] && !ov[1]) break;
      if (ov[0]) {
        const int want = grown_tile_cap(ov[0]), old_cap = tile_cap;
        if (want <= tile_cap || tile_lds_need(want, slot_word_on(), res_lds_extra()) > kTileLdsBudget) break;      // (stays flagged: reported by check_flags / rebuild_now)
        tile_cap = want;
        set_tile_lds_attr();
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&ctl.p->stage_overflow, 0, 1, stream));
        if (g_trace) fprintf(stderr, "[chem trace] slab rebuild: staged-tile capacity %d -> %d slots\n", old_cap, tile_cap);
      }
      if (ov[1]) {
        if (nl_capacity_user > 0) break;
        S = grown_row_stride(ov[1], nglob);
        alloc_lists();
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&ctl.p->nl_overflow, 0, 1, stream));
        if (g_trace) fprintf(stderr, "[chem trace] slab rebuild: list rows grown to %d entries\n", S);
      }
    }
    set_need_rebuild_async(0);
    if (g_trace) { HIPCHK(hipStreamSynchronize(stream)); trd.lap("ghosts+tiles+list"); }
    bwork_dirty = true;   // particle order and ghosts changed: the bonded work list is rebuilt before the next force evaluation
    ++dd_rebuilds;
  }

  // ghost positions: the own boundary layers are contiguous slices of x4, received straight into the ghost ranges
  Transport::Msg halo_msg() const {
    return Transport::Msg{x4.p + halo_dn_off, halo_dn_cnt * sizeof(V4), x4.p + halo_up_off, halo_up_cnt * sizeof(V4), x4.p + G + n, ngup * sizeof(V4),
                          x4.p + G - nglo, nglo * sizeof(V4)};
  }
  // per-step ghost position update
  void halo_update() { tr->exchange(halo_msg(), lower, upper, stream); }

  DevCtl read_ctl() {
    DevCtl h;
    HIPCHK(hipMemcpyAsync(&h, ctl.p, sizeof(DevCtl), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return h;
  }
  template <typename F> void set_ctl_field(F DevCtl::*field, F value) {
    DevCtl* base = nullptr;
    size_t off = (size_t)((char*)&(base->*field) - (char*)base);
    HIPCHK(hipMemcpyAsync((char*)ctl.p + off, &value, sizeof(F), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }

  // forced synchronous rebuild (run() prologue, observe); grows the row stride on overflow
  // resumed: the step at which the device stopped the run is redone.  DevCtl::force_rebuild then says how the launch counts
  // (left by the device: 2, a regular decision; 4 where the stopped launch had counted the step already), so that rebuilds,
  // list_rebuilds and the accumulated distances come out as in a run that never stopped.  An attempt that has not counted the
  // step (it met a full bucket row before its first barrier) leaves the step's fold words and the accumulated distance of
  // parity halt_par untouched and clears only the other set: the next attempt reads the same parity again.  The resumed launch
  // publishes like any step's (the host's look-ahead waits for this step at the next one).
  void rebuild_now(bool resumed = false, int halt_kind = 0, int halt_par = 0) {
    const double t0 = now_s();
    hint_invalidate();
    baro_keep = false;      // (a list build re-sorts the particles, not f4)
    region_keep = false;
    bool counted = resumed && halt_kind == 3;
    for (int attempt = 0; attempt < 6; ++attempt) {
      if (dd_on) {      // (a slab rebuild the host calls for, not one of the device's decisions: counted on the host)
        set_ctl_field(&DevCtl::force_rebuild, 0); set_ctl_field(&DevCtl::acc_maxdist, 0.0); set_ctl_field(&DevCtl::acc_ref, 0.0);
        HIPCHK(hipMemsetAsync(ctl.p->acc_pp, 0, 2 * sizeof(double), stream));
        if (attempt == 0) ++dd_direct_rebuilds;
        rebuild_dd();
      }
      else {
        if (!resumed) {
          set_ctl_field(&DevCtl::force_rebuild, 1);
          // (nothing depends on the maxima of a forced decision: words left behind by a path that does not read them go)
          if (foldmax.p && !dd_on) HIPCHK(hipMemsetAsync(foldmax.p, 0, 2 * kFoldSlots * sizeof(unsigned long long), stream));
        }
        else if (counted) set_ctl_field(&DevCtl::force_rebuild, 4);
        else fused_par = halt_par;
        decide_and_rebuild(resumed);
      }
      DevCtl h = read_ctl();
      if (resumed && !h.bucket_overflow) counted = true;      // (a launch that got past its first barrier has counted the step)
      if (dd_on) agree_flags(h);
      if (h.halt) set_ctl_field(&DevCtl::halt, 0);       // (a launch that could not finish its lists also stopped the run: this IS the recovery)
      if (h.mig_error) throw ChemError(CHEM_ESTATE, "domain decomposition: particle migration error " + std::to_string(h.mig_error));
      if (h.barrier_timeout) throw ChemError(CHEM_ESTATE, "fused rebuild: grid barrier timed out (device shared with another job?); set option fused_rebuild=0");
      if (h.bucket_overflow) {
        // a cell more crowded than a bucket row: widen the rows up to what one wave sorts (64), beyond that this
        // system needs the unfused chain (its crowded-cell path ranks through global memory)
        set_ctl_field(&DevCtl::bucket_overflow, 0);
        set_ctl_field(&DevCtl::halt, 0);       // (the launch that met the full row also stopped the run: this IS the recovery)
        if (h.bucket_overflow <= 64 && bcap < 64) {
          bcap = 64; bucket.alloc((size_t)box.ncell * bcap);
          HIPCHK(hipMemsetAsync(bucket.p, 0, sizeof(int) * (size_t)box.ncell * bcap, stream));   // (the sort phase reads whole rows: entries must always be valid indices)
        }
        else { use_fused = false; if (g_trace) fprintf(stderr, "[chem trace] cell with %d particles: fused rebuild off\n", h.bucket_overflow); }
        continue;
      }
      if (h.stage_overflow) {
        // denser than the mean-occupancy estimate (clusters, chains): grow the staged-tile capacity while it
        // fits the LDS, then build again; beyond that the system is too crowded for tiles
        const int want = grown_tile_cap(h.stage_overflow);
        if (use_tiles && want > tile_cap) {
          if (tile_lds_need(want, slot_word_on(), res_lds_extra()) <= kTileLdsBudget) {
            if (g_trace) fprintf(stderr, "[chem trace] staged-tile capacity %d -> %d slots\n", tile_cap, want);
            tile_cap = want;
            set_tile_lds_attr(); setup_fused();
            set_ctl_field(&DevCtl::stage_overflow, 0);
            continue;
          }
          if (!dd_on) {
            // the stencil no longer fits the LDS next to the list build's image: this system continues on the per-cell
            // kernels (int32 rows, positions through L1/L2) instead of failing
            use_tiles = false; use_fused = false; ntiles = 0;
            alloc_lists();
            set_ctl_field(&DevCtl::stage_overflow, 0);
            if (g_trace) fprintf(stderr, "[chem trace] stencil of %d particles does not fit the LDS: per-cell kernels\n", h.stage_overflow);
            continue;
          }
        }
        throw ChemError(CHEM_ENOSPC, "cell stencil holds " + std::to_string(h.stage_overflow) + " particles, LDS tile capacity " + std::to_string(use_tiles ? tile_cap : 1536) + " (local density too high for the LDS-staged tiles; set option tiles=0)");
      }
      if (!h.nl_overflow) { resort = false; tm.rebuild_wall_s += now_s() - t0; return; }
      if (nl_capacity_user > 0) throw ChemError(CHEM_ENOSPC, "neighbour capacity " + std::to_string(S) + " too small, need " + std::to_string(h.nl_overflow));
      S = grown_row_stride(h.nl_overflow, dd_on ? nglob : n);
      alloc_lists();
      set_ctl_field(&DevCtl::nl_overflow, 0);
    }
    throw ChemError(CHEM_ENOSPC, "neighbour list capacity could not be satisfied");
  }

  // every rank must take the same branch after a collective rebuild: maxima of the flag words
  void agree_flags(DevCtl& h) {
    double v[4] = {(double)h.nl_overflow, (double)h.stage_overflow, (double)h.mig_error, (double)h.skin_violation};
    HIPCHK(hipMemcpyAsync(redbuf.p, v, sizeof(v), hipMemcpyHostToDevice, stream));
    tr->allreduce_max_f64(redbuf.p, 4, stream);
    HIPCHK(hipMemcpyAsync(v, redbuf.p, sizeof(v), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    h.nl_overflow = (int)v[0]; h.stage_overflow = (int)v[1]; h.mig_error = (int)v[2]; h.skin_violation = (int)v[3];
  }
  // the host sums v[0..nv) of an observable, summed over the ranks of a decomposition in place (through buf; one rank: nothing)
  void allreduce_host_sums(double* v, int nv, DBuf<double>& buf) {
    if (!(dd_on && P > 1)) return;
    buf.alloc((size_t)nv);
    HIPCHK(hipMemcpyAsync(buf.p, v, sizeof(double) * nv, hipMemcpyHostToDevice, stream));
    tr->allreduce_sum_f64(buf.p, nv, stream);
    HIPCHK(hipMemcpyAsync(v, buf.p, sizeof(double) * nv, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }

  // ---- forces -------------------------------------------------------------------------
  int pick_tpp() const { return chem::pick_tpp(use_tiles, n, opt_tpp); }

  // what a pair launch asks its plan with (pair_plan, tensor_plan)
  PairInput pair_input(bool energy) {
    PairInput in{use_tiles, n, opt_tpp, pair_bs, energy, coul_on(), res_pairs_on(), caps_on(), lj_only, uniform_lj, cubic_tab, dbg_on || opt_ablate != 0, 0, 0, 0, 0};
    if (in.coul && in.res) first_res_pair(res_mask, in.res_a, in.res_b);
    if (in.coul && in.cap) first_cap_pair(cap_rad, in.cap_a, in.cap_b);
    return in;
  }
  // bond_mode of a pair launch over the tiles: 0 no inline bonds, 1 / 2 what the LAST rebuild did (both only change where a rebuild
  // is forced); the partner slots are recorded by the rebuild itself either way
  int inline_bond_mode() { return bonds_inline() ? (bond_by_pass() ? 2 : 1) : 0; }

  // the pair forces into fdst (ENERGY: and the energy words into eout); the kernel is chem_launch_host.hpp's choice
  template <bool ENERGY> int launch_pair(V4* fdst) {
    const double hs = half_skin_eff();
    const PairPlan plan = pair_plan(pair_input(ENERGY));
    if (plan.code != CHEM_OK) throw ChemError(plan.code, pair_refusal_text(plan));
    const PairVariant& v = plan.v;
    const int bond_mode = inline_bond_mode();
    const bool inline_now = bond_mode != 0;
    if (use_tiles) {
      // which tiles: all (default), or the interior / boundary subset of a slab (see TileSub)
      const TileLayers tl = tile_subset(ntiles, ntxy(), pair_subset);
      const TileSub ts{tl.base1, tl.n1, tl.base2};
      const int nsub = tl.count;
      if (nsub <= 0) return 0;
      // what every tile kernel takes, then what MODE 0..3 and MODE 4..7 take behind it
      auto launch = [&](auto kern, const auto&... tail) {
        hipLaunchKernelGGL(kern, dim3(nsub), dim3(v.block), pair_lds_bytes(), stream, nsub, tile_cap, x4.p, fdst, tdesc.p, nl16.p, nnh.p, S, pcore.p, pext.p, ntypes, tab.p, tail...);
      };
      auto feature = [&](auto kern, const auto&... packs) { launch(kern, eout.p, hs, ctl.p, pair_guard, ts, pair_da, packs...); };
      with_tile_kernel<R>(v, [&](auto kern, auto M_) {
        constexpr int M = decltype(M_)::value;
        if constexpr (M == 4) feature(kern, coul_args((size_t)nsub));
        else if constexpr (M == 5) feature(kern, res_args());
        else if constexpr (M == 6) feature(kern, cap_args());
        else if constexpr (M == 7) feature(kern, res_args(), cap_args());
        else launch(kern, uni, eout.p, hs, ctl.p, pair_guard, opt_ablate, dbg_on ? dbgbuf.p : (long long*)nullptr, ts, pair_da,
                    (inline_now && (!ENERGY || bond_mode >= 2)) ? BondRecs{brec0.p, brec1.p} : BondRecs{}, inline_K, inline_r0, bond_mode, act);
      });
      return ntiles;
    }
    const int nb = cdiv((long long)n * v.tpp, 256);
    auto launch = [&](auto kern, const auto&... packs) {
      hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, stream, n, x4.p, fdst, nlist.p, nn.p, S, box, pcore.p, pext.p, ntypes, tab.p, eout.p, hs, ctl.p, packs...);
    };
    with_row_kernel<R>(v, [&](auto kern, auto M_) {
      constexpr int M = decltype(M_)::value;
      if constexpr (M == 4) launch(kern, coul_args((size_t)nb));
      else if constexpr (M == 5) launch(kern, res_args());
      else if constexpr (M == 6) launch(kern, cap_args());
      else if constexpr (M == 7) launch(kern, res_args(), cap_args());
      else launch(kern, CoulArgs<R>{});
    });
    return nb;
  }

  void compute_forces(bool speculative = false, int subset = 0, bool decide = false) {      // decide: single domain, no neighbour launch on this step (guard 3)
    pair_guard = decide ? 3 : (speculative ? (pair_da.gathered ? 2 : 1) : 0);
    pair_subset = subset;
    const bool timed = timed_step && subset == 0;
    if (timed) tbeg(0);
    launch_pair<false>(f4.p);
    if (timed) tend();
    pair_subset = 0;
    if (subset == 1) { pair_guard = 0; return; }   // interior tiles only: bonded terms follow with the boundary launch
    // the bonded term (chem_launch_host.hpp): nothing where the force kernel has evaluated the harmonic bonds (inline bonds)
    const BondedPlan bp = bonded_plan(BondedInput{nbent, nbent > 0 && bonds_inline(), excl_over, use_fused || dd_on, has_coul14, has_hybrid, bonds_only, nb_owner});
    if (bp.launch == BondedLaunch::work_list) {
      // work-list kernel: owners only, partner indices resolved at the last rebuild
      if (bwork_dirty) {   // bonded lists changed without a rebuild since
        HIPCHK(hipMemsetAsync(&ctl.p->bw64, 0, sizeof(unsigned long long), stream));
        hipLaunchKernelGGL(k_bonded_prep, dim3(std::max(1, std::min(cdiv(n, 256), 1024))), dim3(256), 0, stream, G, n, tag.p, rtag.p, bstart.p, bent.p, bwork.p, bj.p, ctl.p,
                           bp.inline_bonds ? (const int*)excl_start.p : (const int*)nullptr);
        bwork_dirty = false;
      }
      if (timed) tbeg(3);
      if (bp.bonds_only) launch_bonded_work<true>(bp.kind, bp.nown, speculative ? 1 : 0);
      else launch_bonded_work<false>(bp.kind, bp.nown, speculative ? 1 : 0);
      if (timed) tend();
    } else if (bp.launch == BondedLaunch::per_particle) {
      launch_bonded_each<false>(bp.kind, f4.p);
    }
    pair_guard = 0;
  }
  // The bonded kernel of a family (bonded_kind, chem_launch_host.hpp) behind `launch`'s own arguments: hybrid lists add the lambda
  // of every hybrid entry at the step these forces belong to, a 1-4 Coulomb list the charges by tag as well, read at every
  // evaluation (and what `more` holds).
  template <class Launch, class K0, class K1, class K2, class... More>
  void launch_bonded_kind(BondedKind kind, Launch launch, K0 plain, K1 hyb, K2 charged, const More&... more) {
    if (kind == BondedKind::charged) launch(charged, hybrid_args(), (const R*)qtag.p, more...);
    else if (kind == BondedKind::hybrid) launch(hyb, hybrid_args());
    else launch(plain);
  }
  // Observables per list (energies, virials, virial tensors): the passes leave ncomp words per entry of bent in `lent`,
  // k_list_sums adds them up per list in an order that depends on the entry table alone: the same bits for the same state.
  DBuf<double> lent;
  double* list_words(int ncomp) {
    const size_t need = (size_t)ncomp * (size_t)std::max<int64_t>(nbent, 1);
    if (lent.n < need) lent.alloc(need + need / 2);
    HIPCHK(hipMemsetAsync(lent.p, 0, need * sizeof(double), stream));
    return lent.p;
  }
  void launch_list_sums(int ncomp, const double* val, double* out) {
    const int nl = (int)top.lists.size(), nt = nglob > 0 ? nglob : (int)top.n;
    if (nl > 0) hipLaunchKernelGGL(k_list_sums, dim3(nl * ncomp), dim3(256), 0, stream, (const int*)(bstart.p + nt), ncomp, (const BondedEntry*)bent.p, (const BondedParam*)bpar.p, val, out);
  }
  // every particle walks its own entries: forces added into fdst, ENERGY: and the lists' energies into elist (observe())
  template <bool ENERGY> void launch_bonded_each(BondedKind kind, V4* fdst) {
    double* const words = ENERGY ? list_words(1) : elist.p;
    auto each = [&](auto kern, const auto&... packs) {
      hipLaunchKernelGGL(kern, dim3(cdiv(n, 256)), dim3(256), 0, stream, G, n, x4.p, fdst, tag.p, rtag.p, bstart.p, bent.p, bpar.p, boxd, words, ctl.p, btab_view(), packs...);
    };
    launch_bonded_kind(kind, each, &k_bonded<R, ENERGY>, &k_bonded_hyb<R, ENERGY>, &k_bonded_q<R, ENERGY>);
    if (ENERGY) launch_list_sums(1, words, elist.p);
  }
  // the first `nown` owners of the work list, forces added into f4
  template <bool BONDS_ONLY> void launch_bonded_work(BondedKind kind, int nown, int guard) {
    auto work = [&](auto kern, const auto&... packs) {
      hipLaunchKernelGGL(kern, dim3(cdiv(nown, 256)), dim3(256), 0, stream, x4.p, f4.p, bwork.p, bj.p, bent.p, bpar.p, boxd, ctl.p, guard, btab_view(), packs...);
    };
    launch_bonded_kind(kind, work, &k_bonded_work<R, BONDS_ONLY>, &k_bonded_work_hyb<R, BONDS_ONLY>, &k_bonded_work_q<R, BONDS_ONLY>, (const int*)tag.p);
  }

  LangevinP<R> lang_params(int64_t istep, int phase) const {
    LangevinP<R> lp{};
    lp.on = lang ? 1 : 0; lp.kT = kT; lp.gamma = gamma; lp.dt = dt; lp.seed = lang_seed; lp.tmask = lang_tmask; lp.step = (uint64_t)istep; lp.phase = (uint32_t)phase;
    return lp;
  }

  template <int MODE> void launch_integrate(bool with_lang, bool storef, int64_t istep, int phase) {
    const int nb = cdiv(n, kIntPerBlock);
    LangevinP<R> lp = lang_params(istep, phase);
    // CapForce acts on the freshly evaluated conservative force: every launch that applies the thermostat
    // consumes exactly that; without a thermostat f4 is never overwritten, so every launch does.
    const R cap = (cap_force > 0 && (with_lang || !lang)) ? (R)cap_force : (R)0;
    if constexpr (MODE == 1 || MODE == 2) {
      if (piston_on()) {      // Langevin piston: the two half steps carry the factors of the step (the fused integrate is off then)
        const PistonP<R> pp{(R)pist_sv, (R)(1.0 / std::sqrt(pist_mu))};
        const auto kern = with_lang ? (storef ? &k_integrate<R, MODE, true, true, true> : &k_integrate<R, MODE, true, false, true>) : &k_integrate<R, MODE, false, false, true>;
        hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, stream, n, x4.p + G, v4.p + G, f4.p + G, tag.p + G, (R)dt, lp, blockmax.p, opt_criterion ? x0.p + G : (const V4*)nullptr, cap, pos_scale(), (const DevCtl*)ctl.p, fold_arg(), pp);
        return;
      }
    }
    const auto kern = with_lang ? (storef ? &k_integrate<R, MODE, true, true> : &k_integrate<R, MODE, true, false>) : &k_integrate<R, MODE, false, false>;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, stream, n, x4.p + G, v4.p + G, f4.p + G, tag.p + G, (R)dt, lp, blockmax.p, opt_criterion ? x0.p + G : (const V4*)nullptr, cap, pos_scale(), (const DevCtl*)ctl.p, fold_arg(), PistonP<R>{});
  }

  void check_flags() {
    DevCtl h = read_ctl();
    if (use_fused && getenv("CHEM_FUSED_STAMPS")) {   // phase boundaries of the last rebuild, 100 MHz ticks
      GridBar g; HIPCHK(hipMemcpy(&g, gbar.p, sizeof(GridBar), hipMemcpyDeviceToHost));
      fprintf(stderr, "[fused] bin %.1f scan %.1f place %.1f sort %.1f desc %.1f list %.1f us\n", (g.stamp[1] - g.stamp[0]) * 0.01, (g.stamp[2] - g.stamp[1]) * 0.01,
              (g.stamp[3] - g.stamp[2]) * 0.01, (g.stamp[4] - g.stamp[3]) * 0.01, (g.stamp[5] - g.stamp[4]) * 0.01, (g.stamp[6] - g.stamp[5]) * 0.01);
    }
    if (dd_on) agree_flags(h);
    tm.rebuilds = tm_base_rebuilds + h.ref_rebuilds + (dd_on ? dd_direct_rebuilds : 0);   // the reference rule's count (== the list builds unless a wider list skin is in use)
    tm.list_rebuilds = dd_on ? dd_rebuilds : tm_base_list_rebuilds + h.rebuild_count;
    if (h.mig_error) throw ChemError(CHEM_ESTATE, "domain decomposition: particle migration error " + std::to_string(h.mig_error));
    if (h.bonded_missing) throw ChemError(CHEM_ESTATE, "domain decomposition: a bonded partner is farther than the ghost layer (rc+skin)");
    if (h.stage_overflow) throw ChemError(CHEM_ENOSPC, "cell stencil exceeded the LDS tile capacity (" + std::to_string(h.stage_overflow) + " particles)");
    if (h.nl_overflow) throw ChemError(CHEM_ENOSPC, "neighbour row overflow during run: needed " + std::to_string(h.nl_overflow) + ", capacity " + std::to_string(S) + " (chem_set_nlist_capacity)");
    if (h.skin_violation) throw ChemError(CHEM_ESTATE, "internal: neighbour list used past skin/2");
    if (h.excl_slot_error) throw ChemError(CHEM_ESTATE, "internal: list build could not locate an excluded partner in its cell");
    if (h.bond_slot_miss) throw ChemError(CHEM_ESTATE, "internal: inline bonds enabled for a system with a bonded partner outside the located exclusions (set option bonds_inline=0)");
    if (h.barrier_timeout) throw ChemError(CHEM_ESTATE, "fused rebuild: grid barrier timed out (device shared with another job?); set option fused_rebuild=0");
    if (h.bucket_overflow) throw ChemError(CHEM_ENOSPC, "a cell filled up with " + std::to_string(h.bucket_overflow) + " particles during the run (fused rebuild bucket rows hold " + std::to_string(bcap) + "); set option fused_rebuild=0");
    if (h.cand_overflow) throw ChemError(CHEM_ENOSPC, "reaction candidate buffer overflow");
  }

  // one step's neighbour bookkeeping in slab mode: cross-rank max of the displacement, the ghost
  // position update (posted before the decision is known: it is needed unless we rebuild), and the
  // collective rebuild when the trigger fired.  One host synchronisation per step.
  int ntxy() const { return tiles_per_layer(box.nc[0], box.nc[1], box.xs_nb, box.xs_w); }      // tiles of one tile layer
  bool dd_overlap() const { return halo_overlap(opt_overlap, use_tiles, ntiles, ntxy(), !g_dd_nopoll); }
  // decision by the force kernel's workgroups instead of a one-block launch between the halo exchange and the forces
  bool dd_merged() const { return dd_on && opt_dd_merge && use_tiles && !dd_overlap() && !g_dd_nopoll; }
  void dd_step_sync() {
    ensure_hflag();
    if (dd_merged()) {
      const bool fold = fold_on();
      if (fold) {
        // the integrate kernel has folded the block maxima into foldmax with atomics: the words travel with the halo, no fold launch
        tr->exchange_with_scalar(halo_msg(), lower, upper, reinterpret_cast<const double*>(foldmax.p), dd_vals.p, stream, kFoldSlots);
      } else {
        hipLaunchKernelGGL(k_rebuild_decide<R>, dim3(1), dim3(1024), 0, stream, ctl.p, blockmax.p, cdiv(acap(), kIntPerBlock), 0.5 * skin_eff(), opt_criterion, 1,
                           (const double*)nullptr, 0, (volatile int*)nullptr, 0, 0.5 * skin);
        tr->exchange_with_scalar(halo_msg(), lower, upper, &ctl.p->step_m2, dd_vals.p, stream);
      }
      const int ticket = ++hticket;
      pair_da = DecideArgs{dd_vals.p, P, (volatile int*)hflag_dev, ticket, dd_par, opt_criterion, 0.5 * skin, fold ? foldmax.p : nullptr, nullptr, 0, 0};
      dd_par ^= 1;
      compute_forces(true, 0);     // (guard 2: decision in the prologue of the force kernel)
      pair_da = DecideArgs{};
      volatile int* hf = hflag;
      poll_ticket(hflag + 1, ticket, "rebuild decision");
      if (hf[0]) { rebuild_dd(); compute_forces(); }
      return;
    }
    // local fold -> ctl->step_m2; its all-to-all rides in the halo exchange group; decision from the
    // P gathered values, mirrored into pinned host memory so that the host learns it by polling one
    // word (no memcpy, no stream synchronisation call)
    hipLaunchKernelGGL(k_rebuild_decide<R>, dim3(1), dim3(1024), 0, stream, ctl.p, blockmax.p, cdiv(acap(), kIntPerBlock), 0.5 * skin_eff(), opt_criterion, 1,
                       (const double*)nullptr, 0, (volatile int*)nullptr, 0, 0.5 * skin);
    // Overlap: the halo exchange runs on the communication stream while the tiles that need no ghost
    // (every tile layer but the lowest and the highest of the slab) already compute their forces.
    // Those launches cannot know the decision yet; if it is "rebuild", everything is recomputed below.
    // (when it pays: chem_geom_host.hpp halo_overlap)
    const bool overlap = dd_overlap();
    hipStream_t xs = stream;
    if (overlap) {
      if (!cstream) {
        HIPCHK(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ev_fold, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ev_halo, hipEventDisableTiming));
      }
      HIPCHK(hipEventRecord(ev_fold, stream));
      HIPCHK(hipStreamWaitEvent(cstream, ev_fold, 0));
      xs = cstream;
    }
    tr->exchange_with_scalar(halo_msg(), lower, upper, &ctl.p->step_m2, dd_vals.p, xs);
    if (overlap) {
      HIPCHK(hipEventRecord(ev_halo, cstream));
      compute_forces(false, 1);                    // interior tiles, main stream, concurrent with the exchange
      HIPCHK(hipStreamWaitEvent(stream, ev_halo, 0));
    }
    const int ticket = ++hticket;
    hipLaunchKernelGGL(k_rebuild_decide<R>, dim3(1), dim3(1024), 0, stream, ctl.p, blockmax.p, 0, 0.5 * skin_eff(), opt_criterion, 2,
                       dd_vals.p, P, (volatile int*)hflag_dev, ticket, 0.5 * skin);
    // The force kernels are enqueued BEFORE the host looks at the decision: they leave at once when a
    // rebuild is pending (then the host rebuilds and launches them again), otherwise the device never
    // waits for the host's poll + launch latency.
    compute_forces(true, overlap ? 2 : 0);
    if (g_dd_nopoll) { DevCtl hc = read_ctl(); if (hc.need_rebuild) { rebuild_dd(); compute_forces(); } return; }
    volatile int* hf = hflag;
    poll_ticket(hflag + 1, ticket, "rebuild decision");
    if (hf[0]) { rebuild_dd(); compute_forces(); }
  }

  // Berendsen / Isokinetic: scale factor from the global kinetic energy, then one streaming pass over v
  DBuf<double> resc_buf;   // [0] Ekin (local, then global), [1] lambda
  void rescale_velocities() {
    const int nkb = cdiv(n, 256);
    resc_buf.alloc(2);
    hipLaunchKernelGGL(k_kinetic<R>, dim3(nkb), dim3(256), 0, stream, G, n, v4.p, ekout.p);
    const bool multi = dd_on && P > 1;
    hipLaunchKernelGGL(k_rescale_lambda, dim3(1), dim3(256), 0, stream, ekout.p, nkb, resc_buf.p, multi ? (double*)nullptr : resc_buf.p + 1,
                       resc_kind, resc_kT, dt / resc_param, (double)nglob, svr_seed, (uint64_t)step);
    if (multi) {
      tr->allreduce_sum_f64(resc_buf.p, 1, stream);
      hipLaunchKernelGGL(k_rescale_lambda, dim3(1), dim3(256), 0, stream, ekout.p, 0, resc_buf.p, resc_buf.p + 1, resc_kind, resc_kT, dt / resc_param, (double)nglob, svr_seed, (uint64_t)step);
    }
    hipLaunchKernelGGL(k_scale_v<R>, dim3(nkb), dim3(256), 0, stream, G, n, v4.p, resc_buf.p + 1, (const DevCtl*)ctl.p);
  }

  // ---- pressure (chem_get_pressure) and Berendsen barostat (chem_barostat_berendsen); the rules: chem_baro_host.hpp ----
  DBuf<double> vlist, vpart, baro_buf;   // bonded virial per list / per block; k_baro_mu's results
  double* baro_pin = nullptr;            // pinned host words the step's (P, mu, mu^3, ...) are copied into
  int launch_bonded_virial(bool per_list = true) {      // returns the number of block partials in vpart; per_list: the sums by list too
    const int nbv = cdiv(n, 256);
    if (vpart.n < (size_t)nbv) vpart.alloc((size_t)nbv + 64);
    if (per_list) { vlist.alloc(CHEM_MAX_LISTS); HIPCHK(hipMemsetAsync(vlist.p, 0, sizeof(double) * CHEM_MAX_LISTS, stream)); }
    double* const words = per_list ? list_words(1) : nullptr;
    hipLaunchKernelGGL((k_bonded_virial<R>), dim3(nbv), dim3(256), 0, stream, G, n, x4.p, tag.p, rtag.p, bstart.p, bent.p, bpar.p, boxd, words, vpart.p,
                       ctl.p, btab_view(), hybrid_args(), (const R*)qtag.p);
    if (per_list) launch_list_sums(1, words, vlist.p);
    return nbv;
  }
  void pressure(chem_pressure* out) override {
    chem_obs ob;
    observe(&ob);      // kinetic sum and non-bonded virial (summed over the ranks of a decomposition)
    std::memset(out, 0, sizeof(*out));
    std::vector<double> hv(CHEM_MAX_LISTS, 0.0);
    if (nbent > 0 && n > 0) { launch_bonded_virial(); vlist.download(hv, CHEM_MAX_LISTS, stream); }
    allreduce_host_sums(hv.data(), CHEM_MAX_LISTS, redbuf);
    out->volume = L[0] * L[1] * L[2]; out->mv2 = 2.0 * ob.ekin; out->virial_nb = ob.virial_nb;
    double w = ob.virial_nb;
    for (size_t l = 0; l < top.lists.size(); ++l) { out->virial_list[l] = hv[l]; w += hv[l]; }
    out->virial = w;
    out->pressure = baro_pressure(out->mv2, w, out->volume);
  }

  // ---- radial distribution functions (chem_rdf_*; the rules and the launch plan: chem_rdf_host.hpp, the kernels: md_kernels.hpp) ----
  DBuf<unsigned long long> rdf_acc;      // frames, pairs[8], density[8] (bits of doubles), type counts of the frame in flight, then the histograms from word kRdfHead on
  int rdf_ncu = 0; size_t rdf_lds_set[2] = {0, 0};
  // Slabs: every rank accumulates the pairs its home particles own (k_rdf_tiles takes a pair from its lower tag among the home
  // particles, so a pair with a ghost member is counted by one owner) and a frame adds no communication.  The type counts of M
  // have to be global, and the device holds types by slot of the owned particles only: the books (frames, pairs, density) are
  // kept here on the host from top.type, which is replicated by tag -- the same on every rank.  chem_rdf_get sums the histograms.
  uint64_t rdf_h_frames = 0, rdf_h_pairs[CHEM_RDF_MAX_PAIRS] = {}; double rdf_h_density[CHEM_RDF_MAX_PAIRS] = {};
  DBuf<double> rdf_red;
  size_t rdf_words() const { return rdf_hist_words(rdf.nbins, rdf.npairs, rdf.split ? 2 : 1); }
  void rdf_configure() override {
    if (!rdf.on) { if (rdf_acc.p) { HIPCHK(hipStreamSynchronize(stream)); rdf_acc.free(); rdf_red.free(); } return; }
    rdf_acc.alloc((size_t)kRdfHead + rdf_words());
    rdf_reset();
  }
  void rdf_reset() override {
    HIPCHK(hipMemsetAsync(rdf_acc.p, 0, sizeof(unsigned long long) * ((size_t)kRdfHead + rdf_words()), stream));
    rdf_h_frames = 0;
    for (int s = 0; s < CHEM_RDF_MAX_PAIRS; ++s) { rdf_h_pairs[s] = 0; rdf_h_density[s] = 0.0; }
  }
  RdfArgs rdf_args() const {
    RdfArgs a{};
    a.dr = rdf.r_max / (double)rdf.nbins; a.inv_dr = 1.0 / a.dr;
    a.nbins = rdf.nbins; a.nsel = rdf.npairs; a.parts = rdf.split ? 2 : 1;
    rdf_fill_masks(rdf.npairs, rdf.tp, a.mask);
    return a;
  }
  // what a frame needs of the set-up (asked where chem_run starts and at every frame: the cutoff can be set after chem_rdf_init,
  // and the tile capacity can grow); the kernel is told its LDS here, so that a frame inside a run is launches and nothing else
  // while the tile capacity stays what it was when the run started (a larger one sets the attribute once more)
  RdfPlan rdf_plan_now() {
    // (a decomposed context is always on the tile path: plan_tiles refuses a slab without it)
    if (rdf.r_max > rc) throw ChemError(CHEM_EINVAL, "rdf: r_max = " + std::to_string(rdf.r_max) + " exceeds the list cutoff max_cutoff = " + std::to_string(rc) +
                                                     " (the lists of the last build hold nothing beyond it)");
    if (!rdf_ncu) { hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device)); rdf_ncu = prop.multiProcessorCount; }
    RdfPlan pl{}; std::string why;
    const int path = use_tiles ? 0 : 1;
    if (!rdf_plan(path, rdf.nbins, rdf.npairs, rdf.split ? 2 : 1, use_tiles ? tile_lds_bytes() : 0, kTileLdsBudget, rdf_ncu, use_tiles ? ntiles : n, pl, why))
      throw ChemError(CHEM_EINVAL, why);
    if (rdf_lds_set[path] < pl.lds_bytes) {
      const void* fn = use_tiles ? reinterpret_cast<const void*>(&k_rdf_tiles<R, 512>) : reinterpret_cast<const void*>(&k_rdf_all<R>);
      HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
      rdf_lds_set[path] = pl.lds_bytes;
    }
    return pl;
  }
  // one frame of the positions as they are, behind whatever the stream holds (the forces of the step): pair pass, then the books.
  // (Slabs: dd_step_sync has returned, so the host knows the step's decision, a rebuild it asked for has happened, the ghost
  //  positions are those the forces were evaluated at and nothing of the step is speculative any more.)
  void rdf_launch() {
    const RdfPlan pl = rdf_plan_now();
    if ((rdf.split || dd_on) && (labels_pending || label_thr.joinable())) join_thread();      // the labels the reaction scan of this step would read
    const RdfArgs a = rdf_args();
    if (n > 0) {
      if (use_tiles)
        hipLaunchKernelGGL((k_rdf_tiles<R, 512>), dim3(pl.grid), dim3(pl.block), pl.lds_bytes, stream, ntiles, tile_cap, x4.p, tag.p, tdesc.p, mol_id.p, boxd, a,
                           (int)pl.hist_off, rdf_acc.p, (const DevCtl*)ctl.p, (R)(0.5 * skin_eff()));
      else
        hipLaunchKernelGGL(k_rdf_all<R>, dim3(pl.grid), dim3(pl.block), pl.lds_bytes, stream, n, x4.p + G, tag.p + G, mol_id.p, boxd, a, (int)pl.hist_off, rdf_acc.p,
                           (const DevCtl*)ctl.p);
    }
    const double V = L[0] * L[1] * L[2];
    if (dd_on) {
      sync_type_mirrors();
      long long c[CHEM_MAX_TYPES] = {};
      for (int64_t t = 0; t < top.n; ++t) ++c[top.type[(size_t)t] & (CHEM_MAX_TYPES - 1)];
      ++rdf_h_frames;
      for (int s = 0; s < rdf.npairs; ++s) { const unsigned long long M = rdf_norm_pairs(a.mask, s, c); rdf_h_pairs[s] += M; rdf_h_density[s] += (double)M / V; }
    } else {
      if (n > 0) hipLaunchKernelGGL(k_rdf_count<R>, dim3(std::min(cdiv(n, 256), 4 * rdf_ncu)), dim3(256), 0, stream, G, n, x4.p, rdf_acc.p, (const DevCtl*)ctl.p);
      hipLaunchKernelGGL(k_rdf_frame, dim3(1), dim3(64), 0, stream, a, V, rdf_acc.p, (const DevCtl*)ctl.p);
    }
    HIPCHK(hipGetLastError());
  }
  void rdf_sample() override {      // chem_observe's preconditions
    flush_host_state();
    if (resort) { rebuild_now(); compute_forces(); }
    rdf_launch();
  }
  void rdf_get(chem_rdf_result* out, uint64_t* counts, int64_t cap) override {      // collective on a decomposed context, like chem_get_pressure
    const size_t nw = rdf_words();
    if (counts && cap < (int64_t)nw) throw ChemError(CHEM_ENOSPC, "rdf_get: capacity " + std::to_string(cap) + " below npairs * (1 + split) * nbins = " + std::to_string(nw));
    std::vector<unsigned long long> h;
    const bool hist = counts || (dd_on && P > 1);      // (every rank takes part in the sum, whatever it asked for)
    rdf_acc.download(h, hist ? (size_t)kRdfHead + nw : (size_t)kRdfHead, stream);
    if (dd_on && P > 1) {
      // the counts are integers far below 2^53: their sum as doubles is exact
      std::vector<double> d(nw);
      for (size_t k = 0; k < nw; ++k) d[k] = (double)h[kRdfHead + k];
      allreduce_host_sums(d.data(), (int)nw, rdf_red);
      for (size_t k = 0; k < nw; ++k) h[kRdfHead + k] = (unsigned long long)d[k];
    }
    std::memset(out, 0, sizeof(*out));
    out->r_max = rdf.r_max; out->nbins = rdf.nbins; out->npairs = rdf.npairs; out->split = rdf.split ? 1 : 0;
    if (dd_on) {
      out->frames = (int64_t)rdf_h_frames;
      for (int s = 0; s < rdf.npairs; ++s) { out->pairs[s] = rdf_h_pairs[s]; out->density[s] = rdf_h_density[s]; }
    } else {
      out->frames = (int64_t)h[kRdfFrames];
      for (int s = 0; s < rdf.npairs; ++s) { out->pairs[s] = h[kRdfPairs + s]; std::memcpy(&out->density[s], &h[kRdfDensity + s], sizeof(double)); }
    }
    if (counts) for (size_t k = 0; k < nw; ++k) counts[k] = h[kRdfHead + k];
  }

  // ---- static structure factor (chem_sq_*; the rules and the launch plan: chem_sq_host.hpp, the kernels: md_kernels.hpp) ----
  static_assert(kSqTypes == kRdfTypes, "k_rdf_count leaves the type counts where k_sq_accum reads them");
  DBuf<double> sq_acc, sq_part, sq_rho;      // frames, na, nb, box_sum, type counts of the frame in flight, then the sums from word kSqHead on; partials; rho
  int sq_ncu = 0; size_t sq_lds_set = 0;
  double sq_h_frames = 0, sq_h_na[CHEM_SQ_MAX_PAIRS] = {}, sq_h_nb[CHEM_SQ_MAX_PAIRS] = {}, sq_h_box[3] = {};      // the books of a decomposed context (host)
  SqArgs sq_a{};
  size_t sq_words() const { return (size_t)sq.npairs * (size_t)sq_nvec(sq.nmax); }
  void sq_configure() override {
    if (!sq.on) { if (sq_acc.p) { HIPCHK(hipStreamSynchronize(stream)); sq_acc.free(); sq_part.free(); sq_rho.free(); } return; }
    sq_fill_classes(sq.nmax, sq.npairs, sq.tp, sq_a);
    if (sq_acc.p) HIPCHK(hipStreamSynchronize(stream));      // (a smaller configuration before: its frames may still be running)
    sq_acc.free(); sq_part.free(); sq_rho.free();
    sq_acc.alloc((size_t)kSqHead + sq_words());
    sq_rho.alloc((size_t)sq_a.ncls * sq_a.nvec * 2);
    sq_reset();
  }
  void sq_reset() override {
    HIPCHK(hipMemsetAsync(sq_acc.p, 0, sizeof(double) * ((size_t)kSqHead + sq_words()), stream));
    sq_h_frames = 0;
    for (int s = 0; s < CHEM_SQ_MAX_PAIRS; ++s) { sq_h_na[s] = 0.0; sq_h_nb[s] = 0.0; }
    for (int d = 0; d < 3; ++d) sq_h_box[d] = 0.0;
  }
  // the plan of a frame of n home particles (asked where chem_run starts and at every frame); the scratch is allocated for the most
  // super-chunks any n gets and the kernel is told its LDS here, so that a frame inside a run is launches and nothing else
  SqPlan sq_plan_now() {
    if (!sq_ncu) { hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, device)); sq_ncu = prop.multiProcessorCount; }
    SqPlan pl{}; std::string why;
    if (!sq_plan(n > 0 ? n : 1, sq.nmax, sq_a.ncls, kTileLdsBudget, sq_ncu, pl, why)) throw ChemError(CHEM_EINVAL, why);
    sq_part.alloc((size_t)sq_super_cap(sq.nmax, sq_a.ncls, sq_ncu) * sq_partial_bytes(sq.nmax, sq_a.ncls) / sizeof(double));
    if (sq_lds_set < pl.lds_bytes) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sq_walk<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
      sq_lds_set = pl.lds_bytes;
    }
    return pl;
  }
  // one frame of the positions as they are, behind whatever the stream holds (the forces of the step): the home slots x4[G .. G + n)
  // on every path.  (Slabs: as for rdf_launch, dd_step_sync has returned; the all-reduce is the transport's, on this stream.)
  void sq_launch() {
    const SqPlan pl = sq_plan_now();
    const SqArgs& a = sq_a;
    const size_t rw = (size_t)a.ncls * a.nvec;
    if (n > 0) {
      hipLaunchKernelGGL(k_sq_walk<R>, dim3(pl.nqb, pl.nsuper), dim3(pl.block), pl.lds_bytes, stream, G, n, x4.p, boxd, a, pl.per, sq_part.p, (const DevCtl*)ctl.p);
      hipLaunchKernelGGL(k_sq_reduce, dim3(cdiv((long long)rw, 256)), dim3(256), 0, stream, a, pl.nsuper, (const double*)sq_part.p, sq_rho.p, (const DevCtl*)ctl.p);
    } else {
      HIPCHK(hipMemsetAsync(sq_rho.p, 0, sizeof(double) * 2 * rw, stream));
    }
    if (dd_on) {
      if (P > 1) tr->allreduce_sum_f64(sq_rho.p, 2 * rw, stream);
      sync_type_mirrors();
      long long c[CHEM_MAX_TYPES] = {};
      for (int64_t t = 0; t < top.n; ++t) ++c[top.type[(size_t)t] & (CHEM_MAX_TYPES - 1)];
      sq_h_frames += 1.0;
      for (int s = 0; s < sq.npairs; ++s) { sq_h_na[s] += (double)sq_class_count(a, a.sel_a[s], c); sq_h_nb[s] += (double)sq_class_count(a, a.sel_b[s], c); }
      for (int d = 0; d < 3; ++d) sq_h_box[d] += L[d];
    } else if (n > 0) {
      hipLaunchKernelGGL(k_rdf_count<R>, dim3(std::min(cdiv(n, 256), 4 * sq_ncu)), dim3(256), 0, stream, G, n, x4.p, reinterpret_cast<unsigned long long*>(sq_acc.p), (const DevCtl*)ctl.p);
    }
    hipLaunchKernelGGL(k_sq_accum, dim3(cdiv(a.nvec, 256)), dim3(256), 0, stream, a, boxd, dd_on ? 0 : 1, (const double*)sq_rho.p, sq_acc.p, (const DevCtl*)ctl.p);
    HIPCHK(hipGetLastError());
  }
  void sq_sample() override {      // chem_observe's preconditions
    flush_host_state();
    if (resort) { rebuild_now(); compute_forces(); }
    sq_launch();
  }
  // `frames` frames of the current state back to back between two events on the context's stream: milliseconds per frame
  // (tools/sq_workload.py; the frames are accumulated like any other)
  double sq_time_frames(int frames) override {
    flush_host_state();
    if (resort) { rebuild_now(); compute_forces(); }
    (void)sq_plan_now();
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, stream));
    for (int k = 0; k < frames; ++k) sq_launch();
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return (double)ms / (double)(frames > 0 ? frames : 1);
  }
  void sq_get(chem_sq_result* out, double* sums, int64_t cap) override {
    const size_t nw = sq_words();
    if (sums && cap < (int64_t)nw) throw ChemError(CHEM_ENOSPC, "sq_get: capacity " + std::to_string(cap) + " below npairs * nvec = " + std::to_string(nw));
    std::vector<double> h;
    sq_acc.download(h, sums ? (size_t)kSqHead + nw : (size_t)kSqHead, stream);
    std::memset(out, 0, sizeof(*out));
    out->nmax = sq.nmax; out->npairs = sq.npairs; out->nvec = sq_nvec(sq.nmax);
    const double* const fr = dd_on ? &sq_h_frames : &h[kSqFrames];
    const double* const na = dd_on ? sq_h_na : &h[kSqNa]; const double* const nb = dd_on ? sq_h_nb : &h[kSqNb]; const double* const bx = dd_on ? sq_h_box : &h[kSqBox];
    out->frames = (int64_t)*fr;
    for (int s = 0; s < sq.npairs; ++s) { out->na[s] = na[s]; out->nb[s] = nb[s]; }
    for (int d = 0; d < 3; ++d) out->box_sum[d] = bx[d];
    if (sums) for (size_t k = 0; k < nw; ++k) sums[k] = h[kSqHead + k];
  }

  // ---- pressure tensor (chem_get_pressure_tensor; the rules: include/chem_mi355.h, the kernel: chem_tensor_host.hpp) ----
  // Everything below is allocated and launched by the call alone.
  DBuf<double> tpart, tredbuf;      // per-list sums, kinetic and pair block partials (one buffer, one download); the ranks' sums
  // the tensor pass over the lists of the step's forces into tpart (six words per block); returns the number of blocks.  The
  // arguments are those of launch_pair<true>: fdst is scratch, the excluded pairs of inline bonds are taken out again.
  int launch_pair_tensor(V4* fdst, size_t off) {      // off: where the partials start in tpart
    const double hs = half_skin_eff();
    const TensorPlan plan = tensor_plan(pair_input(true));
    if (plan.code != CHEM_OK) throw ChemError(plan.code, pair_refusal_text(plan.refused));
    const TensorVariant& v = plan.v;
    const int nblk = use_tiles ? ntiles : cdiv((long long)n * v.tpp, v.block);
    if (nblk <= 0) return 0;
    tpart.alloc(off + 6 * (size_t)nblk + 8);
    double* const tout = tpart.p + off;
    HIPCHK(hipMemsetAsync(tout, 0, sizeof(double) * 6 * (size_t)nblk, stream));      // (a halted context's kernels leave at once)
    const CoulArgs<R> ca = v.mode == 4 ? coul_args((size_t)nblk) : CoulArgs<R>{};
    const ResArgs<R> ra = (v.mode == 5 || v.mode == 7) ? res_args() : ResArgs<R>{};
    const CapArgs<R> cp = (v.mode == 6 || v.mode == 7) ? cap_args() : CapArgs<R>{};
    bool found = false;
    if (use_tiles) {
      const int bond_mode = inline_bond_mode();
      const TileSub ts{0, ntiles, 0};
      const size_t lds = pair_lds_bytes();
      found = pick_among<3, 4, 5, 6, 7>(v.mode, [&](auto M_) {
        auto kern = &k_pair_tiles_tensor<R, decltype(M_)::value>;
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(512), lds, stream, nblk, tile_cap, x4.p, fdst, tdesc.p, nl16.p, nnh.p, S, pcore.p, pext.p, ntypes, tab.p, eout.p, hs, ctl.p, ts,
                           (v.mode == 3 && bond_mode >= 2) ? BondRecs{brec0.p, brec1.p} : BondRecs{}, bond_mode, act, ca, ra, cp, tout);
        return true;
      });
    } else {
      found = pick_among<0, 4, 5, 6, 7>(v.mode, [&](auto M_) {
        hipLaunchKernelGGL((k_pair_force_tensor<R, decltype(M_)::value>), dim3(nblk), dim3(256), 0, stream, n, x4.p, fdst, nlist.p, nn.p, S, box, pcore.p, pext.p, ntypes, tab.p, eout.p, hs, ctl.p,
                           ca, ra, cp, tout);
        return true;
      });
    }
    if (!found || !tensor_variant_built(v.family, v.mode, v.tpp, v.block)) throw ChemError(CHEM_ESTATE, "internal: no pressure-tensor kernel is built for the planned variant");
    HIPCHK(hipGetLastError());
    return nblk;
  }
  void pressure_tensor(chem_pressure_tensor* out) override {
    flush_host_state();
    if (resort) { rebuild_now(); compute_forces(); }      // (the route of observe(): a rebuild re-sorts the particles but not f4)
    std::memset(out, 0, sizeof(*out));
    constexpr int kParts = 2 + CHEM_MAX_LISTS;              // kinetic, non-bonded, the lists
    // one buffer, one download: [per-list sums | kinetic block partials | pair block partials]
    const int nkb = cdiv(n, 256);
    const size_t o_k = 6 * CHEM_MAX_LISTS, o_p = o_k + 6 * (size_t)nkb;
    const int nb = launch_pair_tensor(x4o.p, o_p);          // scratch force buffer: leaves f4 untouched
    const bool bonded = nbent > 0 && nkb > 0;
    tpart.alloc(o_p + 8);                                   // (launch_pair_tensor has sized it where there are pairs)
    HIPCHK(hipMemsetAsync(tpart.p, 0, sizeof(double) * 6 * CHEM_MAX_LISTS, stream));
    if (nkb > 0) hipLaunchKernelGGL(k_kinetic_tensor<R>, dim3(nkb), dim3(256), 0, stream, G, n, v4.p, tpart.p + o_k);
    if (bonded) {
      double* const words = list_words(6);
      hipLaunchKernelGGL((k_bonded_virial_tensor<R>), dim3(nkb), dim3(256), 0, stream, G, n, x4.p, tag.p, rtag.p, bstart.p, bent.p, bpar.p, boxd, words,
                         ctl.p, btab_view(), hybrid_args(), (const R*)qtag.p);
      launch_list_sums(6, words, tpart.p);
    }
    std::vector<double> h;
    tpart.download(h, o_p + 6 * (size_t)nb, stream);
    double acc[6 * kParts] = {0};                           // block partials folded in block order
    for (int b = 0; b < nkb; ++b) for (int c = 0; c < 6; ++c) acc[c] += h[o_k + 6 * (size_t)b + c];
    for (int b = 0; b < nb; ++b) for (int c = 0; c < 6; ++c) acc[6 + c] += h[o_p + 6 * (size_t)b + c];
    for (int k = 0; k < 6 * CHEM_MAX_LISTS; ++k) acc[12 + k] = h[k];
    allreduce_host_sums(acc, 6 * kParts, tredbuf);      // one all-reduce of the 6 + 6 + 6 * CHEM_MAX_LISTS sums
    out->volume = L[0] * L[1] * L[2];
    for (int c = 0; c < 6; ++c) {
      out->kinetic[c] = acc[c]; out->virial_nb[c] = acc[6 + c];
      double w = acc[6 + c];
      for (size_t l = 0; l < top.lists.size(); ++l) { out->virial_list[l][c] = acc[12 + 6 * l + c]; w += acc[12 + 6 * l + c]; }
      out->virial[c] = w;
      out->tensor[c] = (acc[c] + w) / out->volume;
    }
  }
  // the box lengths alone changed (same cell grid, same plan): everything the kernels take by value
  void refresh_box_lengths() {
    for (int d = 0; d < 3; ++d) {
      box.L[d] = (R)L[d]; box.invL[d] = (R)(1.0 / L[d]);
      box.cell_inv[d] = (R)((box.nc[0] > 0 ? box.nc[d] : 1) / L[d]);
      boxd.L[d] = L[d]; boxd.invL[d] = 1.0 / L[d];
      box.qs[d] = boxd.qs[d] = q_scale(d); box.qh[d] = boxd.qh[d] = 0.5 * L[d];
      box.qsf[d] = (R)q_scale(d); box.qinvf[d] = (R)(1.0 / q_scale(d));
    }
  }
  bool baro_replan_pending = false;      // geom_dirty was raised by a scaling, not by the caller: the forces in f4 stay valid
  // One barostat action has two halves.
  // baro_measure(), behind the second half kick (and the velocity rescaling) of the step that has just been counted: P from the
  // positions and velocities of this step and the virial of its force evaluation (the energy instantiation over the same lists: a
  // second pair pass), the rule on the device (Berendsen: mu; Langevin piston: the kick of the momentum kept on the device and the
  // factors of the next step), the results copied into pinned words.  One host synchronisation of its own (on the fused path the
  // run loop's look at the control block in front of it, for a stop by the device, is a second).  Returns mu.
  // baro_apply(mu, mu_dev): the box, the fp64 positions, what the device keeps in absolute length, the charge to the lists and the
  // re-plan.  Berendsen calls it at once; the piston behind the next step's drift, in front of launch_fix and the rebuild decision.
  static constexpr int kBaroWords = 16, kPistonPe = 8;      // words of baro_buf; the piston momentum's place in it
  int launch_baro_partials(int& nbv, int& nkb) {
    const int nb = launch_pair<true>(x4o.p);      // (scratch force buffer: f4 keeps the step's forces)
    nbv = nbent > 0 ? launch_bonded_virial(false) : 0;
    nkb = cdiv(n, 256);
    hipLaunchKernelGGL(k_kinetic<R>, dim3(nkb), dim3(256), 0, stream, G, n, v4.p, ekout.p);
    baro_buf.alloc(kBaroWords);
    if (!baro_pin) HIPCHK(hipHostMalloc((void**)&baro_pin, 8 * sizeof(double), hipHostMallocDefault));
    return nb;
  }
  double baro_measure() {
    int nbv, nkb;
    const int nb = launch_baro_partials(nbv, nkb);
    const bool cq = coul_on();
    double* h = baro_pin;
    if (piston_on()) {
      if (pist_pe_upload) { HIPCHK(hipMemcpyAsync(baro_buf.p + kPistonPe, &pist_pe, sizeof(double), hipMemcpyHostToDevice, stream)); pist_pe_upload = false; }
      hipLaunchKernelGGL(k_baro_piston, dim3(1), dim3(256), 0, stream, (const double*)ekout.p, nkb, (const double*)eout.p, nb, cq ? (const double*)eoutq.p : (const double*)nullptr, cq ? nb : 0,
                         (const double*)vpart.p, nbv, L[0] * L[1] * L[2], dt, baro_p0, pist_w, pist_gamma, pist_kT, 3.0 * (double)n, pist_seed, (uint64_t)step, baro_buf.p + kPistonPe, baro_buf.p);
      HIPCHK(hipMemcpyAsync(h, baro_buf.p, 8 * sizeof(double), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      baro_p_last = h[0];
      const double sv = piston_sv(h[1], pist_w, 3.0 * (double)n, dt), mu = piston_mu(h[1], pist_w, dt);
      if (!piston_ok(h[1], mu, sv)) {
        char msg[320];
        snprintf(msg, sizeof(msg), "Langevin barostat: piston momentum pe = %.6g (mu = %.6g, sv = %.6g) at step %lld (P = %.6g, P0 = %.6g, mass = %.6g): the box cannot follow; use a larger mass",
                 h[1], mu, sv, (long long)step, h[0], baro_p0, pist_w);
        pist_pe = h[1];
        throw ChemError(CHEM_ESTATE, msg);
      }
      pist_pe = h[1]; pist_eps = h[2]; pist_sv = h[3]; pist_mu = h[4];
      return pist_mu;
    }
    hipLaunchKernelGGL(k_baro_mu, dim3(1), dim3(256), 0, stream, (const double*)ekout.p, nkb, (const double*)eout.p, nb, cq ? (const double*)eoutq.p : (const double*)nullptr, cq ? nb : 0,
                       (const double*)vpart.p, nbv, L[0] * L[1] * L[2], dt, baro_tau, baro_p0, baro_buf.p);
    HIPCHK(hipMemcpyAsync(h, baro_buf.p, 6 * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    baro_p_last = h[0];
    if (!baro_mu3_ok(h[2])) {
      char msg[256];
      snprintf(msg, sizeof(msg), "Berendsen barostat: mu^3 = %.6g <= 0 at step %lld (P = %.6g, P0 = %.6g, dt/tau = %.6g): the box cannot be scaled; use a larger tau",
               h[2], (long long)step, h[0], baro_p0, dt / baro_tau);
      throw ChemError(CHEM_ESTATE, msg);
    }
    return h[1];
  }
  void baro_apply(double mu, const double* mu_dev) {
    if constexpr (!kFixed) hipLaunchKernelGGL(k_baro_scale_x, dim3(cdiv(n, 256)), dim3(256), 0, stream, n, x4.p, mu_dev, (const DevCtl*)ctl.p);
    for (int d = 0; d < 3; ++d) L[d] *= mu;
    // The box lengths reach every kernel by value from here on; what the device keeps in absolute length follows mu: the
    // reference positions of the displacement criterion (fp64 build) and the length fields of the tile descriptors.
    refresh_box_lengths();
    if constexpr (!kFixed) if (opt_criterion) hipLaunchKernelGGL(k_baro_scale_x, dim3(cdiv(n, 256)), dim3(256), 0, stream, n, x0.p, mu_dev, (const DevCtl*)ctl.p);
    if (use_tiles) hipLaunchKernelGGL((k_baro_tile_desc<R>), dim3(std::min(ntiles, 2048)), dim3(128), 0, stream, ntiles, tile_cap, (const int*)cell_start.p, box, tdesc.p, ctl.p,
                                      (const int*)cell_sub.p, (use_fused && opt_lpt) ? (const int*)tile_pos.p : (const int*)nullptr);
    // The lists stay.  A scaling changes a listed separation by at most |mu - 1| (rc + skin_eff): half of that per particle
    // (baro_list_charge), plus |mu - 1| skin_eff / 2 for the displacement already accumulated, which scales too, is charged
    // as displacement -- taken off the half skin of every later decision, under both criteria, until the device has built lists
    // again (its counters say so).  Where the charge and the distance accumulated so far already exceed the half skin, the
    // lists are built behind the next drift (the piston: behind the drift this scaling belongs to) whatever the device decides.
    const DevCtl hc = read_ctl();
    if (hc.rebuild_count != baro_seen_builds) { baro_charge = 0; baro_seen_builds = hc.rebuild_count; }
    if (hc.ref_rebuilds != baro_seen_ref) { baro_charge_ref = 0; baro_seen_ref = hc.ref_rebuilds; }
    const double c = baro_list_charge(mu, rc, skin_eff()) + 0.5 * std::fabs(mu - 1.0) * skin_eff();
    baro_charge += c; baro_charge_ref += c;
    if (hc.acc_maxdist + baro_charge > 0.5 * skin_eff()) { resort = true; hint_invalidate(); }
    // If the new box asks for another cell grid than the one in force (either direction), the geometry is planned again in
    // front of the list build that follows the next drift; until then the tables of the old plan stay (the reaction work of
    // this step reads them: same particles, same tiles).
    if (baro_replan(L, rc + skin_eff(), box.nc)) {
      if (g_trace) fprintf(stderr, "[chem trace] barostat: box %.6f %.6f %.6f asks for another cell grid at step %lld\n", L[0], L[1], L[2], (long long)step);
      geom_dirty = true; baro_replan_pending = true; resort = true; hint_invalidate();
    }
  }
  void baro_step() { const double mu = baro_measure(); baro_apply(mu, baro_buf.p + 1); }      // Berendsen: both halves back to back

  // Does step `step` get its neighbour launch?  (single domain, fused rebuild; the rule and its reasons: chem_idle_host.hpp)
  // The host enqueues far faster than the device runs, so it first lets the device come within idle_lag steps: it spins on the
  // pinned words, for a bounded time -- nothing on the device ever waits for the host, and a wait that runs out only means one
  // launch more.
  static constexpr double kIdleWaitS = 0.05;
  bool neighbour_launch_wanted() {
    ensure_hflag();
    const IdleHost host{hint_gen, resort, want32 || dbg_on};
    if (host.requested || host.diagnostics) return true;
    if (opt_skip_idle == 2) return false;
    IdleHint h = hint_read();
    if (opt_idle_lag > 0 && step - opt_idle_lag >= hint_gen_step && !idle_hint_fresh(h, hint_gen, step, opt_idle_lag)) {      // (lag 0: no wait, whatever is there)
      const double t0 = now_s();
      for (long long spins = 1;; ++spins) {
        h = hint_read();
        if (idle_hint_fresh(h, hint_gen, step, opt_idle_lag)) break;
        if (h.halted == hint_gen) return true;      // the run has stopped: nothing more will be published
        idle_cpu_pause();
        if ((spins & 1023) == 0 && now_s() - t0 > kIdleWaitS) { ++idle_timeouts; return true; }
      }
    }
    return idle_launch(h, host, step, 0.5 * skin_eff(), opt_idle_kappa);
  }

  // ---- the hot call -------------------------------------------------------------------
  void run(int64_t nsteps) override {
    if (!(dt > 0)) throw ChemError(CHEM_ESTATE, "dt not set");
    if (baro_on() && dd_on) throw ChemError(CHEM_ENOTIMPL, std::string(baro_name()) + " barostat on a decomposed context: a gap of the decomposed path (the box of a slab cannot change)");
    // barostat: the forces of the last run's final step (evaluated before its scaling) are the ones this run starts from,
    // provided nothing has touched the system or re-sorted the particles since
    const bool keep_forces = baro_on() && baro_keep && !(particles_dirty || (geom_dirty && !baro_replan_pending) || labels_dirty || pair_dirty || coul_dirty || res_dirty || cap_dirty || fix_dirty || bonded_dirty || excl_dirty);
    baro_keep = false;
    // region rules: likewise behind a change at the last run's final step (the force list is then built behind the first drift)
    const bool dirty_any = particles_dirty || geom_dirty || labels_dirty || pair_dirty || coul_dirty || res_dirty || cap_dirty || fix_dirty || bonded_dirty || excl_dirty;
    const bool keep_region = region_keep && !baro_on() && !dd_on && !dirty_any && device_ready;
    region_keep = false;
    flush_host_state();
    const bool rdf_due = rdf.on && rdf.every > 0;
    if (rdf_due) (void)rdf_plan_now();      // (refusals before the first step, not in the middle of the run)
    const bool sq_due = sq.on && sq.every > 0;
    if (sq_due) (void)sq_plan_now();        // (scratch and the LDS attribute before the first step)
    hint_invalidate();      // (whatever the last call's launches published: the first step of a call gets its neighbour launch)
    const double t0 = now_s();
    if (opt_time_pair) {
      const size_t want = (size_t)std::min<int64_t>(8 * (nsteps / opt_time_pair + 2), 16384);
      while (ev.size() < want) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
      ev_used = 0; ev_kind.clear();
    }
    timed_step = false;
    if (react_on && !reactions.empty() && pin_ev_cap == 0) {
      // pinned staging for the event download: at most one event per two particles; allocated here so
      // that the first reaction step does not pay ~10 ms for it
      pin_ev_cap = (size_t)top.n / 2 + 1024;
      HIPCHK(hipHostMalloc((void**)&pin_ev, pin_ev_cap * sizeof(Candidate), hipHostMallocDefault));
      {  // the first copy-engine transfer out of a fresh device allocation into a fresh pinned range costs ~7 ms
         // (mappings): pay it here, not in the first reaction step
        alloc_reaction_buffers();
        const size_t bytes = std::min(pin_ev_cap, (size_t)cand_cap) * sizeof(Candidate);
        HIPCHK(hipMemsetAsync(evout.p, 0, bytes, stream));
        HIPCHK(hipMemcpyAsync(pin_ev, evout.p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
      }
    }
    if (react_on && !reactions.empty()) reserve_reaction_tables();
    force_step_off = 0;
    if (!keep_forces && !keep_region) {
      if (resort) rebuild_now();
      compute_forces();
      if (lang) launch_integrate<0>(true, true, step, 0);  // thermalize: f += friction + noise, stored
    }
    bool need_int1 = true;
    const int64_t step0 = step;
    bool run_cut = false;      // region rules next to tracked stamps: the call ends behind a firing that changed something
    const bool regions_on = region_any() && !dd_on;
    bool resume = false;       // re-entering the step at which the device stopped the run (DevCtl::halt)
    // The device may stop an asynchronous run (fused rebuild: a cell outgrew its bucket row).  Every launch behind that
    // point has left at once; the host learns of it at its next synchronisation -- a reaction / ATRP step or the end of
    // the call --, repairs the set-up (wider rows or the unfused chain: rebuild_now) and re-enters the loop at that step.
    int resume_kind = 0, resume_par = 0;       // DevCtl::halt and halt_par of that stop
    int64_t timed_idle_skips = 0;
    auto halted = [&](int64_t& s) -> bool {
      if (!use_fused) return false;
      HIPCHK(hipStreamSynchronize(stream));
      const DevCtl h = read_ctl();
      if (!h.halt) return false;
      s = h.halt_step - step0; step = h.halt_step;
      set_ctl_field(&DevCtl::halt, 0);
      if (h.halt == 4) {
        // a region rule stopped the run behind step halt_step: that step is complete, its forces are stored, nothing of the
        // next one has happened (the launches enqueued behind the stop left at once).  Apply the change and go on from there.
        need_int1 = true; fused_par = h.halt_par & 1;
        skip_log_stop(h.halt_step);
        ++region_syncs;
        region_apply();
        if (res_tracking()) run_cut = true;      // (a stamp set here may create a completion step: the piece ends, chem_run asks afresh)
        return true;
      }
      resort = true; resume = true; need_int1 = false;
      resume_kind = h.halt; resume_par = fused_par = h.halt_par & 1;      // (the launches enqueued behind the stop flipped the host's parity and left at once)
      skip_log_stop(h.halt_step);
      if (h.halt == 2) ++idle_wrong;
      ++halts_recovered;
      if (g_trace) fprintf(stderr, "[chem trace] run stopped by the device at step %lld (bucket rows of %d, tile capacity %d, list rows of %d): recovering\n", (long long)h.halt_step, bcap, tile_cap, S);
      return true;
    };
    for (int64_t s = 0; s < nsteps && !run_cut; ++s) {
      // (a stop the device has already told the pinned words about need not wait for the next synchronisation)
      if (!resume && hflag && (skip_applies() || regions_on) && const_cast<const volatile IdleHint*>(hint_host())->halted == hint_gen && halted(s)) { --s; continue; }
      if (need_int1) {
        launch_integrate<2>(false, false, step, 1);
        // Langevin piston: the box and the drifted positions take the step's mu (computed at the last kick) in front of the
        // fixed distances, which are absolute lengths, and of the rebuild decision
        if (piston_on() && pist_mu != 1.0) {
          if (pist_mu_upload) { baro_buf.alloc(kBaroWords); HIPCHK(hipMemcpyAsync(baro_buf.p + 4, &pist_mu, sizeof(double), hipMemcpyHostToDevice, stream)); pist_mu_upload = false; }
          baro_apply(pist_mu, baro_buf.p + 4);
        }
        launch_fix(); need_int1 = false;
      }
      timed_step = opt_time_pair && (pair_launch_no++ % opt_time_pair) == 0;
      if (timed_step) timed_extra = 1 + (int)((pair_launch_no / opt_time_pair) % 3);
      const bool react_due = react_on && interval > 0 && ((step + 1) % interval == 0);
      const bool atrp_due = atrp_on && ((step + 1) % atrp.interval == 0);
      const bool reg_due = regions_on && region_due_at(step + 1);      // (the two half kicks apart: the rule sees x(s), v(s) complete)
      const bool last = (s == nsteps - 1);
      force_step_off = 1;      // (hybrid lists: these are the forces of step + 1, whose counter moves behind the integration)
      if (resume) { resume = false; skip_log_add(false); rebuild_now(true, resume_kind, resume_par); compute_forces(); }   // (positions are drifted, forces of this step were never evaluated)
      else if (dd_on) dd_step_sync();   // decision, (rebuild,) forces
      else if (baro_on() && resort) { if (geom_dirty) setup_geometry(); rebuild_now(); compute_forces(); }      // the scalings used the skin up, or the box asks for another plan
      else if (skip_applies() && !neighbour_launch_wanted()) {
        // the step cannot need a rebuild as far as the host can tell: the force kernel's prologue folds, decides and keeps the books
        pair_da = DecideArgs{nullptr, 0, nullptr, 0, fused_par, 0, 0.5 * skin, foldmax.p, hint_dev(), hint_gen, step};
        fused_par ^= 1;
        compute_forces(false, 0, true);
        pair_da = DecideArgs{};
        skip_log_add(true);
        if (timed_step && timed_extra == 1) ++timed_idle_skips;      // (a decide sample of 0 ms: the neighbour cost per step stays what the timers report)
      }
      else { if (skip_applies()) skip_log_add(false); decide_and_rebuild(true); compute_forces(); }
      force_step_off = 0;
      resort = false;   // a rebuild requested by the last reaction step (force_rebuild on the device) has happened by now
      if (rdf_due && (step + 1) % rdf.every == 0) rdf_launch();      // a frame of x(step + 1): behind its forces, in front of the kick (reads only)
      if (sq_due && (step + 1) % sq.every == 0) sq_launch();         // likewise

      if (last || react_due || atrp_due || reg_due || !opt_fuse || resc_kind || baro_on()) {
        launch_integrate<1>(lang, lang, step, 1);
        ++step;
        if (resc_kind == 1 || resc_kind == 3 || (resc_kind == 2 && step % (int64_t)resc_param == 0)) rescale_velocities();
        if ((react_due || atrp_due || last || baro_on()) && halted(s)) { --s; continue; }   // (the loop's ++s lands on the stopped step)
        // aftIntV: behind the velocity rescaling, in front of the reaction work
        if (piston_on()) baro_measure(); else if (baro_on()) baro_step();
        if (react_due || atrp_due || last) skip_log_confirm();
        if (react_due && !dissociations.empty()) diss_step();   // bonds break before the association scan of the step
        if (react_due) react_step();      // (takes the type snapshot of the removal rules where it finds events)
        if (react_due && react_had_events && reverse_on()) reverse_step();      // bond removals, then joins: behind the events and the neighbour changes
        if (atrp_due) atrp_step();      // behind the reaction step: the driver adds the extension after `ar` (start_simulation.py:737-740)
        if ((react_due || atrp_due) && res_tracking()) res_after_reactions();
        if ((react_due || atrp_due) && fix_tracking()) fix_after_reactions(react_due);
        if (reg_due && region_step(last) && res_tracking()) run_cut = true;      // behind everything else of the step
        need_int1 = true;
      } else {
        tbeg(2);
        launch_integrate<3>(lang, false, step, 1);
        tend();
        launch_fix();
        ++step;
      }
      timed_step = false;
    }
    check_flags();
    baro_keep = baro_on();
    tm.run_wall_s += now_s() - t0;
    tm.steps += step - step0;
    if (nsteps == 0 && keep_region) region_keep = true;      // (nothing ran: the stored forces are still the ones to go on with)
    if (opt_time_pair && !ev_used && timed_idle_skips) { tm.decide_kernel_ms = 0; tm.decide_kernel_launches = timed_idle_skips; }
    if (opt_time_pair && ev_used) {
      // Decomposed path: speculative pair launches that met a pending rebuild leave at once; they are not
      // force evaluations, so samples far below the median are dropped from the average.
      std::vector<float> d(ev_used / 2);
      for (size_t k = 0; k < ev_used / 2; ++k) HIPCHK(hipEventElapsedTime(&d[k], ev[2 * k], ev[2 * k + 1]));
      std::vector<float> pd;
      for (size_t k = 0; k < d.size(); ++k) if (ev_kind[k] == 0) pd.push_back(d[k]);
      std::sort(pd.begin(), pd.end());
      const float cut = (dd_on && !pd.empty()) ? 0.5f * pd[pd.size() / 2] : 0.f;
      tm.pair_kernel_ms = tm.rebuild_kernel_ms = tm.decide_kernel_ms = tm.integrate_kernel_ms = tm.bonded_kernel_ms = 0;
      tm.pair_kernel_launches = tm.rebuild_kernel_launches = tm.decide_kernel_launches = tm.integrate_kernel_launches = tm.bonded_kernel_launches = 0;
      for (size_t k = 0; k < d.size(); ++k) {
        const float t = d[k];
        switch (ev_kind[k]) {
          case 0: if (t >= cut) { tm.pair_kernel_ms += t; tm.pair_kernel_launches++; } break;
          // the neighbour kernel either only takes the decision (a few us) or rebuilds cells, tiles and lists
          // (hundreds of us at any size that uses the fused path): told apart by duration
          case 1: if (t > 0.03f) { tm.rebuild_kernel_ms += t; tm.rebuild_kernel_launches++; } else { tm.decide_kernel_ms += t; tm.decide_kernel_launches++; } break;
          case 2: tm.integrate_kernel_ms += t; tm.integrate_kernel_launches++; break;
          default: tm.bonded_kernel_ms += t; tm.bonded_kernel_launches++; break;
        }
      }
      tm.decide_kernel_launches += timed_idle_skips;
    }
  }

  // The int32 Verlet list (all pairs within rc+skin) is only needed by the reaction scan and by
  // diagnostics: it is produced by a forced rebuild right there instead of at every rebuild.
  void ensure_list32() {
    if (!use_tiles) { if (resort) rebuild_now(); return; }
    want32 = true;
    rebuild_now();
    want32 = false;
    if (bonds_inline() && (sizeof(R) == 8 || bond_by_pass())) rebuild_now();   // same order, same rows; the regular build: partner slots again (fp64), excluded pairs back in the force list (bond pass)
  }

  // ---- reactions ----------------------------------------------------------------------
  void alloc_reaction_buffers() {
    if (cand_cap != 0) return;
    cand_cap = std::max(8 * nglob, 1024);
    cand.alloc(cand_cap); evout.alloc(cand_cap); st0.alloc(cand_cap); st1.alloc(cand_cap);
    asA.alloc(nglob); asB.alloc(nglob); best1.alloc(nglob); best2.alloc(nglob); evcount.alloc(1); rs_dev.alloc(1);
    if (dd_on) { cand_loc.alloc((size_t)cand_cap); cnt_all.alloc(64); }
  }
  // ---- idioms shared by the routines of the reaction cadence (react_step, diss_step, atrp_step) ----
  bool any_typed_list() const { for (auto& l : top.lists) if (l.by_types) return true; return false; }
  void request_rebuild() { resort = true; hint_invalidate(); set_ctl_field(&DevCtl::force_rebuild, 1); }
  // property changes decided on the host (the mirrors already hold them) -> device arrays.  wait = false: the caller
  // keeps `chg` alive and synchronises the stream itself
  DBuf<PropChangeDev> prop_dev;
  void apply_prop_changes(const std::vector<HostTopology::PropChange>& chg, bool wait = true) {
    static_assert(sizeof(HostTopology::PropChange) == sizeof(PropChangeDev), "layout");
    if (chg.empty()) return;
    prop_dev.alloc(chg.size());
    HIPCHK(hipMemcpyAsync(prop_dev.p, chg.data(), chg.size() * sizeof(PropChangeDev), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL((k_apply_props<R>), dim3(cdiv((long long)chg.size(), 256)), dim3(256), 0, stream, (int)chg.size(), prop_dev.p, state.p, rtag.p, x4.p, v4.p);
    if (qtag_arg()) hipLaunchKernelGGL((k_apply_props_q<R>), dim3(cdiv((long long)chg.size(), 256)), dim3(256), 0, stream, (int)chg.size(), prop_dev.p, qtag.p);
    if (wait) HIPCHK(hipStreamSynchronize(stream));
  }
  // the record count of every rank, in rank order (decomposed path)
  std::vector<int> allgather_counts(int nloc) {
    if (!cnt_all.p) cnt_all.alloc(64);
    std::vector<int> cnts(P, 0);
    HIPCHK(hipMemcpyAsync(cnt_all.p + rk, &nloc, sizeof(int), hipMemcpyHostToDevice, stream));
    tr->allgather(cnt_all.p + rk, cnt_all.p, sizeof(int), stream);
    HIPCHK(hipMemcpyAsync(cnts.data(), cnt_all.p, sizeof(int) * P, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return cnts;
  }

  // ---- the association step: every `interval` steps.  The phases below run in this order; the pure host algorithms
  // they call (tables, event order, trim) are in chem_react_host.hpp ----
  void react_step() {
    tm.reaction_steps++;
    react_had_events = false;
    if (reactions.empty()) return;
    // the host runs ahead of the device by up to `interval` steps: drain that backlog first so that
    // reaction_wall_s measures the reaction step, not the MD steps queued before it
    HIPCHK(hipStreamSynchronize(stream));
    const double t0 = now_s();
    join_thread();   // labels of the previous reaction step must be on the device before the scan
    alloc_reaction_buffers();
    const ReactApplySet ras = upload_reaction_set();
    Trace trc("react");
    upload_restrictions();
    const bool any_cons = upload_constraint_bits();
    const ConnTable conn{restricted_mask ? conn_start.p : nullptr, conn_partner.p, conn_mask.p, any_cons ? cons_ok.p : nullptr};
    launch_reaction_scan(conn);
    DevCtl h = read_ctl();
    if (h.cand_overflow && use_tiles && rescan_crowded_tiles(conn)) h = read_ctl();
    trc.lap("scan");
    if (h.cand_overflow) throw ChemError(CHEM_ENOSPC, "reaction candidate buffer overflow");
    const int nc = dd_on ? gather_candidates(h.cand_count) : h.cand_count;
    if (nc == 0) { tm.reaction_wall_s += now_s() - t0; return; }
    int* status = resolve_candidates(nc, trc);
    trim_to_max_per_interval(nc, status);
    const EventSpan hev = apply_and_download_events(nc, status, ras, trc);
    react_had_events = hev.size() > 0;
    if (react_had_events && !rm_rules.empty()) reverse_snapshot();      // the types the removal rules judge by: before any association event reaches the mirrors
    commit_events(hev, trc);
    trc.lap("end");
    tm.reaction_wall_s += now_s() - t0;
  }

  // device descriptors of the reaction table; returns the half the apply kernel takes by value
  ReactApplySet upload_reaction_set() {
    ReactSet rs{};
    rs.n = (int)reactions.size(); rs.seed = react_seed; rs.step = (uint64_t)step; rs.nearest = nearest;
    ReactApplySet ras{};
    for (int q = 0; q < rs.n; ++q) {
      const chem_reaction_desc& d = reactions[q];
      ReactionDev& r = rs.r[q];
      r.type_1 = d.type_1; r.type_2 = d.type_2; r.delta_1 = d.delta_1; r.delta_2 = d.delta_2;
      r.min1 = d.min_state_1; r.max1 = d.max_state_1; r.min2 = d.min_state_2; r.max2 = d.max_state_2;
      r.intramolecular = d.intramolecular; r.intraresidual = d.intraresidual; r.active = d.active;
      r.restricted = (restricted_mask >> q) & 1u;
      r.cons_role = q < (int)constraints.size() ? constraints[q].role : 0; r.pad_ = 0;
      r.cut2 = d.cutoff * d.cutoff; r.mincut2 = d.min_cutoff * d.min_cutoff; r.prob = d.rate * dt * (double)interval;
      ras.r[q] = ReactApply{d.delta_1, d.delta_2, d.new_type_1, d.new_type_2, d.new_mass_1, d.new_mass_2};
    }
    HIPCHK(hipMemcpyAsync(rs_dev.p, &rs, sizeof(ReactSet), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return ras;
  }

  // per-tag CSR of the allowed partners (both directions), built on the host: the map is set-up data
  void upload_restrictions() {
    if (!restrict_dirty) return;
    const RestrictCsr c = build_restrict_csr(restrict_map, nglob);
    conn_start.upload(c.start, stream); conn_partner.upload(c.partner, stream); conn_mask.upload(c.mask, stream);
    restrict_dirty = false;
  }

  // neighbour-state constraints, one bit per reaction and particle; returns whether any reaction carries one
  bool upload_constraint_bits() {
    bool any_cons = false;
    for (auto& cs : constraints) any_cons |= cs.role != 0;
    if (!any_cons) return false;
    refresh_state_mirror();
    sync_type_mirrors();
    const std::vector<unsigned int> ok = constraint_bits(top, reactions, constraints);
    cons_ok.upload(ok, stream);
    return true;
  }

  // No rebuild here: the particle order must not change between the force evaluation of this step and
  // the first kick of the next one (forces are not re-sorted), and on the decomposed path a rebuild
  // would migrate particles away from their forces.  Tiles: scan the staged stencils of the last
  // rebuild (see k_react_scan_tiles).  Per-cell / brute-force lists: the int32 list is always current.
  void launch_reaction_scan(const ConnTable conn) {
    Candidate* cdst = dd_on ? cand_loc.p : cand.p;
    if (use_tiles) {
      const int region_cap = std::max(1, cand_cap / std::max(ntiles, 1));
      tile_cnt.alloc(ntiles + 1); tile_off.alloc(ntiles + 1); tile_need.alloc(ntiles + 1);
      if (scan_role.n < (size_t)acap()) scan_role.alloc((size_t)acap() + 1024);
      hipLaunchKernelGGL(k_react_roles<R>, dim3(std::min(cdiv(acap(), 256), 4096)), dim3(256), 0, stream, acap(), nglob, x4.p, tag.p, state.p, rs_dev.p, scan_role.p);
      hipLaunchKernelGGL((k_react_scan_tiles<R, 512>), dim3(ntiles), dim3(512), scan_roles_staged() ? scan_lds_bytes() : tile_lds_bytes(), stream, ntiles, tile_cap, x4.p, tag.p, tdesc.p, state.p,
                         res_id.p, mol_id.p, boxd, rs_dev.p, evout.p, region_cap, tile_cnt.p, ctl.p, (R)(0.5 * skin_eff()),
                         has_excl ? (const int*)excl_start.p : (const int*)nullptr, (const int*)excl_list.p, conn, (const unsigned int*)scan_role.p, scan_roles_staged() ? 1 : 0,
                         (const int*)nullptr, tile_need.p);
      hipLaunchKernelGGL(k_cand_offsets, dim3(1), dim3(1024), 0, stream, ntiles, tile_cnt.p, tile_off.p, ctl.p);
      hipLaunchKernelGGL(k_cand_gather, dim3(std::min(ntiles, 2048)), dim3(256), 0, stream, ntiles, evout.p, region_cap, tile_cnt.p, tile_off.p, cdst, cand_cap, ctl.p);
    } else {
      HIPCHK(hipMemsetAsync(&ctl.p->cand_count, 0, sizeof(int), stream));
      hipLaunchKernelGGL(k_react_scan<R>, dim3(cdiv((long long)n * 8, 256)), dim3(256), 0, stream, G, n, x4.p, tag.p, nlist.p, nn.p, S, state.p,
                         res_id.p, mol_id.p, boxd, rs_dev.p, cdst, cand_cap, ctl.p, conn);
    }
  }

  // The regions of the tile scan hold cand_cap / ntiles records each, a share of the MEAN density: a cluster in a dilute box
  // fills the regions of its few tiles while the candidate array is almost empty.  The scan counted on (tile_need), so when
  // the total fits cand_cap -- the documented capacity -- the tiles are scanned once more, each writing at its exclusive
  // offset straight into the candidate array (no gather).  Taken only after an overflow; a step whose regions sufficed
  // launches what it always launched.  Returns false when the candidates really exceed cand_cap (the flag stays set).
  bool rescan_crowded_tiles(const ConnTable conn) {
    std::vector<int> need;
    tile_need.download(need, (size_t)ntiles, stream);
    long long tot = 0;
    for (int v : need) tot += v;
    if (tot > cand_cap) return false;
    set_ctl_field(&DevCtl::cand_overflow, 0);
    hipLaunchKernelGGL(k_cand_offsets, dim3(1), dim3(1024), 0, stream, ntiles, tile_need.p, tile_off.p, ctl.p);
    hipLaunchKernelGGL((k_react_scan_tiles<R, 512>), dim3(ntiles), dim3(512), scan_roles_staged() ? scan_lds_bytes() : tile_lds_bytes(), stream, ntiles, tile_cap, x4.p, tag.p, tdesc.p, state.p,
                       res_id.p, mol_id.p, boxd, rs_dev.p, dd_on ? cand_loc.p : cand.p, 0, tile_cnt.p, ctl.p, (R)(0.5 * skin_eff()),
                       has_excl ? (const int*)excl_start.p : (const int*)nullptr, (const int*)excl_list.p, conn, (const unsigned int*)scan_role.p, scan_roles_staged() ? 1 : 0,
                       (const int*)tile_off.p, tile_need.p);
    return true;
  }

  // A boundary pair is seen by two ranks (real-ghost on each); the scan emits it only where the
  // particle with the lower tag is owned, so the union over ranks holds every candidate once.
  // All ranks then run the same deterministic resolve on the gathered set (one exchange).
  // nc local candidates in cand_loc -> all of them in cand, rank order; returns the global count.
  int gather_candidates(int nc) {
    const std::vector<int> cnts = allgather_counts(nc);
    int mx = 0, tot = 0;
    for (int v : cnts) { mx = std::max(mx, v); tot += v; }
    if (tot > cand_cap) throw ChemError(CHEM_ENOSPC, "reaction candidate buffer overflow (gathered)");
    if (mx > 0) {
      // padded all-gather into evout (scratch here, cand_cap records), then compaction into cand in rank order.  The padding
      // is P times the largest share: where that exceeds the scratch (a cluster inside one slab) the shares travel in pieces
      // of cand_cap / P records; otherwise in one piece
      const int piece = std::min(mx, cand_cap / P);
      for (int base = 0; base < mx; base += piece) {
        const int mine = std::max(0, std::min(piece, nc - base));
        if (mine) HIPCHK(hipMemcpyAsync(evout.p + (size_t)rk * piece, cand_loc.p + base, sizeof(Candidate) * mine, hipMemcpyDeviceToDevice, stream));
        tr->allgather(evout.p + (size_t)rk * piece, evout.p, sizeof(Candidate) * piece, stream);
        int off = 0;
        for (int r = 0; r < P; ++r) {
          const int m = std::max(0, std::min(piece, cnts[r] - base));
          if (m) HIPCHK(hipMemcpyAsync(cand.p + off + base, evout.p + (size_t)r * piece, sizeof(Candidate) * m, hipMemcpyDeviceToDevice, stream));
          off += cnts[r];
        }
      }
    }
    return tot;
  }

  // one partner per particle and side (two-sided min / keep), then the matching rounds; returns the status array
  // that holds the outcome (2 = accepted)
  int* resolve_candidates(int nc, Trace& trc) {
    const int ncb = cdiv(nc, 256), npb = cdiv(nglob, 256);
    hipLaunchKernelGGL(k_fill<int>, dim3(ncb), dim3(256), 0, stream, st0.p, 1, (size_t)nc);
    for (int side = 0; side < 2; ++side) {
      hipLaunchKernelGGL(k_fill<unsigned long long>, dim3(npb), dim3(256), 0, stream, best1.p, ~0ull, (size_t)nglob);
      hipLaunchKernelGGL(k_fill<unsigned long long>, dim3(npb), dim3(256), 0, stream, best2.p, ~0ull, (size_t)nglob);
      hipLaunchKernelGGL(k_res_min1, dim3(ncb), dim3(256), 0, stream, nc, cand.p, st0.p, side, nearest, best1.p);
      hipLaunchKernelGGL(k_res_min2, dim3(ncb), dim3(256), 0, stream, nc, cand.p, st0.p, side, nearest, best1.p, best2.p);
      hipLaunchKernelGGL(k_res_keep, dim3(ncb), dim3(256), 0, stream, nc, cand.p, st0.p, side, nearest, best1.p, best2.p);
    }
    hipLaunchKernelGGL(k_fill<int>, dim3(npb), dim3(256), 0, stream, asA.p, -1, (size_t)nglob);
    hipLaunchKernelGGL(k_fill<int>, dim3(npb), dim3(256), 0, stream, asB.p, -1, (size_t)nglob);
    hipLaunchKernelGGL(k_res_index, dim3(ncb), dim3(256), 0, stream, nc, cand.p, st0.p, asA.p, asB.p);
    if (g_trace) { HIPCHK(hipStreamSynchronize(stream)); trc.lap("uniqueAB"); }
    int* sin = st0.p; int* sout = st1.p;
    for (int batch = 0; batch < 20000; ++batch) {
      // `alive` is only meaningful for the last round of a batch: extra rounds on a finished
      // matching are no-ops, so rounds are enqueued 8 at a time between host checks
      for (int rr = 0; rr < 8; ++rr) {
        if (rr == 7) HIPCHK(hipMemsetAsync(&ctl.p->alive, 0, sizeof(int), stream));
        hipLaunchKernelGGL(k_res_round, dim3(ncb), dim3(256), 0, stream, nc, cand.p, sin, sout, asA.p, asB.p, nearest, ctl.p);
        std::swap(sin, sout);
      }
      if (read_ctl().alive == 0) break;
    }
    if (g_trace) { fprintf(stderr, "[chem trace] candidates %d\n", nc); trc.lap("rounds"); }
    return sin;
  }

  // ChemicalReaction.max_per_interval: rare option, selection on the host from the downloaded candidate records (trim_accepted)
  void trim_to_max_per_interval(int nc, int* status) {
    if (max_per_interval <= 0) return;
    std::vector<Candidate> hc; std::vector<int> hs;
    cand.download(hc, nc, stream);
    { hs.resize(nc); HIPCHK(hipMemcpyAsync(hs.data(), status, sizeof(int) * nc, hipMemcpyDeviceToHost, stream)); HIPCHK(hipStreamSynchronize(stream)); }
    if (!trim_accepted(hc, hs, max_per_interval, nearest != 0)) return;
    HIPCHK(hipMemcpyAsync(status, hs.data(), sizeof(int) * nc, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }

  // the event records are processed where the copy kernel put them (pinned, host-cached memory): no second copy
  struct EventSpan { Candidate* p; size_t n; Candidate* begin() const { return p; } Candidate* end() const { return p + n; }
                     Candidate* data() const { return p; } size_t size() const { return n; } Candidate& operator[](size_t k) const { return p[k]; } };
  // accepted candidates -> states, types and masses on the device + the event records, in device order, in pin_ev
  EventSpan apply_and_download_events(int nc, const int* status, const ReactApplySet& ras, Trace& trc) {
    HIPCHK(hipMemsetAsync(evcount.p, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_react_apply<R>, dim3(cdiv(nc, 256)), dim3(256), 0, stream, nc, cand.p, status, ras, state.p, rtag.p, x4.p, v4.p, evout.p, evcount.p);
    if (qtag_arg()) {      // charges of the reactants, by tag
      ReactQSet rqs{};
      for (size_t q = 0; q < reactions.size(); ++q) rqs.r[q] = ReactQ{reactions[q].new_type_1, reactions[q].new_type_2, reactions[q].new_q_1, reactions[q].new_q_2};
      hipLaunchKernelGGL(k_react_apply_q<R>, dim3(cdiv(nc, 256)), dim3(256), 0, stream, nc, (const Candidate*)cand.p, (const int*)status, rqs, qtag.p);
    }
    int nev = 0;
    HIPCHK(hipMemcpyAsync(&nev, evcount.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    trc.lap("resolve+apply");
    if ((size_t)nev > pin_ev_cap) {
      if (pin_ev) (void)hipHostFree(pin_ev);
      pin_ev_cap = std::max<size_t>((size_t)nev * 2, 1 << 16);
      HIPCHK(hipHostMalloc((void**)&pin_ev, pin_ev_cap * sizeof(Candidate), hipHostMallocDefault));
    }
    if (nev) {
      const size_t n16 = ((size_t)nev * sizeof(Candidate) + 15) / 16;   // evout/pin_ev are sized in whole candidates (24 B): rounding up stays inside
      hipLaunchKernelGGL(k_copy16, dim3(512), dim3(256), 0, stream, reinterpret_cast<const uint4*>(evout.p), reinterpret_cast<uint4*>(pin_ev), n16);
    }
    HIPCHK(hipStreamSynchronize(stream));
    trc.lap("download");
    return EventSpan{pin_ev, (size_t)nev};
  }

  // bond-forming events in canonical order, extracted into a heap buffer (bond_ev); the pinned event array stays as the device wrote it.
  // (0.6-0.8 ms at 2.5e5 events, as partitioning and sorting in place was: ONE pass over 6 MB the GPU has just written
  //  through PCIe is most of it -- a device-side compaction of the bond-forming events would be the next step)
  void collect_bond_events(const EventSpan hev) {
    bond_ev.clear();
    for (const Candidate& e : hev) if (!reactions[e.r].is_virtual) bond_ev.push_back(e);
    sort_bond_events(bond_ev, radix_tmp);
  }

  // bond_ev -> the bonded lists; appends the bonds that are new to `newbonds`, in canonical order
  // (measured, round 3: inserting by hash shards on helper threads -- a persistent pool of 1..3 -- made this loop SLOWER,
  //  1.0-1.7 ms -> 2.0-3.9 ms for 2.4-4.3e4 new bonds on the 2-socket host: the table lives on the caller's NUMA node)
  // defer_seen: every bond-forming event is known to be a new bond (see commit_events); the insertion into the list's
  // de-duplication set -- one cache miss per bond in a table of 10^6, 0.2 -> 1.7 ms of this step as the conversion
  // grows -- is left to the bookkeeping thread (label_seen_lists).
  void insert_new_bonds(bool defer_seen, std::vector<std::pair<int32_t, int32_t>>& newbonds) {
    const std::vector<Candidate>& bev = bond_ev;
    top.cur_step = step;      // (the birth step of what a hybrid list gains here)
    label_seen_lists.clear();
    for (size_t k = 0; defer_seen && k < bev.size(); ++k) {
      const Candidate& e = bev[k];
      const chem_reaction_desc& d = reactions[e.r];
      HostList& l = top.lists[d.bond_list];
      const int32_t t[2] = {e.a, e.b};
      l.push_pair(t, step);
      newbonds.emplace_back(e.a, e.b);
      label_seen_lists.push_back(d.bond_list);
    }
    for (size_t k = 0; !defer_seen && k < bev.size(); ++k) {
      const Candidate& e = bev[k];
      const chem_reaction_desc& d = reactions[e.r];
      if (k + 24 < bev.size()) {   // the de-duplication set is a 10^6-entry hash table: hide its misses
        int32_t tp[2] = {bev[k + 24].a, bev[k + 24].b};
        top.lists[reactions[bev[k + 24].r].bond_list].seen.prefetch(tuple_key(tp, 2));
      }
      int32_t t[2] = {e.a, e.b};
      if (top.list_insert(top.lists[d.bond_list], t)) newbonds.emplace_back(e.a, e.b);
    }
  }

  // PostProcessChangeNeighboursProperty: needs the bond graph with this step's bonds and the mirrors of the new
  // types; events in canonical order, role 1 before role 2, rules in insertion order (as the oracle).  Returns whether
  // any particle changed.
  bool neighbour_changes(const EventSpan hev) {
    if (nb_rules.empty()) return false;
    std::vector<Candidate> ord;
    for (auto& e : hev) for (auto& rl : nb_rules) if (rl.reaction == e.r) { ord.push_back(e); break; }
    std::sort(ord.begin(), ord.end(), [](const Candidate& p, const Candidate& q) { return event_key(p) < event_key(q); });
    bool reads_state = false;
    for (auto& rl : nb_rules) reads_state |= rl.set_state == 2 || rl.min_state < rl.max_state;
    if (reads_state) refresh_state_mirror(true);      // states as the events of this step left them (k_react_apply ran on the device)
    std::vector<HostTopology::PropChange> chg;
    for (auto& e : ord)
      for (int role = 1; role <= 2; ++role)
        for (auto& rl : nb_rules) if (rl.reaction == e.r && (rl.invoke_on & role)) top.neighbour_change(role == 1 ? e.a : e.b, rl, chg);
    if (chg.empty()) return false;
    // k_apply_props takes one lane per record: a particle that several visits changed (chained rules, two events around one
    // neighbour) gets ONE record, with what the last visit left in the mirrors (every record holds absolute values; the state
    // mirror is right wherever a record of the particle set it)
    {
      std::unordered_map<int32_t, size_t> at;
      size_t w = 0;
      for (const HostTopology::PropChange& c : chg) {
        auto it = at.find(c.tag);
        if (it == at.end()) { at.emplace(c.tag, w); chg[w++] = c; continue; }
        HostTopology::PropChange& m = chg[it->second];
        m.type = c.type; m.mass = c.mass; m.q = c.q;
        if (c.set_state) { m.set_state = 1; m.state = c.state; }
      }
      chg.resize(w);
    }
    apply_prop_changes(chg);
    if (!reads_state) state_mirror_stale = true;      // (rules that set a state moved the device copy, not a refreshed mirror)
    return true;
  }

  // the bookkeeping thread of this reaction step (joined by join_thread, which rethrows what it caught)
  template <class F> void start_label_thread(F body) {
    label_thr = std::thread([this, body = std::move(body)] { try { body(); } catch (...) { label_err = std::current_exception(); } });
  }

  // Host mirrors + topology.  Only bond-forming events need the canonical order now (it fixes
  // the order of the bond lists); the event log itself is put in canonical order lazily
  // by chem_get_events.
  void commit_events(const EventSpan hev, Trace& trc) {
    collect_bond_events(hev);
    trc.lap("bond events");
    // event log + host mirrors of the new types (only what the host itself needs later: types for
    // bonded-slot resolution and the topology manager; chemical states live on the device).  Events
    // touch disjoint particles, nothing below reads the mirrors unless a list is typed or tuples are
    // spawned, so this runs beside the table builds and is joined at the end of the step.
    // intra-/inter-cluster flag of every event from the cluster labels as they were BEFORE this step's bonds
    // (the label thread of the previous reaction step was joined above, this step's has not started yet)
    std::vector<int8_t> intra_flags;
    if (opt_intra_inter) {
      intra_flags.resize(hev.size());
      for (size_t k = 0; k < hev.size(); ++k) intra_flags[k] = top.mol_id[hev[k].a] == top.mol_id[hev[k].b] ? 1 : 0;
    }
    bool types_changed = false;
    for (size_t k = 0; k < hev.size() && !types_changed; ++k) { const chem_reaction_desc& d = reactions[hev[k].r]; types_changed = d.new_type_1 >= 0 || d.new_type_2 >= 0; }   // (conservative: the force list depends on the types)
    // event log: appended to the arena in device order (canonical order is established lazily by chem_get_events).
    // The host's type mirrors are needed right now only where the host itself resolves something by type;
    // otherwise the log is appended on the thread, while the device rebuilds its tables.
    const bool mirrors_first = top.spawns_tuples() || !nb_rules.empty() || any_typed_list();
    if (mirrors_first) { append_events(hev.data(), hev.size(), step, intra_flags); sync_type_mirrors(); }
    // what the thread still has to log (pin_ev is not touched again before the next reaction step, which joins the thread first)
    const size_t log_n = mirrors_first ? 0 : hev.size();
    auto log_events = [this, log_ev = hev.data(), log_n, log_step = step, intra_flags] { if (log_n) append_events(log_ev, log_n, log_step, intra_flags); };
    // Where every bond is an excluded pair (bonds_excluded: checked at the last full upload, kept by construction since) and the
    // scan honours the exclusions, a candidate pair cannot be bonded already, and a particle takes part in one event per step:
    // every bond-forming event is a new bond.
    const bool defer_seen = bonds_excluded && has_excl && !top.spawns_tuples() && nb_rules.empty();
    std::vector<std::pair<int32_t, int32_t>> newbonds;
    newbonds.reserve(hev.size());
    insert_new_bonds(defer_seen, newbonds);
    state_mirror_stale = true;
    if (g_trace) fprintf(stderr, "[chem trace] events %zu new bonds %zu\n", hev.size(), newbonds.size());
    trc.lap("host events");
    if (newbonds.empty()) {
      if (log_n) start_label_thread(std::move(log_events));     // no bonds, no label work: the thread only writes the log
      types_changed |= neighbour_changes(hev);   // rules on reactions that form no bond
    } else {
      label_bonds = newbonds; label_touched.clear(); labels_pending = true;
      if (!nb_rules.empty()) {
        // same dependency order as below, fully synchronous: graph -> (labels on the thread) -> spawned tuples (types as
        // they are right after the events) -> neighbour property changes -> tables
        top.link_new_bonds(newbonds);
        start_label_thread([this] { top.merge_new_bonds(label_bonds, label_touched); });
        top.spawn_for_new_bonds(newbonds);
        if (label_thr.joinable()) label_thr.join();   // the flood fill reads the graph only; types are not touched by it, but keep it simple
        types_changed |= neighbour_changes(hev);
        upload_excl(false);
        upload_bonded(false);
      } else {
        // Host work of a bond-forming step, arranged by what depends on what:
        //   bonded CSR  <- lists            exclusion CSR <- exclusions <- (spawned tuples <- graph)
        //   cluster labels <- graph, read again only by the NEXT reaction scan -> host thread, joined lazily
        if (!top.spawns_tuples()) {
          // the device tables only need the new tuples / pairs: the bond graph, the cluster labels AND the host's own
          // exclusion rows (read by chem_get_exclusions only) are brought up to date on the thread, beside the MD steps
          top.excl_log.reserve(top.excl_log.size() + newbonds.size());
          for (auto& e : newbonds) top.excl_log.emplace_back(e.first, e.second);   // (a bond's pair is always new: list_insert deduplicated)
          start_label_thread([this, log_events = std::move(log_events)] {
            log_events();
            for (size_t k = 0; k < label_seen_lists.size(); ++k) {      // (deferred de-duplication keys of this step's bonds)
              const int32_t t[2] = {label_bonds[k].first, label_bonds[k].second};
              top.lists[label_seen_lists[k]].seen.insert(tuple_key(t, 2));
            }
            top.link_new_bonds(label_bonds); top.merge_new_bonds(label_bonds, label_touched);
            // rows + pair count; the log already holds these pairs
            for (auto& e : label_bonds) { if (HostTopology::sorted_insert(top.excl[e.first], e.second)) { HostTopology::sorted_insert(top.excl[e.second], e.first); ++top.n_excl_pairs; } }
          });
          trc.lap("threads started");
        } else {
          top.link_new_bonds(newbonds);
          start_label_thread([this] { top.merge_new_bonds(label_bonds, label_touched); });
          top.spawn_for_new_bonds(newbonds);
          trc.lap("link+spawn");
        }
        upload_excl(false, false);
        upload_bonded(false, false);
        trc.lap("table builds enqueued");
        HIPCHK(hipStreamSynchronize(stream));
        trc.lap("uploads");
      }
      request_rebuild();
    }
    if (types_changed) request_rebuild();   // force list depends on types
    if (newbonds.empty() && types_changed && any_typed_list()) upload_bonded(false);     // same tuples, slots re-resolved against the new types
  }

  // ---- dissociation reactions: every `interval` steps, in front of the association scan (rule set: include/chem_mi355.h) ----
  // Device: k_diss_scan over the flat tuple arrays -> records of the broken bonds.  Host: canonical order, property changes
  // (accumulated: one particle may lose several bonds), removal from every table (HostTopology::remove_bonds), then the
  // synchronous full path of a set-up change: both CSR tables from scratch, labels, forced rebuild.  O(all bonds) per step
  // that breaks something; a step that breaks nothing costs the scan and one read-back.
  DBuf<Candidate> diss_rec; DBuf<int> diss_count;
  // behind HostTopology::remove_bonds (diss_step, reverse_step): the synchronous full path of a set-up change
  void rebuild_tables_after_removal() {
    excl_deg.clear();      // (the exclusion log shrank: degrees are counted afresh)
    upload_excl(true);
    upload_bonded(true);      // (re-proves bonds_excluded: a break that keeps its exclusion ends the inline-bond mode; typed slots against the new types)
    mol_id.upload(top.mol_id, stream);
    HIPCHK(hipStreamSynchronize(stream));
    request_rebuild();
  }

  // ---- reverse reactions (rule sets: include/chem_mi355.h, chem_reaction_remove_bond / chem_reaction_join; host selection:
  // chem_react_host.hpp select_removals, chem_fix_host.hpp join_by_reaction) ----
  // A reaction step without events pays nothing for the rules: the snapshot is taken, and reverse_step() is called, only
  // where react_step() found events (react_had_events).
  std::vector<int32_t> type0;      // types at the start of this step's association phase
  bool react_had_events = false;
  void reverse_snapshot() {
    join_async();      // mirrors replayed up to the last step's events (this step's are not in the arena yet); diss_step keeps them current itself
    type0 = top.type;
  }
  DBuf<FixEnt<R>> place_dev;
  void reverse_step() {
    HIPCHK(hipStreamSynchronize(stream));
    const double t0 = now_s();
    join_async();      // this step's block is in the arena, its bonds are in the graph and the lists, the mirrors hold the new types
    std::vector<AssocEvent> evs;
    for (size_t bk = arena.blocks.size(); bk-- > 0 && arena.blocks[bk].first == step;) {
      const size_t lo = arena.blocks[bk].second, hi = bk + 1 < arena.blocks.size() ? arena.blocks[bk + 1].second : arena.size();
      for (size_t k = lo; k < hi; ++k) if (arena.r[k] >= 0) evs.push_back(AssocEvent{arena.a[k], arena.b[k], arena.r[k]});
    }
    if (evs.empty()) return;
    std::sort(evs.begin(), evs.end(), [](const AssocEvent& p, const AssocEvent& q) { return event_key(p) < event_key(q); });
    Trace trc("reverse");
    if (!rm_rules.empty()) {
      const std::vector<RemovedBond> rem = select_removals(top, type0, reactions, rm_rules, evs);
      std::vector<int> rrow;
      const std::vector<HostTopology::BrokenBond> broken = removals_by_list(top, rem, &rrow);
      if (!broken.empty()) {
        for (size_t k = 0; k < broken.size(); ++k) removed_log.push_back(RemovedRec{step, broken[k].a, broken[k].b, broken[k].list, public_index(rrow[k])});
        std::vector<int32_t> touched;
        top.remove_bonds(broken, touched);
        if (g_trace) fprintf(stderr, "[chem trace] removed bonds %zu\n", broken.size());
        trc.lap("host removal");
        rebuild_tables_after_removal();
        trc.lap("table rebuild");
      }
    }
    if (!fix.joins.empty()) {
      std::vector<FixState::JoinEvent> jev;
      for (const AssocEvent& e : evs) jev.push_back(FixState::JoinEvent{public_index(e.reaction), e.a, e.b});
      const std::vector<FixEntry> added = fix.join_by_reaction(jev, step, top.n);
      if (!added.empty()) {
        std::vector<FixEnt<R>> h(added.size());
        for (size_t k = 0; k < added.size(); ++k) { h[k] = FixEnt<R>{}; h[k].a = added[k].anchor; h[k].t = added[k].target; h[k].d = (R)added[k].dist; }
        place_dev.upload(h, stream);
        FixGeom<R> g{};
        for (int d = 0; d < 3; ++d) { g.L[d] = (R)L[d]; g.invL[d] = (R)(1.0 / L[d]); }
        hipLaunchKernelGGL((k_fix_place<R>), dim3(cdiv((long long)added.size(), 256)), dim3(256), 0, stream, (int)added.size(), place_dev.p, rtag.p, nglob, x4.p, v4.p, g, pos_scale());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        upload_fix();
        request_rebuild();      // the target jumped: the rebuild bins it where it is now
        trc.lap("joins");
      }
    }
    tm.reaction_wall_s += now_s() - t0;
  }

  void diss_step() {
    bool any = false;
    for (auto& d : dissociations) any |= d.active != 0;
    if (!any) return;
    HIPCHK(hipStreamSynchronize(stream));
    const double t0 = now_s();
    join_thread();      // lists, graph, labels and exclusion rows of the previous reaction step are complete
    if (fent_n == 0) return;
    Trace trc("diss");
    DissSet ds{};
    ds.n = (int)dissociations.size(); ds.seed = react_seed; ds.step = (unsigned long long)step;
    for (int q = 0; q < ds.n; ++q) {
      const chem_dissociation_desc& d = dissociations[q];
      DissDev& r = ds.r[q];
      r.type_1 = d.type_1; r.type_2 = d.type_2; r.min1 = d.min_state_1; r.max1 = d.max_state_1; r.min2 = d.min_state_2; r.max2 = d.max_state_2;
      r.list = d.bond_list; r.active = d.active; r.pub = diss_pub[q]; r.pad = 0;
      r.cut2 = d.cutoff > 0 ? d.cutoff * d.cutoff : 0.0; r.prob = d.diss_rate * dt * (double)interval;
    }
    if (diss_rec.n < fent_n) diss_rec.alloc(fent_n + fent_n / 2 + 1024);
    if (!diss_count.p) diss_count.alloc(1);
    HIPCHK(hipMemsetAsync(diss_count.p, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_diss_scan<R>, dim3(cdiv((long long)fent_n, 256)), dim3(256), 0, stream, (int)fent_n, fent.p, flist.p, x4.p, rtag.p, nglob,
                       state.p, boxd, ds, diss_rec.p, (int)diss_rec.n, diss_count.p);
    int nrec = 0;
    HIPCHK(hipMemcpyAsync(&nrec, diss_count.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    trc.lap("scan");
    if (nrec <= 0) { tm.reaction_wall_s += now_s() - t0; return; }
    std::vector<Candidate> rec;
    diss_rec.download(rec, (size_t)nrec, stream);
    std::sort(rec.begin(), rec.end(), [&](const Candidate& p, const Candidate& q) {
      const int lp = dissociations[p.r].bond_list, lq = dissociations[q.r].bond_list;
      return lp != lq ? lp < lq : p.h < q.h;
    });
    // property changes on the mirrors, in canonical order; states as they are on the device
    refresh_state_mirror();
    sync_type_mirrors();
    std::vector<int32_t> changed;
    std::vector<HostTopology::BrokenBond> broken;
    broken.reserve(rec.size());
    for (Candidate& e : rec) {
      const chem_dissociation_desc& d = dissociations[e.r];
      top.state[e.a] += d.delta_1; top.state[e.b] += d.delta_2;
      if (d.new_type_1 >= 0) { top.type[e.a] = d.new_type_1; top.mass[e.a] = d.new_mass_1; top.q[e.a] = d.new_q_1; }
      if (d.new_type_2 >= 0) { top.type[e.b] = d.new_type_2; top.mass[e.b] = d.new_mass_2; top.q[e.b] = d.new_q_2; }
      changed.push_back(e.a); changed.push_back(e.b);
      broken.push_back(HostTopology::BrokenBond{e.a, e.b, d.bond_list, d.unexclude});
      e.r = ~e.r;      // the arena tells the two kinds of event apart by the sign
    }
    std::sort(changed.begin(), changed.end());
    changed.erase(std::unique(changed.begin(), changed.end()), changed.end());
    std::vector<HostTopology::PropChange> chg;
    chg.reserve(changed.size());
    for (int32_t t : changed) chg.push_back(HostTopology::PropChange{t, top.type[t], 1, top.state[t], top.mass[t], top.q[t]});
    apply_prop_changes(chg, false);      // (runs beside the host removal below)
    append_events(rec.data(), rec.size(), step, std::vector<int8_t>());
    arena.mirror_pos = arena.size();
    std::vector<int32_t> touched;
    top.remove_bonds(broken, touched);
    HIPCHK(hipStreamSynchronize(stream));
    if (g_trace) fprintf(stderr, "[chem trace] broken bonds %zu\n", rec.size());
    trc.lap("host removal");
    rebuild_tables_after_removal();
    trc.lap("table rebuild");
    tm.reaction_wall_s += now_s() - t0;
  }

  // ---- ATRPActivator: every `interval` steps, on the host (a few thousand centres at reaction cadence) -----------
  // Rule set: include/chem_mi355.h (chem_atrp_desc).  Types and states live on the device: the state array is read
  // back, the type mirrors are replayed from the event arena, the flips go back through k_apply_props.
  void atrp_step() {
    HIPCHK(hipStreamSynchronize(stream));
    join_async();
    refresh_state_mirror();
    const AtrpOutcome o = atrp_select(top, atrp, atrp_centers, step);      // (mirrors and catalyst ratios updated)
    atrp_stats.push_back(o.stats);
    apply_prop_changes(o.changes);
    if (o.types_changed) {     // the force list and the typed bonded slots depend on the types
      if (any_typed_list()) upload_bonded(false);
      request_rebuild();
    }
  }

  // ---- region rules (rule set: include/chem_mi355.h; selection: chem_region_host.hpp; scan: md_kernels.hpp) ----------------
  // region_step: the scan of a firing step, one launch on the run's stream.  On the fused tile path the host does not wait: a
  // firing that changes something stops the run on the device and comes back through run()'s halted().  Elsewhere (the
  // unfused rebuild chain does not know a stopped run; a barostat waits on every step anyway) and at the end of a call the
  // host looks at once.  Returns whether a change was applied here.
  DBuf<RegionCand> region_rec; DBuf<RegionOut> region_out; DBuf<RegionReset> region_reset_dev;
  bool region_step(bool last) {
    RegionSet rs{};
    rs.par = fused_par; rs.gen = hint_gen; rs.step = (unsigned long long)step;
    for (size_t k = 0; k < regions.size(); ++k) {
      const chem_region_desc& d = regions[k];
      if (!region_due(d, region_enabled[k] != 0, step)) continue;
      RegionDev& r = rs.r[rs.n++];
      for (int a = 0; a < 3; ++a) { r.lo[a] = d.lo[a]; r.hi[a] = d.hi[a]; }
      r.value = d.value; r.seed = d.seed; r.target_type = d.target_type; r.mode = d.mode; r.num = d.num; r.rule = (int)k;
      rs.type_mask |= 1u << d.target_type;
    }
    if (rs.n == 0) return false;
    if (step > region_counted) { ++region_firings; region_counted = step; }      // (a step redone behind a stopped run counts once)
    if (region_rec.n < (size_t)n) {
      region_rec.alloc((size_t)n); region_out.alloc(1);
      HIPCHK(hipMemsetAsync(region_out.p, 0, sizeof(RegionOut), stream));
    }
    const bool wait = last || !use_fused || baro_on();
    IdleHint* hint = nullptr;
    if (!wait) { ensure_hflag(); hint = hint_dev(); }
    hipLaunchKernelGGL((k_region_scan<R>), dim3(cdiv(n, 256)), dim3(256), 0, stream, n, (const V4*)(x4.p + G), (const int*)(tag.p + G), boxd, rs,
                       region_rec.p, (int)region_rec.n, region_out.p, ctl.p, hint);
    HIPCHK(hipGetLastError());
    if (!wait) return false;
    if (!last) ++region_syncs;
    HIPCHK(hipStreamSynchronize(stream));
    const DevCtl h = read_ctl();
    if (h.halt != 4) return false;
    set_ctl_field(&DevCtl::halt, 0);
    if (last) ++region_syncs;
    region_apply();
    return true;
  }
  // The change of a firing step, on the host: records down, the selection over them, properties through the route of every
  // host-decided change (mirrors, k_apply_props, charges), the resets, then what follows a type change by any route.  Forces
  // are not evaluated here: the list build is requested for the next evaluation.
  void region_apply() {
    HIPCHK(hipStreamSynchronize(stream));
    join_async();      // the mirrors are written below
    RegionOut ro{};
    HIPCHK(hipMemcpyAsync(&ro, region_out.p, sizeof(RegionOut), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const size_t nrec = (size_t)std::min<int64_t>(std::max(ro.nrec, 0), (int64_t)region_rec.n);
    std::vector<RegionCand> recs;
    if (nrec) region_rec.download(recs, nrec, stream);
    HIPCHK(hipMemsetAsync(region_out.p, 0, sizeof(RegionOut), stream));
    std::vector<RegionChange> chgs;
    region_fire(regions, region_enabled, step, recs, chgs, region_stats);
    if (chgs.empty()) return;
    // a particle hit by several rules of the step: properties of the last, resets of all
    std::vector<int32_t> tags; std::map<int32_t, int> flags;
    for (const RegionChange& c : chgs) {
      const chem_region_desc& d = regions[c.rule];
      const int32_t t = c.tag;
      top.type[t] = d.new_type;
      if (!(d.new_mass < 0)) { top.mass[t] = d.new_mass; top.q[t] = d.new_q; }
      flags[t] |= (d.reset_velocity ? 1 : 0) | (d.reset_force ? 2 : 0);
      region_log.push_back(c);
    }
    std::vector<HostTopology::PropChange> props; std::vector<RegionReset> resets;
    for (const auto& f : flags) {
      const int32_t t = f.first;
      props.push_back(HostTopology::PropChange{t, top.type[t], 0, 0, top.mass[t], top.q[t]});
      if (f.second) resets.push_back(RegionReset{t, f.second});
    }
    apply_prop_changes(props, false);
    if (!resets.empty()) {
      region_reset_dev.upload(resets, stream);
      hipLaunchKernelGGL((k_region_reset<R>), dim3(cdiv((long long)resets.size(), 256)), dim3(256), 0, stream, (int)resets.size(), region_reset_dev.p, rtag.p, v4.p, f4.p);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(stream));
    if (res.on()) {      // re-stamped under the old type's rate, at this step
      res.ensure(top.type);
      std::vector<int32_t> changed;
      res.restamp_type_changes(top.type, step, changed);
      res_push(changed);
    }
    if (any_typed_list()) upload_bonded(false);
    request_rebuild();
    if (fix_tracking()) fix_after_reactions(false);      // a typed set judges its entries with the new type
    region_keep = true;
  }

  // ---- read-back ------------------------------------------------------------------------
  // ---- cross-rank gather of fixed-size host records (read-back paths only) ---------------
  DBuf<unsigned char> gbuf;
  std::vector<unsigned char> gather_records(const std::vector<unsigned char>& loc, size_t rec) {
    if (!dd_on || P == 1) return loc;
    const int nloc = (int)(loc.size() / rec);
    const std::vector<int> cnts = allgather_counts(nloc);
    size_t mx = 0, tot = 0;
    for (int v : cnts) { mx = std::max<size_t>(mx, v); tot += v; }
    std::vector<unsigned char> all(tot * rec);
    if (mx == 0) return all;
    // sized once for any record type and a slab 50 % over its share (it only grows beyond that): the inter-process transport
    // maps peer allocations by handle and caches the mappings -- a buffer that is freed and allocated again at another size
    // between two gathers handed the peers a stale mapping ("copy: invalid argument" in the multi-process driver run)
    if (gbuf.n < mx * rec * P) gbuf.alloc(std::max(mx * rec * P, ((size_t)nglob * 3 / (2 * (size_t)P) + 1024) * 64 * (size_t)P));
    if (nloc) HIPCHK(hipMemcpyAsync(gbuf.p + (size_t)rk * mx * rec, loc.data(), loc.size(), hipMemcpyHostToDevice, stream));
    tr->allgather(gbuf.p + (size_t)rk * mx * rec, gbuf.p, mx * rec, stream);
    std::vector<unsigned char> raw(mx * rec * P);
    HIPCHK(hipMemcpyAsync(raw.data(), gbuf.p, raw.size(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    size_t off = 0;
    for (int r = 0; r < P; ++r) { std::memcpy(all.data() + off, raw.data() + (size_t)r * mx * rec, (size_t)cnts[r] * rec); off += (size_t)cnts[r] * rec; }
    return all;
  }

  struct StateRec { int tag, pad; double v[3]; };

  // ---- read-back ------------------------------------------------------------------------
  int64_t get_state(int what, void* out, int64_t cap) override {
    flush_host_state();
    const int per = (what == CHEM_STATE_POS || what == CHEM_STATE_VEL || what == CHEM_STATE_FORCE || what == CHEM_STATE_IMAGE || what == CHEM_STATE_POS_UNFOLDED) ? 3 : 1;
    if (cap < (int64_t)nglob * per) throw ChemError(CHEM_ENOSPC, "get_state: capacity");
    double* d = (double*)out; int32_t* i32 = (int32_t*)out; int64_t* i64 = (int64_t*)out;
    switch (what) {   // replicated by-tag data: no gather
      case CHEM_STATE_STATE: { std::vector<int> h; state.download(h, nglob, stream); std::copy(h.begin(), h.end(), i32); return nglob; }
      case CHEM_STATE_RESID: { std::vector<int> h; res_id.download(h, nglob, stream); std::copy(h.begin(), h.end(), i32); return nglob; }
      case CHEM_STATE_MOLID: {      // an id in an int32 array: refused where an id does not fit (ids are ascending by tag: the ends decide)
        if (nglob > 0 && (!fits_int32(top.id.front()) || !fits_int32(top.id.back()))) throw ChemError(CHEM_EINVAL, "get_state: CHEM_STATE_MOLID is an int32 read-back of particle ids and this context holds ids beyond 32 bits");
        std::vector<int> h; mol_id.download(h, nglob, stream); for (int t = 0; t < nglob; ++t) i32[t] = (int32_t)top.id[h[t]]; return nglob; }
      case CHEM_STATE_ID: for (int t = 0; t < nglob; ++t) i64[t] = top.id[t]; return nglob;
      case CHEM_STATE_CHARGE: {      // the device's by-tag array while it is alive (charges_on), the host mirror otherwise
        if (charges_on() && qtag.p) { std::vector<R> h; qtag.download(h, nglob, stream); for (int t = 0; t < nglob; ++t) d[t] = (double)h[t]; }
        else for (int t = 0; t < nglob; ++t) d[t] = top.q[t];
        return nglob;
      }
      default: break;
    }
    // per-particle data of the owned range [G, G+n)
    std::vector<int> ht(n); std::vector<V4> hv(n); std::vector<int4> hi;
    if (n) HIPCHK(hipMemcpyAsync(ht.data(), tag.p + G, sizeof(int) * n, hipMemcpyDeviceToHost, stream));
    const V4* src = (what == CHEM_STATE_VEL || what == CHEM_STATE_MASS) ? v4.p : (what == CHEM_STATE_FORCE ? f4.p : x4.p);
    if (n) HIPCHK(hipMemcpyAsync(hv.data(), src + G, sizeof(V4) * n, hipMemcpyDeviceToHost, stream));
    if (what == CHEM_STATE_POS_UNFOLDED || what == CHEM_STATE_IMAGE) { hi.resize(n); if (n) HIPCHK(hipMemcpyAsync(hi.data(), img4.p + G, sizeof(int4) * n, hipMemcpyDeviceToHost, stream)); }
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<unsigned char> loc((size_t)n * sizeof(StateRec));
    StateRec* rec = reinterpret_cast<StateRec*>(loc.data());
    for (int i = 0; i < n; ++i) {
      StateRec r{ht[i], 0, {(double)hv[i].x, (double)hv[i].y, (double)hv[i].z}};
      if (src == x4.p) { r.v[0] = dec_pos(hv[i].x, 0); r.v[1] = dec_pos(hv[i].y, 1); r.v[2] = dec_pos(hv[i].z, 2); }
      if (what == CHEM_STATE_POS) { for (int k = 0; k < 3; ++k) { double s = std::floor(r.v[k] / L[k]); r.v[k] -= s * L[k]; if (r.v[k] >= L[k]) r.v[k] -= L[k]; } }
      else if (what == CHEM_STATE_POS_UNFOLDED) { r.v[0] += hi[i].x * L[0]; r.v[1] += hi[i].y * L[1]; r.v[2] += hi[i].z * L[2]; }
      else if (what == CHEM_STATE_IMAGE) { r.v[0] = hi[i].x; r.v[1] = hi[i].y; r.v[2] = hi[i].z; }
      else if (what == CHEM_STATE_MASS || what == CHEM_STATE_TYPE) r.v[0] = (double)hv[i].w;
      rec[i] = r;
    }
    const std::vector<unsigned char> all = gather_records(loc, sizeof(StateRec));
    const StateRec* ar = reinterpret_cast<const StateRec*>(all.data());
    const size_t na = all.size() / sizeof(StateRec);
    if ((int64_t)na != nglob) throw ChemError(CHEM_ESTATE, "get_state: owned particles do not add up to the global count (" + std::to_string(na) + " vs " + std::to_string(nglob) + ")");
    for (size_t k = 0; k < na; ++k) {
      const int t = ar[k].tag;
      switch (what) {
        case CHEM_STATE_MASS: d[t] = ar[k].v[0]; break;
        case CHEM_STATE_TYPE: i32[t] = (int32_t)ar[k].v[0]; break;
        case CHEM_STATE_IMAGE: for (int c = 0; c < 3; ++c) i32[3 * t + c] = (int32_t)ar[k].v[c]; break;
        default: for (int c = 0; c < 3; ++c) d[3 * t + c] = ar[k].v[c]; break;
      }
    }
    if (what != CHEM_STATE_POS && what != CHEM_STATE_POS_UNFOLDED && what != CHEM_STATE_VEL && what != CHEM_STATE_FORCE && what != CHEM_STATE_MASS &&
        what != CHEM_STATE_TYPE && what != CHEM_STATE_IMAGE) throw ChemError(CHEM_EINVAL, "get_state: unknown selector");
    return nglob;
  }

  void observe(chem_obs* out) override {
    flush_host_state();
    if (resort) { rebuild_now(); compute_forces(); }   // a rebuild re-sorts the particles but not f4: keep it aligned for get_state(FORCE)
    std::memset(out, 0, sizeof(*out));
    const int nb = launch_pair<true>(x4o.p);  // scratch force buffer: leaves f4 untouched
    HIPCHK(hipMemsetAsync(elist.p, 0, sizeof(double) * CHEM_MAX_LISTS, stream));
    if (nbent > 0) launch_bonded_each<true>(bonded_kind(has_coul14, has_hybrid), x4o.p);
    const int nkb = cdiv(n, 256);
    hipLaunchKernelGGL(k_kinetic<R>, dim3(nkb), dim3(256), 0, stream, G, n, v4.p, ekout.p);
    std::vector<double> he, hk, hl;
    eout.download(he, 3 * (size_t)nb, stream); ekout.download(hk, 4 * (size_t)nkb, stream); elist.download(hl, CHEM_MAX_LISTS, stream);
    double acc[9 + CHEM_MAX_LISTS] = {0};   // elj, etab, vir, ek, px, py, pz, ecoul, lists..., vir coul
    for (int b = 0; b < nb; ++b) { acc[0] += he[3 * b]; acc[1] += he[3 * b + 1]; acc[2] += he[3 * b + 2]; }
    if (coul_on()) {
      std::vector<double> hq; eoutq.download(hq, 2 * (size_t)nb, stream);
      for (int b = 0; b < nb; ++b) { acc[7] += hq[2 * b]; acc[8 + CHEM_MAX_LISTS] += hq[2 * b + 1]; }
    }
    for (int b = 0; b < nkb; ++b) { acc[3] += hk[4 * b]; acc[4] += hk[4 * b + 1]; acc[5] += hk[4 * b + 2]; acc[6] += hk[4 * b + 3]; }
    for (int l = 0; l < CHEM_MAX_LISTS; ++l) acc[8 + l] = hl[l];
    allreduce_host_sums(acc, 9 + CHEM_MAX_LISTS, redbuf);
    out->step = step; out->npart = nglob; out->ekin = acc[3]; out->temperature = 2.0 * acc[3] / (3.0 * nglob);
    coul_epot = acc[7]; coul_virial = acc[8 + CHEM_MAX_LISTS];
    out->epot_lj = acc[0]; out->epot_tab = acc[1]; out->virial_nb = acc[2] + coul_virial;      // (sum over ALL non-bonded pairs)
    for (int k = 0; k < 3; ++k) out->momentum[k] = acc[4 + k];
    for (size_t l = 0; l < top.lists.size(); ++l) { out->epot_list[l] = acc[8 + l]; out->list_size[l] = top.lists[l].size(); }
  }

  int64_t verlet_pairs(int64_t* out, int64_t cap) override {
    flush_host_state();
    ensure_list32();
    compute_forces();   // the rebuild re-sorted the particles but not f4: keep it aligned for get_state(FORCE)
    const int ac = acap();
    std::vector<int> hn, ht, hl;
    nn.download(hn, ac, stream); tag.download(ht, ac, stream); nlist.download(hl, (size_t)ac * S, stream);
    std::vector<unsigned char> loc;
    for (int i = G; i < G + n; ++i)
      for (int k = 0; k < hn[i]; ++k) {
        const int a = ht[i], b = ht[hl[(size_t)i * S + k]];
        const int pr2[2] = {std::min(a, b), std::max(a, b)};
        const unsigned char* pb = reinterpret_cast<const unsigned char*>(pr2);
        loc.insert(loc.end(), pb, pb + 8);
      }
    const std::vector<unsigned char> all = gather_records(loc, 8);
    std::vector<std::pair<int64_t, int64_t>> pr;
    pr.reserve(all.size() / 8);
    for (size_t k = 0; k + 8 <= all.size(); k += 8) { int ab[2]; std::memcpy(ab, all.data() + k, 8); pr.emplace_back(top.id[ab[0]], top.id[ab[1]]); }
    std::sort(pr.begin(), pr.end());
    pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
    const int64_t m = (int64_t)pr.size();
    if (!out) return m;
    if (cap < m) throw ChemError(CHEM_ENOSPC, "verlet_pairs: capacity");
    for (int64_t k = 0; k < m; ++k) { out[2 * k] = pr[k].first; out[2 * k + 1] = pr[k].second; }
    return m;
  }

  void set_pair_bs(int v) override { pair_bs = v; }
  void debug_enable(int on) override {
    dbg_on = on != 0;
    if (dbg_on) { dbgbuf.alloc(6 * (size_t)std::max(ntiles, 1)); wgst.alloc(8 * (size_t)std::max(fused_grid, 1)); HIPCHK(hipMemsetAsync(wgst.p, 0, 8 * sizeof(long long) * (size_t)std::max(fused_grid, 1), stream)); }
  }
  // diagnostic / tests: the 16-bit force list of one particle as partner tags, in list order (padding dropped)
  int64_t debug_force_list(int tg, int32_t* out, int64_t cap) override {
    if (!use_tiles || !device_ready) return -1;
    HIPCHK(hipStreamSynchronize(stream));
    int p = -1; HIPCHK(hipMemcpy(&p, rtag.p + tg, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<TileLDS<R>> hd(ntiles);
    HIPCHK(hipMemcpy(hd.data(), tdesc.p, sizeof(TileLDS<R>) * (size_t)ntiles, hipMemcpyDeviceToHost));
    std::vector<int> htag; tag.download(htag, acap(), stream);
    for (int t = 0; t < ntiles; ++t) {
      const TileLDS<R>& T = hd[t];
      for (int sg = 0; sg < NHSEG; ++sg) {
        const int cnt = T.hoff[sg + 1] - T.hoff[sg];
        if (p < T.hstart[sg] || p >= T.hstart[sg] + cnt) continue;
        int q = T.hoff[sg] + (p - T.hstart[sg]);
        const int nhome = T.geom[4], hbase = T.geom[5];
        {      // row order: the position that holds this home's row
          std::vector<int> hw((size_t)nhome);
          HIPCHK(hipMemcpy(hw.data(), nnh.p + hbase, sizeof(int) * (size_t)nhome, hipMemcpyDeviceToHost));
          const auto it = std::find_if(hw.begin(), hw.end(), [q](int w) { return row_word_home(w) == q; });
          if (it == hw.end()) return -1;
          q = (int)(it - hw.begin());
        }
        int n16 = 0; HIPCHK(hipMemcpy(&n16, nnh.p + hbase + q, sizeof(int), hipMemcpyDeviceToHost));
        n16 = row_word_count(n16);
        int64_t m = 0;
        for (int c = 0; c * 8 < n16; ++c) {
          unsigned short ch[8];
          HIPCHK(hipMemcpy(ch, nl16.p + (size_t)hbase * S + ((size_t)c * nhome + q) * 8, 16, hipMemcpyDeviceToHost));
          for (int k = 0; k < 8 && c * 8 + k < n16; ++k) {
            const int sl = ch[k];
            int r = 0; while (r + 1 < NROW && sl >= T.rowoff[r + 1]) ++r;
            const int e = sl - T.rowoff[r];
            int kc = 0; for (int qq = 1; qq < SX; ++qq) kc += e >= T.celloff[r][qq] ? 1 : 0;
            const int j = T.cellg[r][kc] + (e - T.celloff[r][kc]);
            if (m < cap) out[m] = htag[j];
            ++m;
          }
        }
        return m;
      }
    }
    return -1;
  }
  // diagnostic / tests: the stored order of one tile's force-list rows -- out[0 .. nh) = entries of the row at every position,
  // out[nh .. 2 nh) = the home (index in the tile's cell-run order) it belongs to; returns nh, -1 without tiles
  int64_t debug_row_order(int tile, int32_t* out, int64_t cap) override {
    if (!use_tiles || !device_ready || tile < 0 || tile >= ntiles) return -1;
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<TileLDS<R>> hd(1);
    HIPCHK(hipMemcpy(hd.data(), tdesc.p + tile, sizeof(TileLDS<R>), hipMemcpyDeviceToHost));
    const int nh = hd[0].geom[4], hbase = hd[0].geom[5];
    if (!out) return nh;
    if (cap < 2 * (int64_t)nh) throw ChemError(CHEM_ENOSPC, "debug_row_order: capacity");
    if (nh > 0) HIPCHK(hipMemcpy(out, nnh.p + hbase, sizeof(int) * (size_t)nh, hipMemcpyDeviceToHost));
    for (int k = 0; k < nh; ++k) { const int w = out[k]; out[k] = row_word_count(w); out[nh + k] = row_word_home(w); }
    return nh;
  }
  int64_t debug_dump_rebuild(long long* out, int64_t cap) override {
    if (!dbg_on || !use_fused) return 0;
    std::vector<long long> h; wgst.download(h, 8 * (size_t)fused_grid, stream);
    const int64_t m = std::min<int64_t>(cap, (int64_t)h.size());
    std::copy(h.begin(), h.begin() + m, out);
    return m;
  }
  int64_t debug_dump(long long* out, int64_t cap) override {
    if (!dbg_on) return 0;
    std::vector<long long> h; dbgbuf.download(h, 6 * (size_t)ntiles, stream);
    const int64_t m = std::min<int64_t>(cap, (int64_t)h.size());
    std::copy(h.begin(), h.begin() + m, out);
    return m;
  }

  void refresh_timers() override {
    if (!device_ready || particles_dirty) return;
    std::vector<int> hn; (use_tiles ? nnh : nn).download(hn, acap(), stream);
    long long tot = 0;
    if (use_tiles) { for (int k = 0; k < n; ++k) tot += row_word_count(hn[k]); } else { for (int k = G; k < G + n; ++k) tot += hn[k]; }
    tm.nlist_entries = tot; tm.nlist_capacity = S;
  }

  void modify_particle(int t, int what, double value) override {
    if (!device_ready || particles_dirty) return;  // host mirror only; uploaded later
    int idx = 0;
    HIPCHK(hipMemcpyAsync(&idx, rtag.p + t, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    // a slab rank holds only its home particles and ghosts (rtag = -1 for every other tag): nothing to write there; a ghost
    // copy that does exist takes the new type / mass from its owner at the forced rebuild (resort)
    if ((what == CHEM_STATE_TYPE || what == CHEM_STATE_MASS) && idx < 0) return;
    if (what == CHEM_STATE_TYPE) { R w = (R)value; HIPCHK(hipMemcpyAsync(&x4.p[idx].w, &w, sizeof(R), hipMemcpyHostToDevice, stream)); }
    else if (what == CHEM_STATE_MASS) { R w = (R)value; HIPCHK(hipMemcpyAsync(&v4.p[idx].w, &w, sizeof(R), hipMemcpyHostToDevice, stream)); }
    else if (what == CHEM_STATE_STATE) { int w = (int)value; HIPCHK(hipMemcpyAsync(state.p + t, &w, sizeof(int), hipMemcpyHostToDevice, stream)); }
    else if (what == CHEM_STATE_RESID) { int w = (int)value; HIPCHK(hipMemcpyAsync(res_id.p + t, &w, sizeof(int), hipMemcpyHostToDevice, stream)); }
    else if (what == CHEM_STATE_CHARGE && charges_on() && qtag.p && !coul_dirty) { R w = (R)value; HIPCHK(hipMemcpyAsync(qtag.p + t, &w, sizeof(R), hipMemcpyHostToDevice, stream)); }   // (otherwise the host mirror alone: uploaded with the registration)
    HIPCHK(hipStreamSynchronize(stream));
  }
};

static std::string g_create_error;

}  // namespace chem

// =========================================================================================
// C ABI
// =========================================================================================
using namespace chem;

struct chem_ctx { std::unique_ptr<Ctx> c; };

#define CTX (*ctx->c)
#define API_BEGIN try { if (ctx && ctx->c) ctx->c->join_async();
#define API_BEGIN_NOJOIN try {
#define API_END(ctxp)                                                                  \
  } catch (const ChemError& e) { (ctxp)->c->err = e.what(); return e.code; }           \
    catch (const std::exception& e) { (ctxp)->c->err = e.what(); return CHEM_EINVAL; }
#define REQUIRE(cond, code, msg) do { if (!(cond)) throw ChemError((code), (msg)); } while (0)

// ---- checkpoints: the host data of a context as a CkptState and back (format, reader and writer: chem_ckpt_host.hpp) ----
static CkptFingerprint ckpt_fingerprint(const Ctx& c) {
  CkptFingerprint fp;
  for (const HostList& l : c.top.lists) fp.lists.push_back(CkptListKind{l.arity, l.kind, l.by_types, l.hybrid ? 1 : 0});
  fp.n_reactions = (int32_t)c.reactions.size(); fp.n_dissociations = (int32_t)c.dissociations.size(); fp.n_fix_sets = (int32_t)c.fix.sets.size();
  fp.atrp_on = c.atrp_on ? 1 : 0; fp.npart = c.top.n;
  return fp;
}
static int ckpt_baro_kind(const Ctx& c) { return c.piston_on() ? 2 : (c.baro_tau > 0 ? 1 : 0); }
// (the particle data is taken from the staging arrays: Ctx::ckpt_pull has filled them, or -- for the size alone -- zeros stand in)
static CkptState ckpt_collect(const Ctx& c) {
  const HostTopology& t = c.top;
  const size_t n = (size_t)t.n;
  CkptState s;
  s.step = c.step; for (int d = 0; d < 3; ++d) s.L[d] = c.L[d];
  s.react_on = c.react_on ? 1 : 0; s.ran = c.ran ? 1 : 0;
  s.baro_kind = ckpt_baro_kind(c); s.baro_p_last = c.baro_p_last; s.pist_pe = c.pist_pe; s.pist_eps = c.pist_eps; s.pist_sv = c.pist_sv; s.pist_mu = c.pist_mu;
  s.baro_charge = c.baro_charge; s.baro_charge_ref = c.baro_charge_ref;
  s.id = t.id; s.type = t.type; s.state = t.state; s.res_id = t.res_id; s.mol_id = t.mol_id; s.mass = t.mass; s.q = t.q;
  s.pos = c.pos0; s.vel = c.vel0; s.image = c.img0;
  s.pos.resize(3 * n, 0.0); s.vel.resize(3 * n, 0.0); s.image.resize(3 * n, 0);
  s.res_lambda0 = c.res.lambda0; s.res_s0 = c.res.s0; s.res_seen = c.res.seen;
  s.lists.resize(t.lists.size());
  for (size_t l = 0; l < t.lists.size(); ++l) { s.lists[l].ent = t.lists[l].ent; if (t.lists[l].hybrid) s.lists[l].birth = t.lists[l].birth; }
  for (const auto& e : t.excl_log) { s.excl.push_back(e.first); s.excl.push_back(e.second); }
  for (size_t a = 0; a < n; ++a) for (int32_t b : t.graph[a]) if ((size_t)b > a) { s.graph.push_back((int32_t)a); s.graph.push_back(b); }
  s.fix_sets.resize(c.fix.sets.size());
  for (size_t f = 0; f < c.fix.sets.size(); ++f) { s.fix_sets[f].next_seq = c.fix.sets[f].next_seq; s.fix_sets[f].ent = c.fix.sets[f].ent; }
  s.fix_log = c.fix.log; s.fix_joins = c.fix.join_log;
  for (const Ctx::RemovedRec& r : c.removed_log) s.removed.push_back(CkptRemoved{r.step, r.near, r.far, r.list, r.reaction});
  s.ev_a = c.arena.a; s.ev_b = c.arena.b; s.ev_r = c.arena.r; s.ev_d2 = c.arena.d2; s.ev_intra = c.arena.intra;
  for (const auto& b : c.arena.blocks) { s.ev_block_step.push_back(b.first); s.ev_block_first.push_back((uint64_t)b.second); }
  if (c.atrp_on) { s.atrp_ratio_activator = c.atrp.ratio_activator; s.atrp_ratio_deactivator = c.atrp.ratio_deactivator; }
  s.atrp_stats = c.atrp_stats;
  return s;
}
// The state goes into the host data and every dirty flag is raised: particles, labels, tables, lists and forces are built again
// from it at the next call that needs the device.  Both chem_checkpoint_load and chem_checkpoint_save end here.
static void ckpt_apply(Ctx& c, CkptState&& s) {
  HostTopology& t = c.top;
  const size_t n = (size_t)t.n;
  c.ckpt_reset();      // (first: it may still have to look at the device, and nothing has changed if it fails)
  c.step = s.step; t.cur_step = s.step; for (int d = 0; d < 3; ++d) c.L[d] = s.L[d];
  c.react_on = s.react_on != 0; c.ran = s.ran != 0;
  c.baro_p_last = s.baro_p_last; c.pist_pe = s.pist_pe; c.pist_eps = s.pist_eps; c.pist_sv = s.pist_sv; c.pist_mu = s.pist_mu;
  c.pist_pe_upload = c.pist_mu_upload = c.piston_on();      // (the device's words are written before they are read)
  c.region_keep = false; c.region_counted = s.step;
  c.baro_keep = false; c.baro_charge = s.baro_charge; c.baro_charge_ref = s.baro_charge_ref; c.baro_seen_builds = c.baro_seen_ref = -1;
  t.type = std::move(s.type); t.state = std::move(s.state); t.res_id = std::move(s.res_id); t.mol_id = std::move(s.mol_id); t.mass = std::move(s.mass); t.q = std::move(s.q);
  c.pos0 = std::move(s.pos); c.vel0 = std::move(s.vel); c.img0 = std::move(s.image);
  c.res.lambda0 = std::move(s.res_lambda0); c.res.s0 = std::move(s.res_s0); c.res.seen = std::move(s.res_seen);
  for (size_t li = 0; li < t.lists.size(); ++li) {
    HostList& l = t.lists[li];
    l.ent = std::move(s.lists[li].ent); l.birth = std::move(s.lists[li].birth);
    l.seen.clear();
    for (size_t e = 0; e + l.arity <= l.ent.size(); e += l.arity) l.seen.insert(tuple_key(&l.ent[e], l.arity));
  }
  t.excl.assign(n, TagRow()); t.excl_log.clear(); t.n_excl_pairs = 0;
  for (size_t e = 0; e + 1 < s.excl.size(); e += 2) {      // (the log as it was, a pair that entered it twice included; rows and count hold every pair once)
    const int32_t a = s.excl[e], b = s.excl[e + 1];
    t.excl_log.emplace_back(a, b);
    if (HostTopology::sorted_insert(t.excl[a], b)) { HostTopology::sorted_insert(t.excl[b], a); ++t.n_excl_pairs; }
  }
  t.graph.assign(n, TagRow());
  for (size_t e = 0; e + 1 < s.graph.size(); e += 2) t.graph_add(s.graph[e], s.graph[e + 1]);
  c.fix.targets.clear(); c.fix.anchors.clear();
  for (size_t f = 0; f < c.fix.sets.size(); ++f) {
    FixSet& fs = c.fix.sets[f];
    fs.next_seq = s.fix_sets[f].next_seq; fs.ent = std::move(s.fix_sets[f].ent);
    for (const FixEntry& e : fs.ent) { c.fix.targets.insert(e.target); ++c.fix.anchors[e.anchor]; }
  }
  c.fix.log = std::move(s.fix_log); c.fix.join_log = std::move(s.fix_joins);
  c.removed_log.clear();
  for (const CkptRemoved& r : s.removed) c.removed_log.push_back(Ctx::RemovedRec{r.step, r.near, r.far, r.list, r.reaction});
  c.arena.clear(); c.events.clear();
  c.arena.a = std::move(s.ev_a); c.arena.b = std::move(s.ev_b); c.arena.r = std::move(s.ev_r); c.arena.d2 = std::move(s.ev_d2); c.arena.intra = std::move(s.ev_intra);
  for (size_t b = 0; b < s.ev_block_step.size(); ++b) c.arena.blocks.emplace_back(s.ev_block_step[b], (size_t)s.ev_block_first[b]);
  c.arena.mirror_pos = c.arena.size();      // (the mirrors above are those behind the last event)
  if (c.atrp_on) { c.atrp.ratio_activator = s.atrp_ratio_activator; c.atrp.ratio_deactivator = s.atrp_ratio_deactivator; }
  c.atrp_stats = std::move(s.atrp_stats);
  c.particles_dirty = c.geom_dirty = c.pair_dirty = c.bonded_dirty = c.excl_dirty = c.labels_dirty = true; c.resort = true;
  c.coul_dirty = c.res_dirty = c.fix_dirty = true;
}

extern "C" {

int chem_abi_version(void) { return CHEM_ABI_VERSION; }

chem_ctx* chem_create(int device_id, int precision) {
  // an exception that escapes a helper thread or a destructor ends the process: say what it was before it does
  static std::once_flag term_once;
  std::call_once(term_once, [] {
    std::set_terminate([] {
      try { if (auto e = std::current_exception()) std::rethrow_exception(e); fprintf(stderr, "[libchem_mi355] std::terminate without an active exception (a joinable std::thread destroyed?)\n"); }
      catch (const std::exception& ex) { fprintf(stderr, "[libchem_mi355] std::terminate: uncaught exception: %s\n", ex.what()); }
      catch (...) { fprintf(stderr, "[libchem_mi355] std::terminate: uncaught exception of unknown type\n"); }
      std::abort();
    });
  });
  try {
    if (precision != CHEM_PREC_F32 && precision != CHEM_PREC_F64) throw ChemError(CHEM_EINVAL, "precision must be 32 or 64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw ChemError(CHEM_EDEVICE, "no HIP device available (libchem_mi355 has no CPU fall-back)");
    if (device_id < 0 || device_id >= ndev) throw ChemError(CHEM_EINVAL, "device id out of range");
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      throw ChemError(CHEM_EDEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    auto* h = new chem_ctx();
    if (precision == CHEM_PREC_F32) h->c.reset(new CtxT<float>()); else h->c.reset(new CtxT<double>());
    h->c->device = device_id; h->c->prec = precision;
    return h;
  } catch (const std::exception& e) { g_create_error = e.what(); return nullptr; }
}

void chem_destroy(chem_ctx* ctx) { delete ctx; }
const char* chem_last_error(chem_ctx* ctx) { return ctx ? ctx->c->err.c_str() : g_create_error.c_str(); }

int chem_set_box(chem_ctx* ctx, const double L[3]) {
  API_BEGIN
  for (int d = 0; d < 3; ++d) { REQUIRE(L[d] > 0, CHEM_EINVAL, "box edge must be positive"); CTX.L[d] = L[d]; }
  CTX.geom_dirty = true; CTX.resort = true;
  return 0;
  API_END(ctx)
}

int chem_set_cutoff(chem_ctx* ctx, double max_cutoff, double skin) {
  API_BEGIN
  REQUIRE(max_cutoff > 0 && skin >= 0, CHEM_EINVAL, "cutoff must be > 0 and skin >= 0");
  CTX.rc = max_cutoff; CTX.skin = skin; CTX.geom_dirty = true; CTX.resort = true;
  return 0;
  API_END(ctx)
}

int chem_set_dt(chem_ctx* ctx, double dt) { API_BEGIN REQUIRE(dt > 0, CHEM_EINVAL, "dt"); CTX.dt = dt; return 0; API_END(ctx) }

int chem_set_particles(chem_ctx* ctx, int64_t n, const int64_t* id, const int32_t* type, const double* pos, const double* vel,
                       const double* mass, const double* q, const int32_t* state, const int32_t* res_id) {
  API_BEGIN
  REQUIRE(n > 0 && id && type && pos && mass, CHEM_EINVAL, "set_particles: null or empty input");
  REQUIRE(n < (1ll << 27), CHEM_EINVAL, "set_particles: too many particles for one context");
  if (!res_id) for (int64_t i = 0; i < n; ++i) REQUIRE(fits_int32(id[i]), CHEM_EINVAL, "set_particles: the default res_id is the particle id, and id " + std::to_string(id[i]) + " does not fit its 32 bits: pass res_id");
  Ctx& c = CTX; HostTopology& t = c.top;
  std::vector<int64_t> order(n);
  for (int64_t i = 0; i < n; ++i) order[i] = i;
  bool sorted = true;
  for (int64_t i = 1; i < n; ++i) if (id[i] <= id[i - 1]) { sorted = false; break; }
  if (!sorted) std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return id[a] < id[b]; });
  t.n = n; t.id.resize(n); t.type.resize(n); t.state.resize(n); t.res_id.resize(n); t.mol_id.resize(n); t.mass.resize(n); t.q.resize(n);
  t.graph.assign(n, TagRow()); t.excl.assign(n, TagRow()); t.n_excl_pairs = 0; t.excl_log.clear(); t.id2tag.clear();
  for (auto& l : t.lists) { l.ent.clear(); l.seen.clear(); l.birth.clear(); }
  c.pos0.resize(3 * n); c.vel0.assign(3 * n, 0.0);
  t.contiguous = true; t.id0 = id[order[0]];
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = order[k];
    REQUIRE(k == 0 || id[s] != t.id[k - 1], CHEM_EINVAL, "duplicate particle id");
    REQUIRE(type[s] >= 0 && type[s] < CHEM_MAX_TYPES, CHEM_EINVAL, "particle type out of range [0,16)");
    REQUIRE(mass[s] > 0, CHEM_EINVAL, "particle mass must be positive");
    t.id[k] = id[s]; if (id[s] != t.id0 + k) t.contiguous = false;
    t.type[k] = type[s]; t.mass[k] = mass[s]; t.q[k] = q ? q[s] : 0.0;
    t.state[k] = state ? state[s] : 0; t.res_id[k] = res_id ? res_id[s] : (int32_t)id[s]; t.mol_id[k] = (int32_t)k;
    for (int d = 0; d < 3; ++d) { c.pos0[3 * k + d] = pos[3 * s + d]; if (vel) c.vel0[3 * k + d] = vel[3 * s + d]; }
  }
  if (!t.contiguous) for (int64_t k = 0; k < n; ++k) t.id2tag[t.id[k]] = (int32_t)k;
  c.particles_dirty = c.pair_dirty = c.bonded_dirty = c.excl_dirty = c.labels_dirty = true; c.resort = true;
  c.coul_dirty = true;
  c.res.clear(); c.res_dirty = true;      // (a new particle set: every lambda is 1 again; rates, marks and reaction rules stay)
  c.step = 0; c.events.clear(); c.arena.clear(); c.img0.clear();
  // (fixed distances: entries and log go with the tags; sets, post-processes and release rules stay)
  for (FixSet& fs : c.fix.sets) { fs.ent.clear(); fs.next_seq = 0; }
  c.fix.targets.clear(); c.fix.anchors.clear(); c.fix.log.clear(); c.fix.join_log.clear(); c.removed_log.clear(); c.fix_dirty = true; c.ran = false;
  c.region_log.clear(); c.region_stats.clear(); c.region_counted = 0; c.region_keep = false;      // (region rules and their switches stay)
  return 0;
  API_END(ctx)
}

int chem_add_particles(chem_ctx* ctx, int64_t n, const int64_t* id, const int32_t* type, const double* pos, const double* vel,
                       const double* mass, const double* q, const int32_t* state, const int32_t* res_id) {
  API_BEGIN
  Ctx& c = CTX; HostTopology& t = c.top;
  REQUIRE(t.n > 0, CHEM_ESTATE, "add_particles: set particles first");
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "add_particles is not available on the decomposed path");
  REQUIRE(c.step == 0 && !c.ran, CHEM_ESTATE, "add_particles: only at step 0 and before the first chem_run");
  REQUIRE(c.img0.empty(), CHEM_ESTATE, "add_particles: the context holds the staged state of a checkpoint (add the particles before chem_checkpoint_load)");
  REQUIRE(n > 0 && id && type && pos && mass, CHEM_EINVAL, "add_particles: null or empty input");
  REQUIRE(t.n + n < (1ll << 27), CHEM_EINVAL, "add_particles: too many particles for one context");
  std::vector<int64_t> order(n);
  for (int64_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return id[a] < id[b]; });
  const int64_t n0 = t.n, top_id = t.id[n0 - 1];
  REQUIRE(id[order[0]] > top_id, CHEM_EINVAL, "add_particles: every new id must be greater than the largest present id (" + std::to_string(top_id) + ")");
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = order[k];
    REQUIRE(k == 0 || id[s] != id[order[k - 1]], CHEM_EINVAL, "add_particles: duplicate particle id");
    REQUIRE(type[s] >= 0 && type[s] < CHEM_MAX_TYPES, CHEM_EINVAL, "add_particles: particle type out of range [0," + std::to_string(CHEM_MAX_TYPES) + "): CHEM_MAX_TYPES is the limit");
    REQUIRE(mass[s] > 0, CHEM_EINVAL, "add_particles: particle mass must be positive");
    REQUIRE(res_id || fits_int32(id[s]), CHEM_EINVAL, "add_particles: the default res_id is the particle id, and id " + std::to_string(id[s]) + " does not fit its 32 bits: pass res_id");
    for (int d = 0; d < 3; ++d) REQUIRE(std::isfinite(pos[3 * s + d]), CHEM_EINVAL, "add_particles: position");
  }
  c.add_particles_prepare();      // (nothing has failed so far; particle data back in pos0 / vel0 if it was on the device)
  const int64_t n1 = n0 + n;
  t.id.resize(n1); t.type.resize(n1); t.state.resize(n1); t.res_id.resize(n1); t.mol_id.resize(n1); t.mass.resize(n1); t.q.resize(n1);
  t.graph.resize(n1); t.excl.resize(n1);
  c.pos0.resize(3 * n1); c.vel0.resize(3 * n1, 0.0);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = order[k], g = n0 + k;
    t.id[g] = id[s]; if (id[s] != t.id0 + g) t.contiguous = false;
    t.type[g] = type[s]; t.mass[g] = mass[s]; t.q[g] = q ? q[s] : 0.0;
    t.state[g] = state ? state[s] : 0; t.res_id[g] = res_id ? res_id[s] : (int32_t)id[s]; t.mol_id[g] = (int32_t)g;
    for (int d = 0; d < 3; ++d) { c.pos0[3 * g + d] = pos[3 * s + d]; c.vel0[3 * g + d] = vel ? vel[3 * s + d] : 0.0; }
  }
  t.n = n1;
  if (!t.contiguous) { t.id2tag.clear(); for (int64_t k = 0; k < n1; ++k) t.id2tag[t.id[k]] = (int32_t)k; }
  if (c.res.on()) { c.res.lambda0.resize(n1, 1.0); c.res.s0.resize(n1, 0); c.res.seen.resize(n1); for (int64_t g = n0; g < n1; ++g) c.res.seen[g] = t.type[g]; }
  c.particles_dirty = c.pair_dirty = c.bonded_dirty = c.excl_dirty = c.labels_dirty = true; c.resort = true;
  c.coul_dirty = true; c.res_dirty = true; c.fix_dirty = true; c.geom_dirty = true;
  if (!c.restrict_map.empty()) c.restrict_dirty = true;      // (per-tag CSR)
  return 0;
  API_END(ctx)
}

int chem_fix_create(chem_ctx* ctx, int anchor_type, int target_type) {
  API_BEGIN
  REQUIRE(anchor_type >= -1 && anchor_type < CHEM_MAX_TYPES && target_type >= -1 && target_type < CHEM_MAX_TYPES, CHEM_EINVAL, "fix_create: type");
  const int h = CTX.fix.create(anchor_type, target_type);
  REQUIRE(h >= 0, CHEM_ENOSPC, "fix_create: a context holds at most " + std::to_string(CHEM_MAX_FIX_SETS) + " sets (CHEM_MAX_FIX_SETS)");
  return h;
  API_END(ctx)
}

int chem_fix_add(chem_ctx* ctx, int set, int64_t n, const int64_t* ids, double dist) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "fixed distances are not available on the decomposed path (anchor and target may sit on different ranks)");
  REQUIRE(c.top.n > 0, CHEM_ESTATE, "fix_add: set particles first");
  REQUIRE(n >= 0 && (ids || n == 0), CHEM_EINVAL, "fix_add: null input");
  std::vector<int32_t> tags((size_t)(2 * n));
  for (int64_t k = 0; k < 2 * n; ++k) tags[k] = (int32_t)c.top.tag_of(ids[k]);
  std::string why;
  const int rc = c.fix.add(set, n, tags.data(), dist, c.top.n, why);
  if (rc < 0) throw ChemError(rc, "fix_add: " + why);
  if (n) c.fix_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_fix_postprocess(chem_ctx* ctx, int set, int old_type, int new_type, double new_mass, double new_q, int new_state, double lambda) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(set >= 0 && set < (int)c.fix.sets.size(), CHEM_EINVAL, "fix_postprocess: unknown set");
  REQUIRE(old_type >= 0 && old_type < CHEM_MAX_TYPES && new_type < CHEM_MAX_TYPES, CHEM_EINVAL, "fix_postprocess: type");
  REQUIRE(new_type < 0 || (new_mass > 0 && std::isfinite(new_mass) && std::isfinite(new_q)), CHEM_EINVAL, "fix_postprocess: the new mass must be positive");
  REQUIRE(!(lambda > 1.0) && !std::isnan(lambda), CHEM_EINVAL, "fix_postprocess: lambda must lie in [0, 1] (negative: left alone)");
  c.fix.set_post(set, FixPost{old_type, new_type < 0 ? -1 : new_type, new_mass, new_q, new_state < 0 ? -1 : new_state, lambda < 0.0 ? -1.0 : lambda});
  c.pair_dirty = true;      // (the type count of the pair tables covers new_type)
  return 0;
  API_END(ctx)
}

int chem_reaction_release(chem_ctx* ctx, int reaction, int role, int set, int count) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "fixed distances are not available on the decomposed path");
  REQUIRE(c.assoc_row(reaction) >= 0, CHEM_EINVAL, "reaction_release: not an index of chem_reaction_add");
  REQUIRE(role == 1 || role == 2, CHEM_EINVAL, "reaction_release: role must be 1 or 2");
  REQUIRE(set >= 0 && set < (int)c.fix.sets.size(), CHEM_EINVAL, "reaction_release: unknown set");
  REQUIRE(count >= 1, CHEM_EINVAL, "reaction_release: count");
  c.fix.rules.push_back(FixRule{reaction, role, set, count});
  return 0;
  API_END(ctx)
}

int chem_reaction_join(chem_ctx* ctx, int reaction, int role, int set, double dist) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "fixed distances are not available on the decomposed path");
  REQUIRE(c.assoc_row(reaction) >= 0, CHEM_EINVAL, "reaction_join: not an index of chem_reaction_add");
  REQUIRE(role == 1 || role == 2, CHEM_EINVAL, "reaction_join: role must be 1 or 2");
  REQUIRE(set >= 0 && set < (int)c.fix.sets.size(), CHEM_EINVAL, "reaction_join: unknown set");
  REQUIRE(dist > 0.0 && std::isfinite(dist), CHEM_EINVAL, "reaction_join: the distance must be positive and finite");
  c.fix.joins.push_back(FixJoinRule{reaction, role, set, dist});
  return 0;
  API_END(ctx)
}

int64_t chem_fix_joins(chem_ctx* ctx, chem_fix_record* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t m = (int64_t)c.fix.join_log.size();
  if (!out) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "fix_joins: capacity");
  for (int64_t k = 0; k < m; ++k) { const FixRecord& r = c.fix.join_log[k]; out[k] = chem_fix_record{r.step, c.top.id[r.anchor], c.top.id[r.target], r.set, r.cause}; }
  return m;
  API_END(ctx)
}

int chem_reaction_remove_bond(chem_ctx* ctx, const chem_nb_remove* r) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "bond removal by a reaction is not available on the decomposed path");
  REQUIRE(r, CHEM_EINVAL, "reaction_remove_bond: null rule");
  const int row = c.assoc_row(r->reaction);
  REQUIRE(row >= 0, CHEM_EINVAL, "reaction_remove_bond: not an index of chem_reaction_add");
  REQUIRE(r->invoke_on >= 1 && r->invoke_on <= 3, CHEM_EINVAL, "reaction_remove_bond: invoke_on must be 1, 2 or 3");
  REQUIRE(r->nb_level >= 1, CHEM_EINVAL, "reaction_remove_bond: nb_level must be at least 1");
  for (int t : {r->anchor_type, r->type_1, r->type_2}) REQUIRE(t >= 0 && t < CHEM_MAX_TYPES, CHEM_EINVAL, "reaction_remove_bond: type");
  c.rm_rules.push_back(NbRemoveRule{row, r->invoke_on, r->anchor_type, r->nb_level, r->type_1, r->type_2, r->unexclude != 0 ? 1 : 0});
  return 0;
  API_END(ctx)
}

int64_t chem_reaction_removed(chem_ctx* ctx, chem_bond_record* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t m = (int64_t)c.removed_log.size();
  if (!out) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "reaction_removed: capacity");
  for (int64_t k = 0; k < m; ++k) { const Ctx::RemovedRec& r = c.removed_log[k]; out[k] = chem_bond_record{r.step, c.top.id[r.near], c.top.id[r.far], r.list, r.reaction}; }
  return m;
  API_END(ctx)
}

int64_t chem_fix_count(chem_ctx* ctx, int set) {
  API_BEGIN
  REQUIRE(set >= 0 && set < (int)CTX.fix.sets.size(), CHEM_EINVAL, "fix_count: unknown set");
  return (int64_t)CTX.fix.sets[set].ent.size();
  API_END(ctx)
}

int64_t chem_fix_get(chem_ctx* ctx, int set, int64_t* ids, double* dist, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(set >= 0 && set < (int)c.fix.sets.size(), CHEM_EINVAL, "fix_get: unknown set");
  const std::vector<FixEntry>& e = c.fix.sets[set].ent;
  const int64_t m = (int64_t)e.size();
  if (!ids && !dist) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "fix_get: capacity");
  for (int64_t k = 0; k < m; ++k) {
    if (ids) { ids[2 * k] = c.top.id[e[k].anchor]; ids[2 * k + 1] = c.top.id[e[k].target]; }
    if (dist) dist[k] = e[k].dist;
  }
  return m;
  API_END(ctx)
}

int64_t chem_fix_log(chem_ctx* ctx, chem_fix_record* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t m = (int64_t)c.fix.log.size();
  if (!out) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "fix_log: capacity");
  for (int64_t k = 0; k < m; ++k) { const FixRecord& r = c.fix.log[k]; out[k] = chem_fix_record{r.step, c.top.id[r.anchor], c.top.id[r.target], r.set, r.cause}; }
  return m;
  API_END(ctx)
}

int chem_modify_particle(chem_ctx* ctx, int64_t id, int what, double value) {
  API_BEGIN
  Ctx& c = CTX; const int t = c.top.tag_of(id);
  REQUIRE(t >= 0, CHEM_EINVAL, "modify_particle: unknown id");
  if (what == CHEM_STATE_LAMBDA) {
    REQUIRE(std::isfinite(value) && value >= 0.0 && value <= 1.0, CHEM_EINVAL, "modify_particle: lambda must lie in [0, 1]");
    c.res.ensure(c.top.type);
    c.res.stamp((size_t)t, value, c.step);
    c.res_push(std::vector<int32_t>{(int32_t)t});
    return 0;
  }
  if (what == CHEM_STATE_TYPE) {
    REQUIRE(value >= 0 && value < CHEM_MAX_TYPES, CHEM_EINVAL, "type"); c.top.type[t] = (int)value; c.pair_dirty = true; c.bonded_dirty = true; c.resort = true;
    if (c.res.on()) { std::vector<int32_t> ch; c.res.restamp_type_changes(c.top.type, c.step, ch); c.res_push(ch); }      // (re-stamped under the old type's rate)
  }
  else if (what == CHEM_STATE_STATE) c.top.state[t] = (int)value;
  else if (what == CHEM_STATE_MASS) { REQUIRE(value > 0, CHEM_EINVAL, "mass"); c.top.mass[t] = value; }
  else if (what == CHEM_STATE_RESID) c.top.res_id[t] = (int)value;
  else if (what == CHEM_STATE_CHARGE) c.top.q[t] = value;
  else throw ChemError(CHEM_EINVAL, "modify_particle: selector");
  c.modify_particle(t, what, value);
  return 0;
  API_END(ctx)
}

int chem_set_exclusions(chem_ctx* ctx, int64_t n, const int64_t* p) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(t.n > 0, CHEM_ESTATE, "set particles before exclusions");
  std::vector<int32_t> tags((size_t)(n > 0 ? 2 * n : 0));      // (every id is resolved before the old exclusions go: a refused call leaves them as they were)
  for (size_t k = 0; k < tags.size(); ++k) { tags[k] = t.tag_of(p[k]); REQUIRE(tags[k] >= 0, CHEM_EINVAL, "exclusion: unknown particle id " + std::to_string(p[k])); }
  for (auto& r : t.excl) r.clear();
  t.n_excl_pairs = 0; t.excl_log.clear();
  for (int64_t k = 0; k < n; ++k) t.exclude(tags[2 * k], tags[2 * k + 1]);
  CTX.excl_dirty = true; CTX.resort = true;
  return 0;
  API_END(ctx)
}

int chem_nb_lj(chem_ctx* ctx, int t1, int t2, double eps, double sig, double rc, int shift_auto) {
  API_BEGIN
  REQUIRE(t1 >= 0 && t2 >= 0 && t1 < CHEM_MAX_TYPES && t2 < CHEM_MAX_TYPES, CHEM_EINVAL, "nb_lj: type out of range");
  HostPairPot p; p.kind = (sig > 0 && rc > 0) ? 1 : 0; p.eps = eps; p.sig = sig; p.rc = rc;
  if (p.kind && shift_auto) { const double s2 = sig * sig / (rc * rc), s6 = s2 * s2 * s2; p.shift = -4.0 * eps * (s6 * s6 - s6); }
  CTX.pp[t1][t2] = p; CTX.pp[t2][t1] = p; CTX.pair_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_nb_coulomb(chem_ctx* ctx, int t1, int t2, double prefactor, double rc) {
  API_BEGIN
  REQUIRE(t1 >= 0 && t2 >= 0 && t1 < CHEM_MAX_TYPES && t2 < CHEM_MAX_TYPES, CHEM_EINVAL, "nb_coulomb: type out of range");
  Ctx& c = CTX;
  const bool was_on = c.coul_on();
  if (prefactor == 0 || !(rc > 0)) { c.coul_mask[t1] &= ~(1u << t2); c.coul_mask[t2] &= ~(1u << t1); }
  else {
    uint32_t others[CHEM_MAX_TYPES];
    for (int a = 0; a < CHEM_MAX_TYPES; ++a) others[a] = c.coul_mask[a];
    others[t1] &= ~(1u << t2); others[t2] &= ~(1u << t1);
    bool any = false;
    for (uint32_t m : others) any = any || m != 0;
    REQUIRE(!any || (prefactor == c.coul_k && rc == c.coul_rc), CHEM_ENOTIMPL,
            "nb_coulomb: every registered type pair must share one (prefactor, cutoff); registered " + std::to_string(c.coul_k) + ", " + std::to_string(c.coul_rc) +
            ", asked for " + std::to_string(prefactor) + ", " + std::to_string(rc) + " on type pair (" + std::to_string(t1) + "," + std::to_string(t2) + ")");
    c.coul_k = prefactor; c.coul_rc = rc;
    c.coul_mask[t1] |= 1u << t2; c.coul_mask[t2] |= 1u << t1;
  }
  // the type-pair mask of the force list, the kernel selection and the charge array follow the registration; switching the
  // term on or off also changes the LDS footprint the tiles are planned for
  c.pair_dirty = true; c.coul_dirty = true; c.bonded_dirty = true; c.resort = true;
  if (was_on != c.coul_on()) c.geom_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_nb_resolution(chem_ctx* ctx, int t1, int t2, int on, double max_force) {
  API_BEGIN
  REQUIRE(t1 >= 0 && t2 >= 0 && t1 < CHEM_MAX_TYPES && t2 < CHEM_MAX_TYPES, CHEM_EINVAL, "nb_resolution: type out of range");
  REQUIRE(std::isfinite(max_force), CHEM_EINVAL, "nb_resolution: max_force must be finite");
  Ctx& c = CTX;
  const bool was_on = c.res_pairs_on(), word_was = c.slot_word_on();
  if (on) {
    REQUIRE(c.pp[t1][t2].kind != 0, CHEM_EINVAL, "nb_resolution: type pair (" + std::to_string(t1) + "," + std::to_string(t2) + ") carries no LJ or table potential");
    REQUIRE(!(c.cap_rad[t1][t2] > 0), CHEM_EINVAL, "nb_resolution: type pair (" + std::to_string(t1) + "," + std::to_string(t2) + ") is capped (chem_nb_cap): a pair is capped or resolution-scaled, not both");
    c.res_mask[t1] |= 1u << t2; c.res_mask[t2] |= 1u << t1;
    c.res_fmax[t1][t2] = c.res_fmax[t2][t1] = max_force > 0 ? max_force : 0.0;
  } else {
    c.res_mask[t1] &= ~(1u << t2); c.res_mask[t2] &= ~(1u << t1);
    c.res_fmax[t1][t2] = c.res_fmax[t2][t1] = 0.0;
  }
  if (was_on || c.res_pairs_on()) {      // (switching off what was never on changes nothing and costs nothing)
    c.res_dirty = true; c.pair_dirty = true;
    if (was_on != c.res_pairs_on()) { c.bonded_dirty = true; c.resort = true; }      // kernel selection, inline bonds
    if (word_was != c.slot_word_on()) c.geom_dirty = true;      // the LDS footprint the tiles are planned for
  }
  return 0;
  API_END(ctx)
}

int chem_nb_cap(chem_ctx* ctx, int t1, int t2, double caprad) {
  API_BEGIN
  REQUIRE(t1 >= 0 && t2 >= 0 && t1 < CHEM_MAX_TYPES && t2 < CHEM_MAX_TYPES, CHEM_EINVAL, "nb_cap: type out of range");
  REQUIRE(std::isfinite(caprad), CHEM_EINVAL, "nb_cap: caprad must be finite");
  Ctx& c = CTX;
  const bool was_on = c.caps_on();
  const std::string pair = "(" + std::to_string(t1) + "," + std::to_string(t2) + ")";
  if (caprad > 0) {
    REQUIRE(c.pp[t1][t2].kind != 0, CHEM_EINVAL, "nb_cap: type pair " + pair + " carries no LJ or table potential");
    REQUIRE(caprad < c.pp[t1][t2].rc, CHEM_EINVAL, "nb_cap: caprad " + std::to_string(caprad) + " of type pair " + pair + " must lie inside its cutoff " + std::to_string(c.pp[t1][t2].rc));
    REQUIRE(!((c.res_mask[t1] >> t2) & 1u), CHEM_EINVAL, "nb_cap: type pair " + pair + " is resolution-marked: a pair is capped or resolution-scaled, not both");
    c.cap_rad[t1][t2] = c.cap_rad[t2][t1] = caprad;
  } else {
    c.cap_rad[t1][t2] = c.cap_rad[t2][t1] = 0.0;
  }
  if (was_on || c.caps_on()) {      // (removing what was never there changes nothing and costs nothing)
    c.cap_dirty = true; c.pair_dirty = true;
    if (was_on != c.caps_on()) { c.bonded_dirty = true; c.resort = true; c.geom_dirty = true; }      // kernel selection, inline bonds, the LDS footprint the tiles are planned for
  }
  return 0;
  API_END(ctx)
}

int chem_resolution_rate(chem_ctx* ctx, int type, double alpha, int new_type, double new_mass, double new_q, int new_state) {
  API_BEGIN
  REQUIRE(type >= 0 && type < CHEM_MAX_TYPES, CHEM_EINVAL, "resolution_rate: type out of range");
  REQUIRE(std::isfinite(alpha), CHEM_EINVAL, "resolution_rate: alpha must be finite");
  REQUIRE(new_type < CHEM_MAX_TYPES, CHEM_EINVAL, "resolution_rate: new type out of range");
  REQUIRE(!(alpha > 0 && new_type >= 0) || (new_mass > 0 && std::isfinite(new_mass) && std::isfinite(new_q)), CHEM_EINVAL, "resolution_rate: the new mass must be positive and finite, the new charge finite");
  Ctx& c = CTX;
  REQUIRE(c.top.n > 0, CHEM_ESTATE, "set particles before resolution_rate");
  if (!(alpha > 0) && !c.res.on()) return 0;      // removing what was never there
  c.res.ensure(c.top.type);
  std::vector<int32_t> changed;
  c.res.restamp_type_changes(c.top.type, c.step, changed);      // (types that moved while no rate was registered: lambda did not depend on them)
  ResRate r; r.alpha = alpha; r.new_type = new_type < 0 ? -1 : new_type; r.new_mass = new_mass; r.new_q = new_q; r.new_state = new_state < 0 ? -1 : new_state;
  c.res.set_rate(type, r, c.step, changed);
  c.res_dirty = true;      // (rates and stamps: uploaded whole)
  if (r.alpha > 0 && r.new_type >= 0) c.pair_dirty = true;      // (the type count may grow)
  return 0;
  API_END(ctx)
}

int chem_set_resolution(chem_ctx* ctx, int64_t n, const int64_t* ids, const double* lambda) {
  API_BEGIN
  REQUIRE(n >= 0 && (n == 0 || (ids && lambda)), CHEM_EINVAL, "set_resolution: null input");
  Ctx& c = CTX;
  std::vector<int32_t> tags((size_t)n);
  bool all_one = true;
  for (int64_t k = 0; k < n; ++k) {
    tags[k] = c.top.tag_of(ids[k]);
    REQUIRE(tags[k] >= 0, CHEM_EINVAL, "set_resolution: unknown id");
    REQUIRE(std::isfinite(lambda[k]) && lambda[k] >= 0.0 && lambda[k] <= 1.0, CHEM_EINVAL, "set_resolution: lambda must lie in [0, 1]");
    all_one = all_one && lambda[k] == 1.0;
  }
  if (n == 0 || (all_one && !c.res.on())) return 0;      // (every particle is at 1 already: nothing comes alive)
  c.res.ensure(c.top.type);
  for (int64_t k = 0; k < n; ++k) c.res.stamp((size_t)tags[k], lambda[k], c.step);
  c.res_push(tags);
  return 0;
  API_END(ctx)
}

int chem_reaction_set_resolution(chem_ctx* ctx, int reaction, int role, double lambda) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(reaction >= 0 && reaction < (int)c.pub_map.size(), CHEM_EINVAL, "reaction_set_resolution: unknown reaction index");
  REQUIRE(role == 1 || role == 2, CHEM_EINVAL, "reaction_set_resolution: role must be 1 or 2");
  REQUIRE(!(lambda > 1.0) && !std::isnan(lambda), CHEM_EINVAL, "reaction_set_resolution: lambda must lie in [0, 1] (negative: remove the rule)");
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "reaction_set_resolution is not available on the decomposed path (chem_comm_init*)");
  auto it = c.res_rules.find(reaction);
  if (lambda < 0.0) {
    if (it != c.res_rules.end()) { it->second[role - 1] = -1.0; if (it->second[0] < 0.0 && it->second[1] < 0.0) c.res_rules.erase(it); }
    return 0;
  }
  if (it == c.res_rules.end()) it = c.res_rules.emplace(reaction, std::array<double, 2>{-1.0, -1.0}).first;
  it->second[role - 1] = lambda;
  return 0;
  API_END(ctx)
}

int chem_get_coulomb(chem_ctx* ctx, double* epot, double* virial) {
  API_BEGIN
  chem_obs o;
  CTX.observe(&o);
  if (epot) *epot = CTX.coul_epot;
  if (virial) *virial = CTX.coul_virial;
  return 0;
  API_END(ctx)
}

int chem_get_pressure(chem_ctx* ctx, chem_pressure* out) { API_BEGIN REQUIRE(out, CHEM_EINVAL, "null output"); CTX.pressure(out); return 0; API_END(ctx) }
int chem_get_pressure_tensor(chem_ctx* ctx, chem_pressure_tensor* out) { API_BEGIN REQUIRE(out, CHEM_EINVAL, "null output"); CTX.pressure_tensor(out); return 0; API_END(ctx) }

int chem_barostat_berendsen(chem_ctx* ctx, double pressure, double tau) {
  API_BEGIN
  Ctx& c = CTX;
  if (!(tau > 0)) {      // off: nothing of it stays (lists that scalings have aged are built again first)
    if (c.piston_on()) return 0;      // (the other barostat is the one that is on: its state stays)
    c.baro_forget();
    c.baro_tau = 0; c.baro_p0 = 0;
    return 0;
  }
  REQUIRE(std::isfinite(pressure) && std::isfinite(tau), CHEM_EINVAL, "Berendsen barostat: pressure and tau must be finite");
  REQUIRE(!c.piston_on(), CHEM_EINVAL, "Berendsen barostat: the Langevin barostat is on (one barostat at a time: switch it off first, chem_barostat_langevin with mass 0)");
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "Berendsen barostat on a decomposed context: a gap of the decomposed path (the box of a slab cannot change)");
  c.baro_p0 = pressure; c.baro_tau = tau;
  return 0;
  API_END(ctx)
}

int chem_barostat_langevin(chem_ctx* ctx, double pressure, double mass, double gammaP, double kT, uint64_t seed) {
  API_BEGIN
  Ctx& c = CTX;
  if (!(mass > 0)) {      // off: nothing of it stays, the piston momentum included
    if (!c.piston_on()) return 0;      // (a Berendsen barostat that is on stays)
    c.baro_forget();
    c.pist_w = c.pist_gamma = c.pist_kT = 0; c.pist_seed = 0; c.baro_p0 = 0;
    c.pist_pe = c.pist_eps = 0; c.pist_sv = c.pist_mu = 1; c.pist_pe_upload = c.pist_mu_upload = false;
    return 0;
  }
  REQUIRE(std::isfinite(pressure) && std::isfinite(mass) && std::isfinite(gammaP) && std::isfinite(kT), CHEM_EINVAL, "Langevin barostat: pressure, mass, gammaP and kT must be finite");
  REQUIRE(gammaP >= 0 && kT >= 0, CHEM_EINVAL, "Langevin barostat: gammaP and kT must not be negative");
  REQUIRE(!(c.baro_tau > 0), CHEM_EINVAL, "Langevin barostat: the Berendsen barostat is on (one barostat at a time: switch it off first, chem_barostat_berendsen with tau 0)");
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "Langevin barostat on a decomposed context: a gap of the decomposed path (the box of a slab cannot change)");
  if (!c.piston_on()) { c.pist_pe = c.pist_eps = 0; c.pist_sv = c.pist_mu = 1; c.pist_pe_upload = true; c.pist_mu_upload = false; }      // switched on: the piston starts at rest
  else if (mass != c.pist_w && c.dt > 0) {      // the momentum survives; the factors of the next step follow the new mass
    const double nf = 3.0 * (double)c.top.n, sv = chem::piston_sv(c.pist_pe, mass, nf, c.dt), mu = chem::piston_mu(c.pist_pe, mass, c.dt);
    REQUIRE(chem::piston_ok(c.pist_pe, mu, sv), CHEM_EINVAL, "Langevin barostat: the piston momentum in force cannot be carried by this mass");
    c.pist_eps = c.pist_pe / mass; c.pist_sv = sv; c.pist_mu = mu; c.pist_mu_upload = true;      // (the device's copy of mu is the old mass's)
  }
  c.baro_p0 = pressure; c.pist_w = mass; c.pist_gamma = gammaP; c.pist_kT = kT; c.pist_seed = seed;
  return 0;
  API_END(ctx)
}

int chem_barostat_state_get(chem_ctx* ctx, chem_barostat_state* out) {
  API_BEGIN
  REQUIRE(out, CHEM_EINVAL, "null output");
  const Ctx& c = CTX;
  std::memset(out, 0, sizeof(*out));
  out->kind = c.piston_on() ? 2 : (c.baro_tau > 0 ? 1 : 0);
  out->pressure_last = c.baro_p_last; out->momentum = c.pist_pe; out->eps_dot = c.pist_eps; out->mu_next = c.pist_mu; out->sv_next = c.pist_sv;
  return 0;
  API_END(ctx)
}

int chem_get_box(chem_ctx* ctx, double L[3]) {
  API_BEGIN
  REQUIRE(L, CHEM_EINVAL, "null output");
  for (int d = 0; d < 3; ++d) L[d] = CTX.L[d];
  return 0;
  API_END(ctx)
}

int chem_nb_table(chem_ctx* ctx, int t1, int t2, int64_t nrow, double r0, double dr, const double* e, const double* f, double rc) {
  return chem_nb_table_interp(ctx, t1, t2, nrow, r0, dr, e, f, rc, TAB_LINEAR);
}

int chem_nb_table_interp(chem_ctx* ctx, int t1, int t2, int64_t nrow, double r0, double dr, const double* e, const double* f, double rc, int itype) {
  API_BEGIN
  REQUIRE(t1 >= 0 && t2 >= 0 && t1 < CHEM_MAX_TYPES && t2 < CHEM_MAX_TYPES, CHEM_EINVAL, "nb_table: type out of range");
  REQUIRE(itype >= TAB_LINEAR && itype <= TAB_CUBIC, CHEM_EINVAL, "nb_table: itype must be 1 (linear), 2 (Akima) or 3 (natural cubic spline)");
  REQUIRE(nrow >= 2 && dr > 0 && e && f && rc > 0, CHEM_EINVAL, "nb_table: need >=2 rows, dr>0");
  REQUIRE(tab_args_ok(itype, nrow), CHEM_EINVAL, "nb_table: the spline kinds (itype 2, 3) need >= 4 rows");
  HostPairPot p; p.kind = 2; p.itype = itype; p.rc = rc; p.r0 = r0; p.dr = dr; p.e.assign(e, e + nrow); p.f.assign(f, f + nrow);
  CTX.pp[t1][t2] = p; CTX.pp[t2][t1] = p; CTX.pair_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_list_create(chem_ctx* ctx, int arity, int kind, int by_types) {
  API_BEGIN
  REQUIRE(arity >= 2 && arity <= 4, CHEM_EINVAL, "list arity must be 2, 3 or 4");
  const bool ok = (arity == 2 && (kind == CHEM_POT_HARMONIC || kind == CHEM_POT_FENE || kind == CHEM_POT_TABULATED || kind == CHEM_POT_FENE_LJ || kind == CHEM_POT_LJ_BOND ||
                                  kind == CHEM_POT_COULOMB_BOND)) ||
                  (arity == 3 && (kind == CHEM_POT_ANG_HARMONIC || kind == CHEM_POT_ANG_COSINE || kind == CHEM_POT_ANG_TABULATED)) ||
                  (arity == 4 && (kind == CHEM_POT_DIH_NCOS || kind == CHEM_POT_DIH_RB || kind == CHEM_POT_DIH_TABULATED || kind == CHEM_POT_DIH_HARMONIC));
  REQUIRE(ok, CHEM_ENOTIMPL, "potential kind not supported for this arity");
  REQUIRE((int)CTX.top.lists.size() < CHEM_MAX_LISTS, CHEM_ENOSPC, "too many lists");
  HostList l; l.arity = arity; l.kind = kind; l.by_types = by_types ? 1 : 0;
  CTX.top.lists.push_back(std::move(l));
  if (kind == CHEM_POT_COULOMB_BOND) { CTX.coul_dirty = true; CTX.bonded_dirty = true; CTX.resort = true; }   // the charge array comes alive with the list; inline bonds go
  return (int)CTX.top.lists.size() - 1;
  API_END(ctx)
}

int chem_table_create(chem_ctx* ctx, int64_t nrow, double r0, double dr, const double* e, const double* f) {
  return chem_table_create_interp(ctx, nrow, r0, dr, e, f, TAB_LINEAR);
}

int chem_table_create_interp(chem_ctx* ctx, int64_t nrow, double r0, double dr, const double* e, const double* f, int itype) {
  API_BEGIN
  REQUIRE(itype >= TAB_LINEAR && itype <= TAB_CUBIC, CHEM_EINVAL, "table_create: itype must be 1 (linear), 2 (Akima) or 3 (natural cubic spline)");
  REQUIRE(nrow >= 2 && dr > 0 && e && f, CHEM_EINVAL, "table_create: need >= 2 rows, dr > 0");
  REQUIRE(tab_args_ok(itype, nrow), CHEM_EINVAL, "table_create: the spline kinds (itype 2, 3) need >= 4 rows");
  HostBondTable t; t.r0 = r0; t.dr = dr; t.itype = itype; t.e.assign(e, e + nrow); t.f.assign(f, f + nrow);
  CTX.top.btables.push_back(std::move(t));
  CTX.bonded_dirty = true;
  return (int)CTX.top.btables.size() - 1;
  API_END(ctx)
}

int chem_list_add(chem_ctx* ctx, int list, int64_t n, const int64_t* ids) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size(), CHEM_EINVAL, "list handle");
  REQUIRE(t.n > 0, CHEM_ESTATE, "set particles before list entries");
  HostList& l = t.lists[list];
  t.cur_step = CTX.step;
  std::vector<std::pair<int32_t, int32_t>> nb;
  std::vector<int32_t> tags((size_t)(n > 0 ? n : 0) * l.arity);      // (every id is resolved before the first entry goes in: a refused call leaves the list as it was)
  for (size_t k = 0; k < tags.size(); ++k) { tags[k] = t.tag_of(ids[k]); REQUIRE(tags[k] >= 0, CHEM_EINVAL, "list_add: unknown particle id " + std::to_string(ids[k])); }
  for (int64_t e = 0; e < n; ++e) {
    const int32_t* tg = &tags[(size_t)e * l.arity];
    if (t.list_insert(l, tg) && l.arity == 2) nb.emplace_back(tg[0], tg[1]);
  }
  for (auto& e : nb) t.graph_add(e.first, e.second);
  std::vector<int32_t> touched;
  for (auto& e : nb) if (t.mol_id[e.first] != t.mol_id[e.second]) t.merge_cluster(e.first, e.second, false, touched);
  CTX.bonded_dirty = true; CTX.labels_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_list_set_params(chem_ctx* ctx, int list, int t1, int t2, int t3, int t4, const double* p, int np) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size() && p && np >= 1 && np <= CHEM_MAX_POT_PARAMS, CHEM_EINVAL, "list_set_params");
  if (t.lists[list].kind == CHEM_POT_TABULATED || t.lists[list].kind == CHEM_POT_ANG_TABULATED || t.lists[list].kind == CHEM_POT_DIH_TABULATED)
    REQUIRE(p[0] >= 0 && p[0] < (double)t.btables.size() && p[0] == (double)(int)p[0], CHEM_EINVAL, "tabulated bonded terms: parameter must be a handle from chem_table_create");
  HostList& l = t.lists[list];
  if (l.kind == CHEM_POT_COULOMB_BOND)
    REQUIRE(np == 2 && std::isfinite(p[0]) && std::isfinite(p[1]) && p[1] > 0, CHEM_EINVAL, "1-4 Coulomb pairs: parameters are { prefactor, cutoff > 0 }, both finite");
  std::array<double, CHEM_MAX_POT_PARAMS> v{};
  std::copy(p, p + np, v.begin());
  if (!l.by_types) { l.plain = v; l.has_plain = true; }
  else {
    int tt[4] = {t1, t2, t3, t4};
    std::array<int, 4> key{-1, -1, -1, -1};
    for (int k = 0; k < l.arity; ++k) { REQUIRE(tt[k] >= 0 && tt[k] < CHEM_MAX_TYPES, CHEM_EINVAL, "type tuple"); key[k] = tt[k]; }
    l.typed[key] = v;
  }
  CTX.bonded_dirty = true;
  return 0;
  API_END(ctx)
}

int64_t chem_get_list(chem_ctx* ctx, int list, int64_t* out, int64_t cap) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size(), CHEM_EINVAL, "list handle");
  const HostList& l = t.lists[list];
  if (!out) return l.size();
  REQUIRE(cap >= l.size(), CHEM_ENOSPC, "get_list: capacity");
  for (size_t k = 0; k < l.ent.size(); ++k) out[k] = t.id[l.ent[k]];
  return l.size();
  API_END(ctx)
}

int chem_list_set_hybrid(chem_ctx* ctx, int list, double lambda0, double rate) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size(), CHEM_EINVAL, "list handle");
  const int rc = t.lists[list].set_hybrid(lambda0, rate);
  REQUIRE(rc != CHEM_EINVAL, CHEM_EINVAL, "list_set_hybrid: needs a pair list, lambda0 in [0, 1] and a finite rate >= 0");
  REQUIRE(rc != CHEM_ESTATE, CHEM_ESTATE, "list_set_hybrid: the list already has entries (their birth steps are unknown)");
  CTX.bonded_dirty = true; CTX.resort = true;      // (a context with a hybrid list leaves the inline-bond mode: rebuild)
  return 0;
  API_END(ctx)
}

int chem_list_set_hybrid_tuples(chem_ctx* ctx, int list, double lambda0, double rate) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size(), CHEM_EINVAL, "list handle");
  REQUIRE(t.lists[list].arity != 2, CHEM_EINVAL, "list_set_hybrid_tuples: needs a triple or quadruple list (pair lists: chem_list_set_hybrid)");
  const int rc = t.lists[list].set_hybrid_tuples(lambda0, rate);
  REQUIRE(rc != CHEM_EINVAL, CHEM_EINVAL, "list_set_hybrid_tuples: needs lambda0 in [0, 1] and a finite rate >= 0");
  REQUIRE(rc != CHEM_ESTATE, CHEM_ESTATE, "list_set_hybrid_tuples: the list already has entries (their birth steps are unknown)");
  CTX.bonded_dirty = true; CTX.resort = true;      // (as chem_list_set_hybrid: the bonded kernels of the hybrid family from the next launch on)
  return 0;
  API_END(ctx)
}

int64_t chem_list_get_lambda(chem_ctx* ctx, int list, double* out, int64_t cap) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size(), CHEM_EINVAL, "list handle");
  const HostList& l = t.lists[list];
  if (!out) return l.size();
  REQUIRE(cap >= l.size(), CHEM_ENOSPC, "list_get_lambda: capacity");
  for (int64_t e = 0; e < l.size(); ++e) out[e] = l.lambda_at((size_t)e, CTX.step);
  return l.size();
  API_END(ctx)
}

int chem_thermostat_langevin(chem_ctx* ctx, double kT, double gamma, uint64_t seed) {
  API_BEGIN
  CTX.lang = gamma > 0 && kT >= 0; CTX.kT = kT; CTX.gamma = gamma; CTX.lang_seed = seed;
  return 0;
  API_END(ctx)
}

int chem_thermostat_langevin_types(chem_ctx* ctx, int n, const int32_t* types) {
  API_BEGIN
  REQUIRE(n >= 0 && (n == 0 || types), CHEM_EINVAL, "thermal groups");
  uint32_t m = 0;
  for (int k = 0; k < n; ++k) { REQUIRE(types[k] >= 0 && types[k] < CHEM_MAX_TYPES, CHEM_EINVAL, "thermal group type id"); m |= 1u << types[k]; }
  CTX.lang_tmask = m;
  return 0;
  API_END(ctx)
}

int chem_thermostat_rescale(chem_ctx* ctx, int kind, double kT, double param) {
  API_BEGIN
  REQUIRE(kind >= 0 && kind <= 2, CHEM_EINVAL, "thermostat_rescale: kind must be 0 (off), 1 (Berendsen) or 2 (Isokinetic)");
  if (kind) REQUIRE(kT > 0, CHEM_EINVAL, "thermostat_rescale: temperature");
  if (kind == 1) REQUIRE(param > 0, CHEM_EINVAL, "Berendsen: tau must be > 0");
  if (kind == 2) REQUIRE(param >= 1, CHEM_EINVAL, "Isokinetic: coupling must be >= 1 step");
  CTX.resc_kind = kind; CTX.resc_kT = kT; CTX.resc_param = kind == 2 ? std::floor(param) : param;
  return 0;
  API_END(ctx)
}

int chem_thermostat_svr(chem_ctx* ctx, double kT, double coupling, uint64_t seed) {
  API_BEGIN
  if (coupling > 0) REQUIRE(kT > 0, CHEM_EINVAL, "thermostat_svr: temperature");
  CTX.resc_kind = coupling > 0 ? 3 : 0; CTX.resc_kT = kT; CTX.resc_param = coupling; CTX.svr_seed = seed;
  return 0;
  API_END(ctx)
}

int chem_cap_force(chem_ctx* ctx, double max_force) { API_BEGIN CTX.cap_force = max_force > 0 ? max_force : 0; return 0; API_END(ctx) }

int chem_reaction_init(chem_ctx* ctx, int interval, int nearest, int max_per_interval, uint64_t seed) {
  API_BEGIN
  REQUIRE(interval > 0, CHEM_EINVAL, "reaction interval must be positive");
  CTX.react_init = true; CTX.interval = interval; CTX.nearest = nearest ? 1 : 0; CTX.react_seed = seed;
  CTX.max_per_interval = max_per_interval > 0 ? max_per_interval : 0;
  return 0;
  API_END(ctx)
}

int chem_reaction_add(chem_ctx* ctx, const chem_reaction_desc* d) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(c.react_init, CHEM_ESTATE, "chem_reaction_init first");
  REQUIRE(d, CHEM_EINVAL, "null descriptor");
  REQUIRE((int)c.reactions.size() < CHEM_MAX_REACTIONS, CHEM_ENOSPC, "too many reactions");
  REQUIRE(d->type_1 >= 0 && d->type_1 < CHEM_MAX_TYPES && d->type_2 >= 0 && d->type_2 < CHEM_MAX_TYPES, CHEM_EINVAL, "reaction types");
  REQUIRE(d->new_type_1 < CHEM_MAX_TYPES && d->new_type_2 < CHEM_MAX_TYPES, CHEM_EINVAL, "reaction new types");
  REQUIRE(d->cutoff > 0 && d->cutoff <= c.rc + 1e-12, CHEM_EINVAL, "reaction cutoff must be in (0, max_cutoff]: candidates come from the Verlet list");
  if (!d->is_virtual) REQUIRE(d->bond_list >= 0 && d->bond_list < (int)c.top.lists.size() && c.top.lists[d->bond_list].arity == 2, CHEM_EINVAL, "reaction bond_list must be an arity-2 list");
  if (d->new_type_1 >= 0) REQUIRE(d->new_mass_1 > 0, CHEM_EINVAL, "new_mass_1");
  if (d->new_type_2 >= 0) REQUIRE(d->new_mass_2 > 0, CHEM_EINVAL, "new_mass_2");
  c.reactions.push_back(*d); c.pair_dirty = true;
  c.pub_map.push_back((int)c.reactions.size() - 1); c.assoc_pub.push_back((int)c.pub_map.size() - 1);
  return (int)c.pub_map.size() - 1;
  API_END(ctx)
}

int chem_dissociation_add(chem_ctx* ctx, const chem_dissociation_desc* d) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(c.react_init, CHEM_ESTATE, "chem_reaction_init first");
  REQUIRE(d, CHEM_EINVAL, "null descriptor");
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "dissociation reactions are not available on the decomposed path (chem_comm_init*)");
  REQUIRE((int)c.dissociations.size() < CHEM_MAX_REACTIONS && c.pub_map.size() < 256, CHEM_ENOSPC, "too many reactions");
  REQUIRE(d->type_1 >= 0 && d->type_1 < CHEM_MAX_TYPES && d->type_2 >= 0 && d->type_2 < CHEM_MAX_TYPES, CHEM_EINVAL, "dissociation types");
  REQUIRE(d->new_type_1 < CHEM_MAX_TYPES && d->new_type_2 < CHEM_MAX_TYPES, CHEM_EINVAL, "dissociation new types");
  REQUIRE(d->diss_rate >= 0, CHEM_EINVAL, "diss_rate must not be negative");
  REQUIRE(d->bond_list >= 0 && d->bond_list < (int)c.top.lists.size() && c.top.lists[d->bond_list].arity == 2, CHEM_EINVAL, "dissociation bond_list must be an arity-2 list");
  if (d->new_type_1 >= 0) REQUIRE(d->new_mass_1 > 0, CHEM_EINVAL, "new_mass_1");
  if (d->new_type_2 >= 0) REQUIRE(d->new_mass_2 > 0, CHEM_EINVAL, "new_mass_2");
  c.dissociations.push_back(*d); c.pair_dirty = true;
  c.pub_map.push_back(~((int)c.dissociations.size() - 1)); c.diss_pub.push_back((int)c.pub_map.size() - 1);
  return (int)c.pub_map.size() - 1;
  API_END(ctx)
}

int chem_reaction_neighbour_change(chem_ctx* ctx, const chem_nb_change* r) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(r, CHEM_EINVAL, "null rule");
  REQUIRE(c.assoc_row(r->reaction) >= 0, CHEM_EINVAL, "neighbour_change: reaction index");
  REQUIRE(r->invoke_on >= 1 && r->invoke_on <= 3 && r->nb_level >= 1, CHEM_EINVAL, "neighbour_change: invoke_on must be 1, 2 or 3 and nb_level >= 1");
  REQUIRE(r->old_type >= 0 && r->old_type < CHEM_MAX_TYPES && r->new_type >= 0 && r->new_type < CHEM_MAX_TYPES, CHEM_EINVAL, "neighbour_change: types");
  REQUIRE(r->new_mass > 0, CHEM_EINVAL, "neighbour_change: new_mass");
  c.nb_rules.push_back(*r); c.nb_rules.back().reaction = c.assoc_row(r->reaction); c.pair_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_reaction_constraint(chem_ctx* ctx, int reaction, int role, int nb_type, int min_state, int max_state) {
  API_BEGIN
  Ctx& c = CTX;
  reaction = c.assoc_row(reaction);
  REQUIRE(reaction >= 0 && reaction < (int)c.reactions.size() && reaction < 32, CHEM_EINVAL, "reaction_constraint: reaction index");
  REQUIRE((role == 1 || role == 2) && nb_type >= 0 && nb_type < CHEM_MAX_TYPES, CHEM_EINVAL, "reaction_constraint: role must be 1 or 2, nb_type a type id");
  if (c.constraints.size() < c.reactions.size()) c.constraints.resize(c.reactions.size());
  c.constraints[reaction] = NbCons{role, nb_type, min_state, max_state};
  return 0;
  API_END(ctx)
}

int chem_reaction_restrict(chem_ctx* ctx, int reaction, int64_t n, const int64_t* p) {
  API_BEGIN
  Ctx& c = CTX;
  reaction = c.assoc_row(reaction);
  REQUIRE(reaction >= 0 && reaction < (int)c.reactions.size() && reaction < 32, CHEM_EINVAL, "reaction_restrict: reaction index");
  REQUIRE(n >= 0 && (n == 0 || p), CHEM_EINVAL, "reaction_restrict: pairs");
  for (int64_t k = 0; k < n; ++k) {      // (every pair is checked before the first one counts: a refused call leaves the reaction as it was)
    const int a = c.top.tag_of(p[2 * k]), b = c.top.tag_of(p[2 * k + 1]);
    REQUIRE(a >= 0 && b >= 0 && a != b, CHEM_EINVAL, "reaction_restrict: unknown id or self pair");
  }
  for (int64_t k = 0; k < n; ++k) {
    const int a = c.top.tag_of(p[2 * k]), b = c.top.tag_of(p[2 * k + 1]);
    c.restrict_map[{std::min(a, b), std::max(a, b)}] |= 1u << reaction;
  }
  c.restricted_mask |= 1u << reaction; c.restrict_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_atrp_init(chem_ctx* ctx, const chem_atrp_desc* d) {
  API_BEGIN
  Ctx& c = CTX;
  if (!d) { c.atrp_on = false; return 0; }
  REQUIRE(d->interval > 0 && d->num_particles > 0, CHEM_EINVAL, "atrp_init: interval and num_particles must be positive");
  REQUIRE(d->ratio_activator >= 0 && d->ratio_deactivator >= 0 && d->delta_catalyst >= 0 && d->k_activate >= 0 && d->k_deactivate >= 0, CHEM_EINVAL, "atrp_init: negative rate or ratio");
  c.atrp = *d; c.atrp_on = true;
  return 0;
  API_END(ctx)
}

int chem_atrp_add_center(chem_ctx* ctx, int type, int state, int is_activator, int new_type, double new_mass, double new_q, int delta_state) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(type >= 0 && type < CHEM_MAX_TYPES && new_type < CHEM_MAX_TYPES, CHEM_EINVAL, "atrp_add_center: types");
  REQUIRE(new_type < 0 || new_mass > 0, CHEM_EINVAL, "atrp_add_center: new_mass");
  c.atrp_centers.push_back(AtrpCenter{type, state, is_activator ? 1 : 0, new_type, delta_state, new_mass, new_q});
  c.pair_dirty = true;    // (the type-pair tables must cover the new type)
  return 0;
  API_END(ctx)
}

int64_t chem_atrp_get_stats(chem_ctx* ctx, chem_atrp_stats* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t n = (int64_t)c.atrp_stats.size();
  if (!out) return n;
  REQUIRE(cap >= n, CHEM_ENOSPC, "atrp stats capacity");
  std::copy(c.atrp_stats.begin(), c.atrp_stats.end(), out);
  return n;
  API_END(ctx)
}

// ---- region rules (rule set in the header; chem_region_host.hpp) ----
int chem_region_add(chem_ctx* ctx, const chem_region_desc* d) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "region rules are not available on the decomposed path (a selection by count would need a gather across ranks)");
  REQUIRE(d, CHEM_EINVAL, "region_add: null descriptor");
  std::string why;
  if (region_validate(*d, why) != 0) throw ChemError(CHEM_EINVAL, "region_add: " + why);
  REQUIRE((int)c.regions.size() < CHEM_MAX_REGIONS, CHEM_ENOSPC, "region_add: more than CHEM_MAX_REGIONS rules");
  c.regions.push_back(*d); c.region_enabled.push_back(0);
  c.pair_dirty = true;    // (the type-pair tables must cover the new type)
  return (int)c.regions.size() - 1;
  API_END(ctx)
}

int chem_region_enable(chem_ctx* ctx, int rule, int on) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(rule >= 0 && rule < (int)c.regions.size(), CHEM_EINVAL, "region_enable: unknown rule");
  c.region_enabled[rule] = on ? 1 : 0;
  return 0;
  API_END(ctx)
}

int64_t chem_region_get_changes(chem_ctx* ctx, chem_region_change* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t m = (int64_t)c.region_log.size();
  if (!out) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "region_get_changes: capacity");
  for (int64_t k = 0; k < m; ++k) { const RegionChange& r = c.region_log[k]; out[k] = chem_region_change{r.step, c.top.id[r.tag], r.rule, 0}; }
  return m;
  API_END(ctx)
}

int64_t chem_region_get_stats(chem_ctx* ctx, chem_region_stats* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t m = (int64_t)c.region_stats.size();
  if (!out) return m;
  REQUIRE(cap >= m, CHEM_ENOSPC, "region_get_stats: capacity");
  for (int64_t k = 0; k < m; ++k) { const RegionStat& r = c.region_stats[k]; out[k] = chem_region_stats{r.step, (int64_t)r.rule, r.candidates, r.changed}; }
  return m;
  API_END(ctx)
}

int chem_region_counters(chem_ctx* ctx, int64_t* firings, int64_t* syncs) {
  API_BEGIN
  if (firings) *firings = CTX.region_firings;
  if (syncs) *syncs = CTX.region_syncs;
  return 0;
  API_END(ctx)
}

int chem_topology_register(chem_ctx* ctx, int arity, int list, const int32_t* types) {
  API_BEGIN
  HostTopology& t = CTX.top;
  REQUIRE(list >= 0 && list < (int)t.lists.size() && t.lists[list].arity == arity && types, CHEM_EINVAL, "topology_register");
  std::array<int, 4> key{-1, -1, -1, -1};
  for (int k = 0; k < arity; ++k) key[k] = types[k];
  t.lists[list].registered.push_back(key);
  return 0;
  API_END(ctx)
}

int chem_reactions_enable(chem_ctx* ctx, int on) { API_BEGIN CTX.react_on = on != 0; return 0; API_END(ctx) }

int chem_reaction_set_rate(chem_ctx* ctx, int r, double rate) {
  API_BEGIN
  REQUIRE(r >= 0 && r < (int)CTX.pub_map.size(), CHEM_EINVAL, "reaction index");
  const int row = CTX.pub_map[r];
  if (row >= 0) CTX.reactions[row].rate = rate;
  else { REQUIRE(rate >= 0, CHEM_EINVAL, "diss_rate must not be negative"); CTX.dissociations[~row].diss_rate = rate; }
  return 0;
  API_END(ctx)
}

int64_t chem_checkpoint_save(chem_ctx* ctx, void* buf, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "checkpoint_save on a decomposed context: a gap of the decomposed path (the state lives on several ranks)");
  REQUIRE(c.top.n > 0, CHEM_ESTATE, "checkpoint_save: set particles first");
  if (!buf) return (int64_t)ckpt_write(c.prec, ckpt_fingerprint(c), ckpt_collect(c)).size();      // (the size depends on counts alone: the device is not asked)
  REQUIRE(cap >= 0, CHEM_EINVAL, "checkpoint_save: capacity");
  {      // refused before anything is touched
    const int64_t need = (int64_t)ckpt_write(c.prec, ckpt_fingerprint(c), ckpt_collect(c)).size();
    REQUIRE(cap >= need, CHEM_ENOSPC, "checkpoint_save: capacity " + std::to_string(cap) + " is less than the " + std::to_string(need) + " bytes the blob needs");
  }
  c.ckpt_pull();
  CkptState s = ckpt_collect(c);
  const std::vector<uint8_t> blob = ckpt_write(c.prec, ckpt_fingerprint(c), s);
  REQUIRE((int64_t)blob.size() <= cap, CHEM_ENOSPC, "checkpoint_save: capacity");
  std::memcpy(buf, blob.data(), blob.size());
  ckpt_apply(c, std::move(s));      // the context goes on from the blob's data, exactly as one that loads it
  return (int64_t)blob.size();
  API_END(ctx)
}

int chem_checkpoint_load(chem_ctx* ctx, const void* buf, int64_t nbytes) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(!c.dd_on, CHEM_ENOTIMPL, "checkpoint_load on a decomposed context: a gap of the decomposed path (the state lives on several ranks)");
  REQUIRE(c.top.n > 0, CHEM_ESTATE, "checkpoint_load: set the context up first, chem_set_particles with the ids of the saved one included");
  REQUIRE(buf && nbytes >= 0, CHEM_EINVAL, "checkpoint_load: no blob");
  CkptState s; std::string why;
  const int rc = ckpt_read(buf, nbytes, c.prec, ckpt_fingerprint(c), s, why);
  if (rc != 0) throw ChemError(rc, why);
  for (size_t t = 0; t < s.id.size(); ++t)
    REQUIRE(s.id[t] == c.top.id[t], CHEM_EINVAL, "checkpoint: the particle ids differ from the context's (tag " + std::to_string(t) + ": blob " + std::to_string(s.id[t]) + ", context " + std::to_string(c.top.id[t]) + ")");
  REQUIRE(s.baro_kind == ckpt_baro_kind(c), CHEM_EINVAL, "checkpoint: the configuration differs from the one the blob was saved under: barostat kind (blob " + std::to_string(s.baro_kind) +
                                                          ", context " + std::to_string(ckpt_baro_kind(c)) + ")");
  ckpt_apply(c, std::move(s));
  c.region_log.clear(); c.region_stats.clear();      // (not part of a blob: from here on they hold what happens since the load)
  return 0;
  API_END(ctx)
}

int chem_rdf_init(chem_ctx* ctx, double r_max, int nbins, int npairs, const int32_t* type_pairs, int split_molecules) {
  API_BEGIN
  Ctx& c = CTX;
  std::string why;
  if (rdf_validate(r_max, nbins, npairs, type_pairs, why) != 0) throw ChemError(CHEM_EINVAL, why);
  Ctx::RdfConf r;
  if (npairs > 0) {
    r.on = true; r.r_max = r_max; r.nbins = nbins; r.npairs = npairs; r.split = split_molecules ? 1 : 0;
    for (int k = 0; k < 2 * npairs; ++k) r.tp[k] = type_pairs[k];
  }
  c.rdf = r;      // (in-run sampling is off again: the accumulators start from nothing)
  c.rdf_configure();
  return 0;
  API_END(ctx)
}
int chem_rdf_sample(chem_ctx* ctx) { API_BEGIN REQUIRE(CTX.rdf.on, CHEM_ESTATE, "rdf_sample before chem_rdf_init"); CTX.rdf_sample(); return 0; API_END(ctx) }
int chem_rdf_sample_every(chem_ctx* ctx, int every) {
  API_BEGIN
  REQUIRE(CTX.rdf.on, CHEM_ESTATE, "rdf_sample_every before chem_rdf_init");
  CTX.rdf.every = every > 0 ? every : 0;
  return 0;
  API_END(ctx)
}
int chem_rdf_get(chem_ctx* ctx, chem_rdf_result* out, uint64_t* counts, int64_t cap) {
  API_BEGIN
  REQUIRE(CTX.rdf.on, CHEM_ESTATE, "rdf_get before chem_rdf_init");
  REQUIRE(out, CHEM_EINVAL, "null output");
  CTX.rdf_get(out, counts, cap);
  return 0;
  API_END(ctx)
}
int chem_rdf_reset(chem_ctx* ctx) { API_BEGIN REQUIRE(CTX.rdf.on, CHEM_ESTATE, "rdf_reset before chem_rdf_init"); CTX.rdf_reset(); return 0; API_END(ctx) }

int chem_sq_init(chem_ctx* ctx, int nmax, int npairs, const int32_t* type_pairs) {
  API_BEGIN
  Ctx& c = CTX;
  std::string why;
  if (sq_validate(nmax, npairs, type_pairs, why) != 0) throw ChemError(CHEM_EINVAL, why);
  Ctx::SqConf q;
  if (npairs > 0) {
    q.on = true; q.nmax = nmax; q.npairs = npairs;
    for (int k = 0; k < 2 * npairs; ++k) q.tp[k] = type_pairs[k];
  }
  c.sq = q;      // (in-run sampling is off again: the accumulators start from nothing)
  c.sq_configure();
  return 0;
  API_END(ctx)
}
int chem_sq_sample(chem_ctx* ctx) { API_BEGIN REQUIRE(CTX.sq.on, CHEM_ESTATE, "sq_sample before chem_sq_init"); CTX.sq_sample(); return 0; API_END(ctx) }
int chem_sq_sample_every(chem_ctx* ctx, int every) {
  API_BEGIN
  REQUIRE(CTX.sq.on, CHEM_ESTATE, "sq_sample_every before chem_sq_init");
  CTX.sq.every = every > 0 ? every : 0;
  return 0;
  API_END(ctx)
}
int chem_sq_get(chem_ctx* ctx, chem_sq_result* out, double* sums, int64_t cap) {
  API_BEGIN
  REQUIRE(CTX.sq.on, CHEM_ESTATE, "sq_get before chem_sq_init");
  REQUIRE(out, CHEM_EINVAL, "null output");
  CTX.sq_get(out, sums, cap);
  return 0;
  API_END(ctx)
}
int chem_sq_reset(chem_ctx* ctx) { API_BEGIN REQUIRE(CTX.sq.on, CHEM_ESTATE, "sq_reset before chem_sq_init"); CTX.sq_reset(); return 0; API_END(ctx) }

int chem_run(chem_ctx* ctx, int64_t nsteps) {
  API_BEGIN_NOJOIN   // a pending label merge keeps running beside the MD steps; react_step joins it
  REQUIRE(nsteps >= 0, CHEM_EINVAL, "nsteps");
  // a pair cutoff beyond the list cutoff (max_cutoff) would make the forces depend on the list's own radius (list_skin): the
  // reference builds its Verlet list at the largest pair cutoff (start_simulation.py:80,193-197), so it never asks for this.
  // (Without a cutoff the system is incomplete: CTX.run reports that, as orc_run does.)
  if (CTX.rc > 0) for (int a = 0; a < CHEM_MAX_TYPES; ++a) for (int b = a; b < CHEM_MAX_TYPES; ++b) {
    const HostPairPot& p = CTX.pp[a][b];
    if (p.kind && p.rc > CTX.rc * (1.0 + 1e-12))
      throw ChemError(CHEM_EINVAL, "run: cutoff " + std::to_string(p.rc) + " of type pair (" + std::to_string(a) + "," + std::to_string(b) +
                                   ") exceeds the list cutoff max_cutoff = " + std::to_string(CTX.rc));
  }
  if (CTX.rc > 0 && CTX.coul_on() && CTX.coul_rc > CTX.rc * (1.0 + 1e-12)) {
    int a = 0, b = 0;
    for (a = 0; a < CHEM_MAX_TYPES && !CTX.coul_mask[a]; ++a) {}
    for (b = 0; b < CHEM_MAX_TYPES && !((CTX.coul_mask[a] >> b) & 1u); ++b) {}
    throw ChemError(CHEM_EINVAL, "run: Coulomb cutoff " + std::to_string(CTX.coul_rc) + " of type pair (" + std::to_string(std::min(a, b)) + "," + std::to_string(std::max(a, b)) +
                                 ") exceeds the list cutoff max_cutoff = " + std::to_string(CTX.rc));
  }
  Ctx& c = CTX;
  c.ran = true;
  // fixed distances: a type that chem_modify_particle changed since the last call releases entries of a typed set here
  const bool fix_live = c.fix.any();
  if (fix_live) { c.join_async(); c.fix_after_reactions(false); }
  if (!c.res_tracking() && !c.fix_tracking() && c.fix.joins.empty()) { c.run(nsteps); return 0; }
  // Resolution ramps with a property change: the call runs in pieces that end where a lambda reaches 1 (the host knows every
  // stamp, so it knows every such step: chem_res_host.hpp); the change is applied there, and the forces are evaluated again
  // where the call ends on such a step, so that the forces current at s_full are those of the new properties.  A reaction or
  // ATRP step may stamp particles (type changes, chem_reaction_set_resolution) and so create completion steps nobody could
  // know before: while stamps are tracked a piece also ends at every such step, and the next completion is asked afresh.
  // (a completion changes a type: the release by type of the fixed-distance sets follows it)
  auto completions = [&]() -> int { int k = c.res_apply_completions(); if (k && c.fix.any()) k += c.fix_after_reactions(false); return k; };
  completions();
  if (nsteps == 0) c.run(0);
  for (int64_t left = nsteps; left > 0;) {
    int64_t stop = c.res.next_completion(c.step);
    auto sooner = [&](int64_t every) { const int64_t at = (c.step / every + 1) * every; if (stop < 0 || at < stop) stop = at; };
    if (c.react_on && c.interval > 0) sooner(c.interval);
    if (c.atrp_on && c.atrp.interval > 0) sooner(c.atrp.interval);
    const int64_t len = res_next_piece(c.step, left, stop);
    const int64_t from = c.step;
    c.run(len); left -= c.step - from;      // (a region rule that changed something ends the piece there: its stamps may complete early)
    if (completions() && left == 0) c.run(0);
  }
  return 0;
  API_END(ctx)
}

int64_t chem_num_particles(chem_ctx* ctx) { return ctx->c->top.n; }
int64_t chem_get_step(chem_ctx* ctx) { return ctx->c->step; }

int64_t chem_get_state(chem_ctx* ctx, int what, void* out, int64_t cap) {
  API_BEGIN
  REQUIRE(out, CHEM_EINVAL, "null output");
  if (what == CHEM_STATE_LAMBDA) {      // the fp64 host expression at the current step (replicated by tag: no gather)
    Ctx& c = CTX;
    REQUIRE(cap >= c.top.n, CHEM_ENOSPC, "get_state: capacity");
    for (int64_t t = 0; t < c.top.n; ++t) ((double*)out)[t] = c.res.lambda_at((size_t)t, c.step);
    return c.top.n;
  }
  return CTX.get_state(what, out, cap);
  API_END(ctx)
}

int64_t chem_get_events(chem_ctx* ctx, chem_event* out, int64_t cap) {
  API_BEGIN
  Ctx& c = CTX;
  const int64_t n = (int64_t)c.arena.size();
  if (!out) return n;
  REQUIRE(cap >= n, CHEM_ENOSPC, "get_events: capacity");
  // expand the blocks that are new since the last call, each into canonical order: (step, min id, max id)
  auto& A = c.arena;
  for (size_t bi = A.expanded_blocks; bi < A.blocks.size(); ++bi) {
    const size_t k0 = A.blocks[bi].second, k1 = bi + 1 < A.blocks.size() ? A.blocks[bi + 1].second : A.size(), first = c.events.size();
    for (size_t k = k0; k < k1; ++k)
      c.events.push_back(chem_event{A.blocks[bi].first, c.top.id[A.a[k]], c.top.id[A.b[k]], c.public_index(A.r[k]), A.intra.size() > k ? (int32_t)A.intra[k] : 0, A.d2[k]});
    std::sort(c.events.begin() + first, c.events.end(), [](const chem_event& p, const chem_event& q) {
      return std::make_pair(std::min(p.id_a, p.id_b), std::max(p.id_a, p.id_b)) < std::make_pair(std::min(q.id_a, q.id_b), std::max(q.id_a, q.id_b));
    });
  }
  A.expanded_blocks = A.blocks.size();
  std::copy(c.events.begin(), c.events.end(), out);
  return n;
  API_END(ctx)
}

int64_t chem_get_exclusions(chem_ctx* ctx, int64_t* out, int64_t cap) {
  API_BEGIN
  HostTopology& t = CTX.top;
  if (!out) return t.n_excl_pairs;
  REQUIRE(cap >= t.n_excl_pairs, CHEM_ENOSPC, "get_exclusions: capacity");
  int64_t k = 0;
  for (int64_t a = 0; a < t.n; ++a) for (int32_t b : t.excl[a]) if (b > a) { out[2 * k] = t.id[a]; out[2 * k + 1] = t.id[b]; ++k; }
  return k;
  API_END(ctx)
}

int64_t chem_get_verlet_pairs(chem_ctx* ctx, int64_t* out, int64_t cap) { API_BEGIN return CTX.verlet_pairs(out, cap); API_END(ctx) }

int chem_observe(chem_ctx* ctx, chem_obs* out) { API_BEGIN REQUIRE(out, CHEM_EINVAL, "null output"); CTX.observe(out); return 0; API_END(ctx) }

int chem_get_timers(chem_ctx* ctx, chem_timers* out) {
  API_BEGIN
  REQUIRE(out, CHEM_EINVAL, "null output");
  CTX.refresh_timers();
  *out = CTX.tm;
  return 0;
  API_END(ctx)
}

int chem_device_sync(chem_ctx* ctx) { API_BEGIN CTX.sync(); return 0; API_END(ctx) }

int chem_set_nlist_capacity(chem_ctx* ctx, int m) { API_BEGIN REQUIRE(m >= 0, CHEM_EINVAL, "capacity"); CTX.nl_capacity_user = m; CTX.geom_dirty = true; return 0; API_END(ctx) }

int chem_set_option(chem_ctx* ctx, const char* name, double value) {
  API_BEGIN
  const std::string k = name ? name : "";
  if (k == "tpp") { const int v = (int)value; REQUIRE(v == 0 || v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64, CHEM_EINVAL, "tpp must be a power of two <= 64"); CTX.opt_tpp = v; }
  else if (k == "time_pair_kernel") CTX.opt_time_pair = value > 0 ? (int)value : 0;
  else if (k == "fuse_integrate") CTX.opt_fuse = value != 0;
  else if (k == "ablate_list") CTX.opt_ablate_list = (int)value;
  else if (k == "dd_merge") CTX.opt_dd_merge = value != 0;
  else if (k == "dd_fold") CTX.opt_dd_fold = value != 0;
  else if (k == "dd_fastx") { CTX.opt_dd_fastx = value != 0; CTX.resort = true; }
  else if (k == "coop_overflow") { CTX.opt_coop_overflow = value != 0 ? 1 : 0; CTX.resort = true; }
  else if (k == "row_order") { CTX.opt_row_order = value != 0 ? 1 : 0; CTX.resort = true; }
  else if (k == "lpt_tiles") { CTX.opt_lpt = value != 0; CTX.resort = true; }
  else if (k == "tiles") { CTX.opt_tiles = value != 0; CTX.geom_dirty = true; }
  else if (k == "fused_rebuild") { CTX.opt_fused = value != 0; CTX.geom_dirty = true; }
  else if (k == "overlap_halo") CTX.opt_overlap = value < 0 ? -1 : (value != 0 ? 1 : 0);
  else if (k == "pair_block") { const int v = (int)value; REQUIRE(v == 256 || v == 512 || v == 1024, CHEM_EINVAL, "pair_block must be 256, 512 or 1024"); CTX.set_pair_bs(v); }
  else if (k == "ablate") CTX.opt_ablate = (int)value;
  else if (k == "rebuild_criterion") { CTX.opt_criterion = value != 0 ? 1 : 0; CTX.resort = true; CTX.geom_dirty = true; }
  else if (k == "bonds_inline") { CTX.opt_bonds_inline = value != 0; CTX.resort = true; }
  else if (k == "bond_pass") { CTX.set_bond_pass(value != 0); CTX.resort = true; }
  else if (k == "bond_slots_kernel") { CTX.opt_bond_slots_kernel = value != 0 ? 1 : 0; CTX.resort = true; }
  else if (k == "bucket_cap") { CTX.opt_bucket_cap = (int)value; CTX.geom_dirty = true; }
  else if (k == "tile_split") { CTX.opt_tile_split = (int)value; CTX.geom_dirty = true; CTX.resort = true; }
  else if (k == "list_skin") { CTX.opt_list_skin = value; CTX.geom_dirty = true; CTX.resort = true; }
  else if (k == "debug_stamps") CTX.debug_enable((int)value);
  else if (k == "dd_self") {   // testing: one rank, ghost layers in z exchanged with itself by device copies
    REQUIRE(CTX.particles_dirty && !CTX.dd_on, CHEM_ESTATE, "dd_self must be set before the first run");
    if (value != 0) { CTX.tr.reset(new SelfTransport()); CTX.dd_on = true; CTX.P = 1; CTX.rk = 0; CTX.geom_dirty = true; }
  }
  else if (k == "dd_self_rccl") {   // testing: the same through RCCL (one-rank communicator, send/recv to self)
    REQUIRE(CTX.particles_dirty && !CTX.dd_on, CHEM_ESTATE, "dd_self_rccl must be set before the first run");
    char uid[128];
    REQUIRE(chem_comm_unique_id(uid) == 0, CHEM_ECOMM, "cannot create an RCCL unique id");
    CTX.tr.reset(new RcclTransport(1, 0, uid)); CTX.dd_on = true; CTX.P = 1; CTX.rk = 0; CTX.geom_dirty = true;
  }
  else if (k == "skip_idle") { const int v = (int)value; REQUIRE(v >= 0 && v <= 2, CHEM_EINVAL, "skip_idle must be 0, 1 or 2"); CTX.opt_skip_idle = v; CTX.resort = true; }
  else if (k == "idle_lag") { const int v = (int)value; REQUIRE(v >= 0 && v <= 64, CHEM_EINVAL, "idle_lag must be 0..64"); CTX.opt_idle_lag = v; }
  else if (k == "idle_kappa") { REQUIRE(value >= 1.0 && value <= 16.0, CHEM_EINVAL, "idle_kappa must be 1..16"); CTX.opt_idle_kappa = value; }
  else if (k == "count_intra_inter") CTX.opt_intra_inter = value != 0;
  else if (k == "skip_inactive_pairs") { CTX.opt_skip_inactive = value != 0; CTX.pair_dirty = true; }
  else throw ChemError(CHEM_EINVAL, "unknown option " + k);
  return 0;
  API_END(ctx)
}

// diagnostic: per-tile phase stamps of the last pair-force launch (6 int64 per tile); not part of the public header
int64_t chem_debug_dump(chem_ctx* ctx, long long* out, int64_t cap) { return ctx->c->debug_dump(out, cap); }
// diagnostic: 8 int64 per workgroup of the last rebuilding k_rebuild_fused launch (phase stamps, tiles done)
int64_t chem_debug_dump_rebuild(chem_ctx* ctx, long long* out, int64_t cap) { return ctx->c->debug_dump_rebuild(out, cap); }
// diagnostic / tests: partner tags of the force list of particle `tag`, in list order; -1 without tiles
// diagnostics / tests (unlisted, like chem_debug_force_list): how many times a run stopped by the device was resumed
// ... and the tile geometry in use: out[0..5] = tiles, cells along x, wide tiles per row, width of the narrow ones, tile rows, LDS slots per tile
// diagnostics of tools/sq_workload.py (not in the header): `frames` frames back to back, device milliseconds per frame between two events
int chem_debug_sq_frame_ms(chem_ctx* ctx, int frames, double* ms) {
  API_BEGIN
  REQUIRE(CTX.sq.on, CHEM_ESTATE, "sq frame timing before chem_sq_init");
  REQUIRE(frames > 0 && ms, CHEM_EINVAL, "frames");
  *ms = CTX.sq_time_frames(frames);
  return 0;
  API_END(ctx)
}
int64_t chem_debug_tiles(chem_ctx* ctx, int32_t* out) { try { ctx->c->debug_tiles(out); return 0; } catch (...) { return -2; } }
int64_t chem_debug_halts(chem_ctx* ctx) { return ctx && ctx->c ? ctx->c->halts_recovered : -1; }
int64_t chem_debug_idle_skipped(chem_ctx* ctx) { return ctx && ctx->c ? ctx->c->idle_skipped : -1; }
int64_t chem_debug_idle_wrong_skips(chem_ctx* ctx) { return ctx && ctx->c ? ctx->c->idle_wrong : -1; }
int64_t chem_debug_idle_timeouts(chem_ctx* ctx) { return ctx && ctx->c ? ctx->c->idle_timeouts : -1; }
// tests (unlisted): out[0] = DevCtl::acc_ref, out[1] = DevCtl::acc_maxdist after the last call
int64_t chem_debug_acc(chem_ctx* ctx, double* out) { try { ctx->c->debug_acc(out); return 0; } catch (...) { return -2; } }
// ... the stored order of a tile's force-list rows (option row_order): counts by position, then the home of every position; returns the tile's home count
int64_t chem_debug_row_order(chem_ctx* ctx, int32_t tile, int32_t* out, int64_t cap) { try { return ctx->c->debug_row_order(tile, out, cap); } catch (...) { return -2; } }
int64_t chem_debug_force_list(chem_ctx* ctx, int32_t tag, int32_t* out, int64_t cap) { try { return ctx->c->debug_force_list(tag, out, cap); } catch (...) { return -2; } }

int chem_comm_unique_id(char uid[128]) {
  RcclApi& a = rccl_api();
  if (!a.load()) { g_create_error = a.err; return CHEM_ECOMM; }
  RcclApi::UniqueId id;
  if (a.GetUniqueId(&id) != 0) { g_create_error = "ncclGetUniqueId failed"; return CHEM_ECOMM; }
  std::memcpy(uid, id.internal, 128);
  return 0;
}

int chem_comm_init(chem_ctx* ctx, int nranks, int rank, const int node_grid[3], const char uid[128]) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, CHEM_EINVAL, "comm_init: rank/nranks");
  REQUIRE(c.dissociations.empty(), CHEM_ENOTIMPL, "dissociation reactions are registered: they are not available on the decomposed path");
  REQUIRE(c.res_rules.empty(), CHEM_ENOTIMPL, "reaction_set_resolution rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.fix.any() && c.fix.rules.empty(), CHEM_ENOTIMPL, "fixed-distance entries or release rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.reverse_on(), CHEM_ENOTIMPL, "bond-removal or join rules are registered: they are not available on the decomposed path");
  REQUIRE(c.regions.empty(), CHEM_ENOTIMPL, "region rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.dd_on, CHEM_ESTATE, "comm_init: already initialised");
  if (nranks == 1 && !uid) return 0;   // single domain, nothing to do
  REQUIRE(node_grid && node_grid[0] == 1 && node_grid[1] == 1 && node_grid[2] == nranks, CHEM_ENOTIMPL,
          "comm_init: this build decomposes along z only, node grid must be (1,1,nranks)");
  REQUIRE(uid, CHEM_EINVAL, "comm_init: unique id");
  REQUIRE(c.particles_dirty, CHEM_ESTATE, "comm_init must precede the first run (particles are already on the device)");
  HIPCHK(hipSetDevice(c.device));   // the communicator binds to the calling thread's current device
  c.tr.reset(new RcclTransport(nranks, rank, uid));
  c.dd_on = true; c.P = nranks; c.rk = rank; c.geom_dirty = true;
  return 0;
  API_END(ctx)
}

// In-process ranks (several contexts of one process, one host thread each) exchanging through a
// shared hub: validates the multi-rank decomposition on a single GPU.  Same contract as
// chem_comm_init, `hub_id` names the group.
namespace chem {
IpcTransport::IpcTransport(int nr, int rk, const char* shm_name) {
  nranks = nr; rank = rk; name = shm_name ? shm_name : "";
  if (nr > IpcShm::kMaxRanks || name.empty()) throw ChemError(CHEM_EINVAL, "ipc transport: 1..16 ranks and a segment name");
  // rank 0 creates the segment, the others wait for it (the launcher hands every rank the same fresh name)
  int fd = -1;
  if (rk == 0) {
    shm_unlink(name.c_str());
    fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0 || ftruncate(fd, sizeof(IpcShm)) != 0) throw ChemError(CHEM_ECOMM, "ipc transport: cannot create shared memory " + name);
    owner = true;
  } else {
    const double t0 = now();
    struct stat st;
    while ((fd = shm_open(name.c_str(), O_RDWR, 0600)) < 0 || fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(IpcShm)) {
      if (fd >= 0) { close(fd); fd = -1; }
      if (now() - t0 > 120.0) throw ChemError(CHEM_ECOMM, "ipc transport: shared memory " + name + " did not appear");
      usleep(1000);
    }
  }
  void* p = mmap(nullptr, sizeof(IpcShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (p == MAP_FAILED) throw ChemError(CHEM_ECOMM, "ipc transport: mmap");
  shm = (IpcShm*)p;
  if (rk == 0) { shm->P = (unsigned)nr; shm->arrived = 0; shm->gen = 0; shm->attached = 0; __atomic_store_n(&shm->magic, 0xC4E31234u, __ATOMIC_RELEASE); }
  else {
    const double t0 = now();
    while (__atomic_load_n(&shm->magic, __ATOMIC_ACQUIRE) != 0xC4E31234u) { if (now() - t0 > 120.0) throw ChemError(CHEM_ECOMM, "ipc transport: segment never initialised"); usleep(1000); }
    if (shm->P != (unsigned)nr) throw ChemError(CHEM_ECOMM, "ipc transport: rank count mismatch");
  }
  __atomic_add_fetch(&shm->attached, 1u, __ATOMIC_ACQ_REL);
  barrier();
}
IpcTransport::~IpcTransport() {
  for (auto& kv : opened) (void)hipIpcCloseMemHandle(kv.second);
  if (shm) {
    const unsigned left = __atomic_sub_fetch(&shm->attached, 1u, __ATOMIC_ACQ_REL);
    munmap(shm, sizeof(IpcShm));
    if (owner || left == 0) shm_unlink(name.c_str());
  }
}
}  // namespace chem

/* One process per rank, several ranks per device allowed: the slab decomposition of chem_comm_init over hipIpc
 * memory handles with a POSIX shared-memory rendezvous named `shm_name` (same fresh name on every rank). */
int chem_comm_init_ipc(chem_ctx* ctx, int nranks, int rank, const char* shm_name) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks && shm_name, CHEM_EINVAL, "comm_init_ipc: rank/nranks/name");
  REQUIRE(c.dissociations.empty(), CHEM_ENOTIMPL, "dissociation reactions are registered: they are not available on the decomposed path");
  REQUIRE(c.res_rules.empty(), CHEM_ENOTIMPL, "reaction_set_resolution rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.fix.any() && c.fix.rules.empty(), CHEM_ENOTIMPL, "fixed-distance entries or release rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.reverse_on(), CHEM_ENOTIMPL, "bond-removal or join rules are registered: they are not available on the decomposed path");
  REQUIRE(c.regions.empty(), CHEM_ENOTIMPL, "region rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.dd_on && c.particles_dirty, CHEM_ESTATE, "comm_init_ipc must precede the first run");
  HIPCHK(hipSetDevice(c.device));
  c.tr.reset(new IpcTransport(nranks, rank, shm_name));
  c.dd_on = true; c.P = nranks; c.rk = rank; c.geom_dirty = true;
  return 0;
  API_END(ctx)
}

int chem_comm_init_local(chem_ctx* ctx, int nranks, int rank, int hub_id) {
  API_BEGIN
  Ctx& c = CTX;
  REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, CHEM_EINVAL, "comm_init_local: rank/nranks");
  REQUIRE(c.dissociations.empty(), CHEM_ENOTIMPL, "dissociation reactions are registered: they are not available on the decomposed path");
  REQUIRE(c.res_rules.empty(), CHEM_ENOTIMPL, "reaction_set_resolution rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.fix.any() && c.fix.rules.empty(), CHEM_ENOTIMPL, "fixed-distance entries or release rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.reverse_on(), CHEM_ENOTIMPL, "bond-removal or join rules are registered: they are not available on the decomposed path");
  REQUIRE(c.regions.empty(), CHEM_ENOTIMPL, "region rules are registered: they are not available on the decomposed path");
  REQUIRE(!c.dd_on && c.particles_dirty, CHEM_ESTATE, "comm_init_local must precede the first run");
  c.tr.reset(new LocalTransport(nranks, rank, hub_id));
  c.dd_on = true; c.P = nranks; c.rk = rank; c.geom_dirty = true;
  return 0;
  API_END(ctx)
}

}  // extern "C"
