// The host's side of "neighbour launch only on steps that can need a rebuild" (single domain, fused rebuild, accumulated
// criterion).  The device decides about the Verlet list on every step; on most steps the decision is
// "still valid" and the launch of k_rebuild_fused that would take it does nothing else.  The host may leave that launch out --
// the force kernel's prologue takes the decision then -- when it can tell from a published state of the device that the step
// cannot need a rebuild.  This header is the rule, free of HIP: CtxT::run (chem_api.hip) calls it once per step,
// tests/host/idle_harness.cpp checks it on the CPU.
#pragma once
#include <cmath>

namespace chem {

// What the bookkeeping thread of a step's decision writes into pinned host memory (md_kernels.hpp publish_hint): the
// accumulated distance after step `step` and that step's largest displacement.  `step` is written last, behind a release
// fence.  The host copies the words and reads `step` again: a copy whose two reads of `step` differ is thrown away.  A copy
// that is torn all the same (the device two steps ahead of a reader that was descheduled in the middle) can only mislead the
// prediction, never the result: the device decides on every step, see idle_launch.
struct IdleHint {
  long long step;      // -1: nothing published
  double acc;          // DevCtl::acc_pp after that step (0 behind a rebuild)
  double d;            // sqrt(DevCtl::step_m2) of that step
  int gen;             // generation the launch was enqueued under
  int halted;          // != 0: generation whose run a launch-less step has stopped (the host need not wait for its next synchronisation)
};

// what the host knows by itself when it is about to enqueue step s
struct IdleHost {
  int gen;             // current generation: bumped by everything that changes the device's accumulated distance behind the hint's back
  bool requested;      // the host itself asked for a rebuild on this step (resort, a reaction step's request_rebuild, set-up changes)
  bool diagnostics;    // want32 / debug_stamps: those launches are the point
};

// true: enqueue the neighbour launch for step s; false: leave it out.
// The criterion is cumulative -- acc += max_i |dx_i| per step, rebuild at acc > half_skin -- and the per-step maximum over
// many particles is steady, so acc_s <= acc_p + (s - p) d' with d' a little above d_p.  The rule allows kappa * d_p per step
// and one step more than lie between p and s.  It is a prediction: a rebuild that falls due on a launch-less step stops the
// run there (DevCtl::halt) and the host redoes the step with the launch.
inline bool idle_launch(const IdleHint& h, const IdleHost& host, long long s, double half_skin, double kappa) {
  if (host.requested || host.diagnostics) return true;
  if (h.step < 0 || h.gen != host.gen || h.step >= s) return true;      // nothing published, another generation, not older than s
  if (!(h.acc >= 0.0) || !(h.d >= 0.0) || !std::isfinite(h.acc) || !std::isfinite(h.d)) return true;
  if (!(kappa >= 1.0) || !(half_skin > 0.0)) return true;
  const double bound = h.acc + (double)(s - h.step + 1) * kappa * h.d;
  return !(bound <= half_skin);
}

// the look-ahead: before it enqueues step s the host wants a hint about step s - lag or later (of its generation)
inline bool idle_hint_fresh(const IdleHint& h, int gen, long long s, int lag) { return h.gen == gen && h.step >= 0 && h.step >= s - (long long)lag; }

// one turn of the host's wait on the pinned words
inline void idle_cpu_pause() {
#if defined(__HIP_DEVICE_COMPILE__)
#elif defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#endif
}

}  // namespace chem
