// Which pressure-tensor kernel runs (DESIGN.md "Pressure tensor").  The tensor pass walks the lists the step's forces used and
// evaluates what the energy pass of that context evaluates, so its rule starts from pair_plan's answer for the ENERGY launch
// (chem_launch_host.hpp, which this header reads and does not change) and narrows it to the few TENSOR instantiations the
// library builds: an observable needs neither the lanes-per-particle nor the block-size options.  Free of HIP:
// CtxT::launch_pair_tensor (chem_api.hip) turns the answer into an instantiation; tests/host/tensor_harness.cpp checks it on
// the CPU.
#pragma once
#include "chem_launch_host.hpp"

namespace chem {

// tiles: MODE 3 (general with both table kinds: serves what MODE 0..3 serve) or 4..7, one lane per particle, 512 threads;
// rows:  MODE 0 (the plain kernel in its CUBIC build) or 4..7, four lanes per particle, 256 threads
struct TensorVariant { PairFamily family; int mode, tpp, block; };
constexpr bool tensor_variant_built(PairFamily family, int mode, int tpp, int block) {
  if (family == PairFamily::tiles) return (mode >= 3 && mode <= 7) && tpp == 1 && block == 512;
  return (mode == 0 || (mode >= 4 && mode <= 7)) && tpp == 4 && block == 256;
}
struct TensorPlan {
  int code;              // CHEM_OK: launch `v`; otherwise pair_plan's refusal, `refused`, with its code and its text
  TensorVariant v;
  PairPlan refused;
};
// `in` as CtxT fills it for a launch; its `energy` field is not looked at
inline TensorPlan tensor_plan(PairInput in) {
  in.energy = true;
  const PairPlan p = pair_plan(in);
  TensorPlan t{p.code, TensorVariant{p.v.family, 0, 0, 0}, p};
  if (p.code != CHEM_OK) return t;
  const bool feature = p.v.mode >= 4;
  if (p.v.family == PairFamily::tiles) t.v = TensorVariant{PairFamily::tiles, feature ? p.v.mode : 3, 1, 512};
  else t.v = TensorVariant{PairFamily::rows, feature ? p.v.mode : 0, 4, 256};
  return t;
}

}  // namespace chem
