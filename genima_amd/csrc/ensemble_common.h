// The weighted mean of temporal ensembling (include/genima_hip.h states the rule), written once: action_ensemble_kernel walks its ring with it,
// openloop_exec_actions_kernel walks the table of an evaluation's chunks with it.  Both live in ensemble.hip, so both get the same contraction
// flags and the same instruction sequence per term: equal inputs in equal order give equal bits.
#pragma once
#include "common.h"

__device__ __forceinline__ float ens_load(const float* p) { return *p; }
__device__ __forceinline__ float ens_load(const f16* p) { return (float)*p; }

// term(j, v) for j = 0 .. n - 1, oldest candidate first: false = candidate j does not take part, true = it does, with the value v.
// -> sum_i w_i v_i / sum_i w_i over the taking-part ones, i their rank, w_0 = 1, w_i = expf(-m i); f32, accumulated from the oldest on.
// At least one candidate must take part (the callers' newest chunk always does), so the denominator is >= 1.
template <typename F>
__device__ __forceinline__ float ens_weighted_mean(int n, float m, int* n_used, F&& term) {
  float num = 0.f, den = 0.f;
  int i = 0;
  for (int j = 0; j < n; ++j) {
    float v;
    if (!term(j, v)) continue;
    const float wt = i == 0 ? 1.0f : expf(-m * (float)i);
    num += wt * v;
    den += wt;
    ++i;
  }
  if (n_used) *n_used = i;
  return num / den;
}
