// The weighted mean of temporal ensembling (include/genima_hip.h states the rule), written once: action_ensemble_kernel walks its ring with it,
// openloop_exec_actions_kernel walks the table of an evaluation's chunks with it.  Both live in ensemble.hip, so both get the same contraction
// flags and the same instruction sequence per term: equal inputs in equal order give equal bits.
//
// Further down, the pieces that combine R sampled chunks into the one that is executed (gn_action_ensemble_samples_f16 and
// gn_openloop_exec_actions_samples): the sample mean, the medoid pick of one workgroup and the spread, each written once for both.
#pragma once
#include "common.h"

constexpr int ENS_THREADS = 256;
constexpr int ENS_WAVES = ENS_THREADS / 64;
constexpr int ENS_MAX_SAMPLES = GN_ENSEMBLE_MAX_SAMPLES;
constexpr int ENS_MAX_STAGED = GN_ENSEMBLE_MAX_STAGED;               // f32 values of one row's R samples a workgroup stages in LDS
constexpr int ENS_PARTS = (ENS_MAX_SAMPLES + 1) * ENS_WAVES;         // per-wave partial sums: one line per D_r, the last one for the spread

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

// ---- R sampled chunks -> the executed one --------------------------------------------------------------------------------------------------
// The sample mean of one element: x(r) widened to f32, added in sample order starting FROM x(0) (so that one sample comes back as it is, the
// sign of a zero included), one multiplication by inv_R = (float)(1.0 / R) at the end.
template <typename F>
__device__ __forceinline__ float ens_sample_mean(int R, float inv_R, F&& x) {
  float s = x(0);
  for (int r = 1; r < R; ++r) s += x(r);
  return s * inv_R;
}

// Sum over the 64 lanes of a wave by the xor butterfly 32, 16, .. 1: f32 addition commutes, so every lane ends with the same bits.
__device__ __forceinline__ float ens_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The medoid of the R samples staged as f32 s_x[R][n] in LDS (complete: the caller's barrier stands behind the staging).  The fixed order:
// thread t adds |x_r[e] - x_q[e]| for q = 0 .. R - 1 (outer) and e = t, t + ENS_THREADS, .. < n (inner) into one f32; the wave butterfly
// above; D_r = ((w0 + w1) + w2) + w3 over the four waves; thread 0 takes the first r with the smallest D_r (strict <: ties go to the lowest r).
// Every thread returns the pick.  s_part: ENS_PARTS floats, s_pick: one int.
__device__ __forceinline__ int ens_medoid_pick(const float* s_x, int R, int n, float* s_part, int* s_pick) {
  const int tid = threadIdx.x;
  for (int r = 0; r < R; ++r) {
    float acc = 0.f;
    for (int q = 0; q < R; ++q)
      for (int e = tid; e < n; e += ENS_THREADS) acc += fabsf(s_x[r * n + e] - s_x[q * n + e]);
    acc = ens_wave_sum(acc);
    if ((tid & 63) == 0) s_part[r * ENS_WAVES + (tid >> 6)] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    float best_d = 0.f;
    for (int r = 0; r < R; ++r) {
      const float* w = s_part + r * ENS_WAVES;
      const float d = ((w[0] + w[1]) + w[2]) + w[3];
      if (r == 0 || d < best_d) best = r, best_d = d;
    }
    *s_pick = best;
  }
  __syncthreads();
  return *s_pick;
}

// One workgroup combines the staged samples s_x[R][n]: the combined chunk (the mean, or sample `pick`) ends in s_x[0 .. n), visible to every
// thread on return; thread t reads and writes its own elements e = t, t + ENS_THREADS, .. of every sample alone.  -> the pick (-1 under mean);
// spread = (sum_r sum_e |x_r[e] - chosen[e]|) * inv_R / n with the sum in the order of ens_medoid_pick: per thread e outer and r inner, the wave
// butterfly, the four waves left to right; then one multiplication, then one division by (float)n.
__device__ __forceinline__ int ens_combine_samples(float* s_x, int R, int n, float inv_R, int combine, float* s_part, int* s_pick, float& spread) {
  const int tid = threadIdx.x;
  const int pick = combine ? ens_medoid_pick(s_x, R, n, s_part, s_pick) : -1;
  float acc = 0.f;
  for (int e = tid; e < n; e += ENS_THREADS) {
    const float c = combine ? s_x[pick * n + e] : ens_sample_mean(R, inv_R, [&](int r) { return s_x[r * n + e]; });
    for (int r = 0; r < R; ++r) acc += fabsf(s_x[r * n + e] - c);
    s_x[e] = c;
  }
  acc = ens_wave_sum(acc);
  float* w = s_part + ENS_MAX_SAMPLES * ENS_WAVES;
  if ((tid & 63) == 0) w[tid >> 6] = acc;
  __syncthreads();
  spread = (((w[0] + w[1]) + w[2]) + w[3]) * inv_R / (float)n;
  return pick;
}
