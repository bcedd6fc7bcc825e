// The ACT replay's per-sample rules, shared by the kernels that assemble a training batch from the device-resident tables (replay.hip:
// replay_gather_kernel; replay_render.hip: replay_render_kernel) so that their low-dimensional outputs agree bit for bit.  D is the
// descriptor (gn_replay_gather_desc, gn_replay_render_desc): both name the tables and their sizes alike.  Every table index is clamped into
// its table, so a wrong index reads a wrong row, never outside the tables.
#pragma once
#include "common.h"

__device__ __forceinline__ int rg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the observation of frame-stack slot k of transition n: the stack ends at the transition's own observation and repeats the episode's first
template <class D>
__device__ __forceinline__ int rg_obs(const D& d, int n, int k) {
  const int o = d.obs_index[n] - (d.fs - 1) + k, first = d.first_obs[n];
  return rg_clamp(o < first ? first : o, 0, (int)d.N_obs - 1);
}

// sample b's low_dim_state, action chunk and token row of transition n, by the THREADS threads of one block (tid: the thread's index in it)
template <int THREADS, class D>
__device__ __forceinline__ void rg_write_low_dim(const D& d, int b, int n, int tid) {
  const int nS = d.fs * d.S, nA = d.T * d.A;
  for (int e = tid; e < nS; e += THREADS) {
    const int k = e / d.S, s = e - k * d.S;
    d.low_dim_state[(long)b * nS + e] = d.qpos[(long)rg_obs(d, n, k) * d.S + s];
  }
  const int last = d.last_tr[n];
  for (int e = tid; e < nA; e += THREADS) {
    const int j = e / d.A, a = e - j * d.A;
    const int row = rg_clamp(n + j < last ? n + j : last, 0, d.N - 1);  // the chunk repeats the episode's last action
    d.action_out[(long)b * nA + e] = d.action[(long)row * d.A + a];
  }
  if (d.tokens_out) {  // the episode's task string, tokenised once at load
    const int ep = rg_clamp(d.episode[n], 0, d.N_ep - 1);
    for (int e = tid; e < d.L_tok; e += THREADS) d.tokens_out[(long)b * d.L_tok + e] = d.lang_tokens[(long)ep * d.L_tok + e];
  }
}
