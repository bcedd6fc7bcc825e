// Attention-probability dropout: the keep mask as a pure function of (seed, batch * heads + head, query row, key index), so the forward
// kernel (attention.hip), both backward kernels (attention_bwd.hip) and the elementwise gn_attention_dropout_apply evaluate it where
// they hold a probability and nothing is materialised.  The formula is stated in include/genima_hip.h (gn_attn_dropout); all of it is
// uint32 arithmetic that wraps.  tests/attention_dropout_ref.py restates it in numpy.
#pragma once
#include "common.h"

struct AttnDropout {
  unsigned threshold, seed_lo, seed_hi;
  float inv_keep;
};

// the argument checks of the three dropout entry points and the kernel argument made from a gn_attn_dropout
inline int32_t attn_dropout_args(const gn_attn_dropout* dr, AttnDropout& out, const char* who) {
  GN_REQUIRE(dr, "%s: null dropout descriptor", who);
  GN_REQUIRE(dr->inv_keep >= 1.0f && dr->inv_keep < INFINITY, "%s: inv_keep %g must be finite and >= 1", who, (double)dr->inv_keep);
  out.threshold = dr->threshold; out.seed_lo = dr->seed_lo; out.seed_hi = dr->seed_hi; out.inv_keep = dr->inv_keep;
  return GN_OK;
}

__device__ __forceinline__ unsigned attn_drop_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// wave-uniform part: one per (batch, head)
__device__ __forceinline__ unsigned attn_drop_head(const AttnDropout& d, int bh) {
  return attn_drop_mix(d.seed_lo ^ 0x6A09E667u ^ ((unsigned)bh * 0x9E3779B9u)) ^ d.seed_hi;
}
// one per query row a lane owns
__device__ __forceinline__ unsigned attn_drop_row(unsigned head, int i) { return attn_drop_mix(head + (unsigned)i * 0x85EBCA6Bu); }
// one per probability
__device__ __forceinline__ bool attn_drop_keep(unsigned row, int j, unsigned threshold) {
  return attn_drop_mix(row ^ ((unsigned)j * 0xC2B2AE35u)) >= threshold;
}
