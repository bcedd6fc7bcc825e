// The ACT controller's random-background training batch, drawn instead of gathered (genima_amd/replay.py DeviceReplay(render=...); the
// reference's rnd_bg tree, render/render_data.py:296-311): per sample, view and frame-stack slot the joint-target spheres of the slot's
// observation are ray-cast and alpha-blended over a texture of a device-resident bank, texture and blend factor picked by a hash of
// (seed, draw, sample, view, slot), in ONE launch per batch.  genima_hip.h (gn_replay_render) states the arithmetic; the ray-caster and the
// composite are render_common.h's (gn_render_spheres' pixels, bit for bit), the per-sample rules replay_common.h's (gn_replay_gather's).
//
// Shape: render.hip's.  blockIdx.z = sample, blockIdx.y = view * fs + slot, blockIdx.x = a 64 x 4 pixel block of the frame (a wave = 64
// consecutive pixels of one row: 1 KiB of contiguous 16-byte stores on the f16 NHWC-8 output).  The slot's indirection (transition ->
// observation -> view) is block-uniform integer work on scalar loads; thread 0 makes the slot's texture layer and f64 blend once and the
// first `count` threads bring the view's spheres into eye space, both left in LDS.  A pixel outside every bounding rectangle is the
// texture's without casting a ray.  The blocks of grid row (x = 0, y = 0) also write their sample's low_dim_state, action chunk and token
// row.  No scratch, no atomics.  Built with -ffp-contract=off: the blend is numpy's unfused f64 multiply / multiply / add, truncated.
#include "attention_dropout.h"
#include "render_common.h"
#include "replay_common.h"

namespace {

constexpr int RR_THREADS = 256;

struct DrawLds {
  int layer;
  double blend;
};

__global__ __launch_bounds__(RR_THREADS) void replay_render_kernel(const gn_replay_render_desc d) {
  __shared__ SphereLds sph[MAX_SPHERES];
  __shared__ DrawLds pick;
  const int b = blockIdx.z, slot = blockIdx.y;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const int n = rg_clamp(d.idx[b], 0, d.N - 1);
  const int v = slot / d.fs, k = slot - v * d.fs;
  const long view = (long)rg_obs(d, n, k) * d.V + v;
  const float* __restrict__ cam = d.cams + view * CAM_FLOATS;
  int cnt = d.count[view];
  cnt = cnt < 0 ? 0 : (cnt > d.n_spheres ? d.n_spheres : cnt);
  const long frame = (long)b * gridDim.y + slot;
  if (tid == 0) {  // the slot's texture and blend (gn_replay_render in genima_hip.h): uint32 arithmetic that wraps, then f64
    const unsigned base = attn_drop_mix(d.seed_lo ^ 0x6A09E667u ^ (d.draw * 0x9E3779B9u)) ^ d.seed_hi;
    const unsigned s = attn_drop_mix(base + (unsigned)frame * 0x85EBCA6Bu);
    const int layer = (int)(((uint64_t)attn_drop_mix(s ^ 0xC2B2AE35u) * (uint64_t)(unsigned)d.NB) >> 32);
    const unsigned u = attn_drop_mix(s ^ 0x27D4EB2Fu) >> 8;
    const double alpha = d.alpha_blend;
    const double blend = __dadd_rn(alpha, __dmul_rn(__dsub_rn(1.0, alpha), __dmul_rn((double)u, 0x1p-24)));
    pick.layer = layer, pick.blend = blend;
    if (blockIdx.x == 0) {
      if (d.bg_layer) d.bg_layer[frame] = layer;
      if (d.blend_out) d.blend_out[frame] = blend;
    }
  }
  if (tid < cnt)
    sphere_to_lds(sph[tid], cam, d.spheres + (view * d.n_spheres + tid) * SPHERE_FLOATS, d.tex_index[view * d.n_spheres + tid], d.n_tex, d.W, d.H);
  if (blockIdx.x == 0 && slot == 0) rg_write_low_dim<RR_THREADS>(d, b, n, tid);  // the sample's low-dimensional values
  __syncthreads();

  const int bw = (d.W + 63) / 64;  // blocks across a row
  const int by = blockIdx.x / bw, bx = blockIdx.x - by * bw;
  const int px = bx * 64 + threadIdx.x, py = by * 4 + threadIdx.y;
  if (px >= d.W || py >= d.H) return;
  const long pix = (frame * d.H + py) * d.W + px;

  uint8_t r8, g8, b8;
  shade_pixel(sph, cnt, SphereAtlas{d.atlas, d.n_tex, d.th, d.tw}, cam, d.samples, px, py, r8, g8, b8);
  const bool white = r8 == 255 && g8 == 255 && b8 == 255;  // render_data.py keys on the COLOUR, not on coverage
  const uint8_t* __restrict__ t = d.bank + (((long)pick.layer * d.H + py) * d.W + px) * 3;
  uint8_t tr = t[0], tg = t[1], tb = t[2];
  if (!white) {
    const double bl = pick.blend, om = 1.0 - bl;
    tr = blend_u8(r8, tr, bl, om), tg = blend_u8(g8, tg, bl, om), tb = blend_u8(b8, tb, bl, om);
  }
  if (d.images_u8) d.images_u8[pix * 3] = tr, d.images_u8[pix * 3 + 1] = tg, d.images_u8[pix * 3 + 2] = tb;
  store_f16_pixel((f16*)d.images + pix * 8, tr, tg, tb, 1.0f, 0.0f);
}

}  // namespace

extern "C" int32_t gn_replay_render(gn_ctx* ctx, const gn_replay_render_desc* dp) {
  GN_REQUIRE(ctx && dp, "gn_replay_render: null argument");
  const gn_replay_render_desc& d = *dp;
  GN_REQUIRE(d.cams && d.spheres && d.tex_index && d.count && d.atlas && d.bank && d.qpos && d.action && d.obs_index && d.first_obs && d.last_tr && d.idx &&
                 d.images && d.low_dim_state && d.action_out,
             "gn_replay_render: null table or output (only images_u8, bg_layer, blend_out and the token tables are optional)");
  GN_REQUIRE(!d.tokens_out || (d.lang_tokens && d.episode && d.N_ep > 0 && d.L_tok > 0 && d.L_tok <= (1 << 16) &&
                               (((uintptr_t)d.lang_tokens | (uintptr_t)d.episode | (uintptr_t)d.tokens_out) & 3) == 0),
             "gn_replay_render: tokens_out needs lang_tokens, episode, N_ep (%d) > 0 and L_tok (%d) > 0", d.N_ep, d.L_tok);
  GN_REQUIRE(d.B > 0 && d.B <= 65535 && d.V > 0 && d.fs > 0 && (int64_t)d.V * d.fs <= 65535, "gn_replay_render: B (%d), V (%d), fs (%d) out of range", d.B,
             d.V, d.fs);
  GN_REQUIRE(d.T > 0 && d.S > 0 && d.A > 0 && (int64_t)d.T * d.A <= (1 << 24) && (int64_t)d.fs * d.S <= (1 << 24),
             "gn_replay_render: T (%d), S (%d), A (%d) out of range", d.T, d.S, d.A);
  GN_REQUIRE(d.N > 0 && d.N_obs > 0 && d.N_obs * d.V <= INT32_MAX, "gn_replay_render: N (%d), N_obs (%ld) out of range", d.N, (long)d.N_obs);
  GN_REQUIRE(d.n_spheres > 0 && d.n_spheres <= MAX_SPHERES && d.H > 0 && d.W > 0 && d.H <= (1 << 16) && d.W <= (1 << 16),
             "gn_replay_render: bad n_spheres / H / W (n_spheres <= %d)", MAX_SPHERES);
  GN_REQUIRE(d.samples == 1 || d.samples == 4, "gn_replay_render: samples must be 1 or 4");
  GN_REQUIRE(d.n_tex > 0 && d.th > 0 && d.tw > 0 && d.NB >= 1, "gn_replay_render: empty atlas or background bank (NB = %d)", d.NB);
  GN_REQUIRE(d.alpha_blend >= 0.0 && d.alpha_blend <= 1.0, "gn_replay_render: alpha_blend %g must lie in [0, 1]", d.alpha_blend);
  GN_REQUIRE(((uintptr_t)d.images & 15) == 0, "gn_replay_render: images must be 16-byte aligned");
  GN_REQUIRE(((uintptr_t)d.blend_out & 7) == 0 &&
                 (((uintptr_t)d.cams | (uintptr_t)d.spheres | (uintptr_t)d.tex_index | (uintptr_t)d.count | (uintptr_t)d.atlas | (uintptr_t)d.qpos |
                   (uintptr_t)d.action | (uintptr_t)d.obs_index | (uintptr_t)d.first_obs | (uintptr_t)d.last_tr | (uintptr_t)d.idx | (uintptr_t)d.bg_layer |
                   (uintptr_t)d.low_dim_state | (uintptr_t)d.action_out) & 3) == 0,
             "gn_replay_render: misaligned table or output");
  const int64_t blocks = (int64_t)((d.W + 63) / 64) * ((d.H + 3) / 4);
  hipLaunchKernelGGL(replay_render_kernel, dim3((unsigned)blocks, (unsigned)(d.V * d.fs), (unsigned)d.B), dim3(64, 4), 0, ctx->stream, d);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
