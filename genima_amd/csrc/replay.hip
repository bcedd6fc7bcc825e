// Batch assembly of the ACT controller's training replay (genima_amd/replay.py DeviceReplay): every frame, proprioception row and action
// (and task-token row) of the demo set stays on the device, and ONE launch gathers a batch from B transition indices that are themselves on the device.
//
// Grid: x = blocks of 4-pixel threads over a frame, y = view * fs + frame-stack slot, z = sample.  A thread converts four pixels: 12 bytes
// in as three dwords (a frame that is not 4-byte aligned, and the pixels % 4 tail, take byte loads), one 16-byte store per pixel; the
// per-byte expression is image_convert.h's, with mul / add passed at run time as gn_image_u8_to_f16 gets them, so the two outputs agree bit
// for bit.  The blocks of grid row (x = 0, y = 0) also write their sample's low_dim_state, action chunk and token row.  Plain vector loads and stores,
// no atomics; every table index is clamped into its table, so a wrong index reads a wrong row, never outside the tables.
#include "image_convert.h"
#include "replay_common.h"

namespace {

constexpr int RG_THREADS = 256;

typedef const __attribute__((address_space(1))) uint8_t* rg_gptr8;  // the frames are global memory: global_load, not flat_load
typedef const __attribute__((address_space(1))) uint32_t* rg_gptr32;

__device__ __forceinline__ void rg_store_pixel(f16* __restrict__ o, uint8_t r, uint8_t g, uint8_t b, float mul, float add) {
  const f16 z = (f16)0.0f;
  *reinterpret_cast<f16x8*>(o) = f16x8{u8_to_f16_value(r, mul, add), u8_to_f16_value(g, mul, add), u8_to_f16_value(b, mul, add), z, z, z, z, z};
}

__global__ __launch_bounds__(RG_THREADS) void replay_gather_kernel(gn_replay_gather_desc d, float mul, float add) {
  const int b = blockIdx.z, slot = blockIdx.y;
  const int n = rg_clamp(d.idx[b], 0, d.N - 1);
  if (blockIdx.x == 0 && slot == 0) rg_write_low_dim<RG_THREADS>(d, b, n, threadIdx.x);  // the sample's low-dimensional values
  const long p0 = ((long)blockIdx.x * RG_THREADS + threadIdx.x) * 4;
  if (p0 >= d.pixels) return;
  const int v = slot / d.fs, k = slot - v * d.fs;
  const rg_gptr8 in = (rg_gptr8)d.frame_ptr[(long)rg_obs(d, n, k) * d.V + v];
  const long frame = (long)b * gridDim.y + slot;
  f16* __restrict__ o = (f16*)d.images + (frame * d.pixels + p0) * 8;
  uint8_t* __restrict__ o8 = d.images_u8 ? d.images_u8 + (frame * d.pixels + p0) * 3 : nullptr;
  if (p0 + 4 <= d.pixels && ((uintptr_t)in & 3) == 0) {
    const rg_gptr32 w = (rg_gptr32)(in + p0 * 3);
    const uint32_t q[3] = {w[0], w[1], w[2]};
    uint8_t by[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) by[i] = (uint8_t)(q[i >> 2] >> ((i & 3) * 8));
#pragma unroll
    for (int j = 0; j < 4; ++j) rg_store_pixel(o + j * 8, by[j * 3], by[j * 3 + 1], by[j * 3 + 2], mul, add);
    if (o8) {
      if (((uintptr_t)o8 & 3) == 0) {  // an odd pixel count puts every other frame of the byte output off the dword grid
        uint32_t* w8 = reinterpret_cast<uint32_t*>(o8);
        w8[0] = q[0]; w8[1] = q[1]; w8[2] = q[2];
      } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) o8[i] = by[i];
      }
    }
  } else {
    const int cnt = d.pixels - p0 < 4 ? (int)(d.pixels - p0) : 4;
    for (int j = 0; j < cnt; ++j) {
      const uint8_t r = in[(p0 + j) * 3], g = in[(p0 + j) * 3 + 1], bl = in[(p0 + j) * 3 + 2];
      rg_store_pixel(o + j * 8, r, g, bl, mul, add);
      if (o8) { o8[j * 3] = r; o8[j * 3 + 1] = g; o8[j * 3 + 2] = bl; }
    }
  }
}

}  // namespace

extern "C" {

int32_t gn_replay_gather(gn_ctx* ctx, const gn_replay_gather_desc* dp) {
  GN_REQUIRE(ctx && dp, "gn_replay_gather: null argument");
  const gn_replay_gather_desc& d = *dp;
  GN_REQUIRE(d.frame_ptr && d.qpos && d.action && d.obs_index && d.first_obs && d.last_tr && d.idx && d.images && d.low_dim_state && d.action_out,
             "gn_replay_gather: null table or output (only images_u8 and the token tables are optional)");
  GN_REQUIRE(!d.tokens_out || (d.lang_tokens && d.episode && d.N_ep > 0 && d.L_tok > 0 && d.L_tok <= (1 << 16) &&
                               (((uintptr_t)d.lang_tokens | (uintptr_t)d.episode | (uintptr_t)d.tokens_out) & 3) == 0),
             "gn_replay_gather: tokens_out needs lang_tokens, episode, N_ep (%d) > 0 and L_tok (%d) > 0", d.N_ep, d.L_tok);
  GN_REQUIRE(d.B > 0 && d.B <= 65535 && d.V > 0 && d.fs > 0 && (int64_t)d.V * d.fs <= 65535, "gn_replay_gather: B (%d), V (%d), fs (%d) out of range", d.B,
             d.V, d.fs);
  GN_REQUIRE(d.T > 0 && d.S > 0 && d.A > 0 && (int64_t)d.T * d.A <= (1 << 24) && (int64_t)d.fs * d.S <= (1 << 24),
             "gn_replay_gather: T (%d), S (%d), A (%d) out of range", d.T, d.S, d.A);
  GN_REQUIRE(d.N > 0 && d.N_obs > 0 && d.N_obs <= INT32_MAX && d.pixels > 0 && cdiv64(cdiv64(d.pixels, 4), RG_THREADS) <= INT32_MAX,
             "gn_replay_gather: N (%d), N_obs (%ld), pixels (%ld) out of range", d.N, (long)d.N_obs, (long)d.pixels);
  GN_REQUIRE(((uintptr_t)d.images & 15) == 0, "gn_replay_gather: images must be 16-byte aligned");
  GN_REQUIRE((((uintptr_t)d.frame_ptr) & 7) == 0 && (((uintptr_t)d.qpos | (uintptr_t)d.action | (uintptr_t)d.obs_index | (uintptr_t)d.first_obs |
                                                       (uintptr_t)d.last_tr | (uintptr_t)d.idx | (uintptr_t)d.low_dim_state | (uintptr_t)d.action_out) & 3) == 0,
             "gn_replay_gather: misaligned table or output");
  hipLaunchKernelGGL(replay_gather_kernel, dim3((unsigned)cdiv64(cdiv64(d.pixels, 4), RG_THREADS), (unsigned)(d.V * d.fs), (unsigned)d.B), dim3(RG_THREADS), 0,
                     ctx->stream, d, 1.0f, 0.0f);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"
