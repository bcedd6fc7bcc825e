// What the open-loop score kernels share (openloop.hip, openloop_orient.hip, openloop_seeds.hip): the workgroup size, global-load pointer
// types, the integer wave sum, the window clamp and the optional host check of a window table.  All three are built with -ffp-contract=off.
#pragma once
#include "common.h"

constexpr int OL_THREADS = 256;
constexpr int OL_WIN_MAX = 256;  // a window's longest side

typedef const __attribute__((address_space(1))) uint8_t* ol_gptr8;  // global_load, not flat_load
typedef const __attribute__((address_space(1))) uint32_t* ol_gptr32;

template <int CTRL>
__device__ __forceinline__ uint32_t ol_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// common.h's wave_sum on unsigned integers: every lane gets the wave's total; all 64 lanes must be active
__device__ __forceinline__ uint32_t ol_wave_sum(uint32_t v) {
  v += ol_dpp<0xB1>(v);
  v += ol_dpp<0x4E>(v);
  v += ol_dpp<0x141>(v);
  v += ol_dpp<0x140>(v);
  const int b = (int)v;
  return ((uint32_t)__builtin_amdgcn_readlane(b, 0) + (uint32_t)__builtin_amdgcn_readlane(b, 16)) +
         ((uint32_t)__builtin_amdgcn_readlane(b, 32) + (uint32_t)__builtin_amdgcn_readlane(b, 48));
}

__device__ __forceinline__ int ol_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The check gn_openloop_sphere_metrics and gn_openloop_orientation make of the optional HOST copy of their n windows (x0, y0, x1, y1): GN_OK,
// or GN_ERR_INVALID with the error text set.  A window that passes is one the kernels' clamp leaves as it is.
inline int32_t ol_check_windows(const char* who, const int32_t* win_host, int64_t n, int W, int H) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* q = win_host + i * 4;
    GN_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[2] >= q[0] && q[3] >= q[1] && q[2] <= W && q[3] <= H && q[2] - q[0] <= OL_WIN_MAX && q[3] - q[1] <= OL_WIN_MAX,
               "%s: window %ld = (%d, %d, %d, %d) must lie inside the %d x %d image with x0 <= x1, y0 <= y1 and at most %d per side", who, (long)i, q[0], q[1],
               q[2], q[3], W, H, OL_WIN_MAX);
  }
  return GN_OK;
}
