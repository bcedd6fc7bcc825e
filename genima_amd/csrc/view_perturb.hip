// Camera-pose and light perturbation of a batch of views (genima_amd/openloop.py OpenLoopEval(perturb=...), genima_amd/perturb.py): one
// launch warps every view by its own 3x3 homography, resamples it bilinearly and applies a per-channel gain and offset.
// include/genima_hip.h (gn_view_perturb) states the pixel rule; tests/perturb_ref.py restates it in numpy f64 and is compared bit for bit.
//
// One thread per run of four output pixels of one image row, 256 threads per workgroup, blockIdx.y the view.  The run's 12 output bytes go
// out as three dwords and its four `valid` bytes as one where the row's address allows (W % 4 == 0 makes every row allow it); a run that is
// cut by the row's end or is not dword-aligned takes the byte stores of the tail.  The source is a gather of four texels per pixel through
// byte loads; a view fits in L2.  The matrix and the colour row are the same for the whole workgroup, so the compiler reads them with
// scalar loads.
//
// All arithmetic is f64, one rounded operation at a time in the order the header gives: this file is built with -ffp-contract=off (no
// fused multiply-add), the divisions are IEEE divisions and rint rounds half to even.  The revealed count is an integer sum -- wave sum, LDS,
// one atomicAdd per workgroup -- so its bits do not depend on the order of arrival.
//
// gn_view_augment_tiled is the same rule over the trainer's frames: 2 x 2 tiled uint8 frames, stacked or behind a device pointer table (the
// DataLoader's frame cache), every tile an independent view with its own matrix and colour row.  blockIdx.y is (frame, tile); a thread makes
// a run of four pixels of one TILE row, so no run straddles two tiles and no sample leaves its tile (vp_pixel folds and clamps inside the
// H x W tile it is given; the tile's rows are 2 W * 3 bytes apart).  The right-hand tiles begin W * 3 bytes into a row, so the dword / byte
// choice is made per run from the address, as above.  The f16 NHWC-8 copy is one 16-byte store per pixel of image_convert.h's conversion.
#include "image_convert.h"
#include "openloop_common.h"

namespace {

constexpr int VP_RUN = 4;  // output pixels per thread
constexpr double VP_DBL_MAX = 1.7976931348623157e308;

__device__ __forceinline__ bool vp_finite(double v) { return fabs(v) <= VP_DBL_MAX; }  // false for an infinity and for a NaN
__device__ __forceinline__ double vp_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// one reflection about the edge pixel's centre (torch's `reflect`), then the clamp that catches what one reflection leaves outside
__device__ __forceinline__ int vp_fold(int i, int n) {
  if (i < 0) {
    i = -i;
  } else if (i > n - 1) {
    i = 2 * (n - 1) - i;
  }
  return ol_clamp(i, 0, n - 1);
}

// Output pixel (x, y) of one view whose source rows lie `pitch` bytes apart: its three bytes into o[0..2]; returns `valid`.
__device__ __forceinline__ bool vp_pixel(ol_gptr8 src, int pitch, const double* __restrict__ M, const double* __restrict__ col, int x, int y, int H,
                                         int W, uint8_t* o) {
  const double X = (double)x + 0.5, Y = (double)y + 0.5;
  const double a = (M[0] * X + M[1] * Y) + M[2];
  const double c = (M[3] * X + M[4] * Y) + M[5];
  const double w = (M[6] * X + M[7] * Y) + M[8];
  if (!(w > 0.0) || !vp_finite(a) || !vp_finite(c) || !vp_finite(w)) {
    o[0] = o[1] = o[2] = 0;
    return false;
  }
  const double u = a / w, v = c / w;
  const bool valid = u >= 0.0 && u <= (double)W && v >= 0.0 && v <= (double)H;
  const double su = vp_clamp(u - 0.5, -(double)(W - 1), 2.0 * (double)(W - 1));
  const double sv = vp_clamp(v - 0.5, -(double)(H - 1), 2.0 * (double)(H - 1));
  const double fx = floor(su), fy = floor(sv);
  const double tx = su - fx, ty = sv - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const int xa = vp_fold(x0, W), xb = vp_fold(x0 + 1, W), ya = vp_fold(y0, H), yb = vp_fold(y0 + 1, H);
  const ol_gptr8 r0 = src + (long)ya * pitch, r1 = src + (long)yb * pitch;
  const double ux = 1.0 - tx, uy = 1.0 - ty;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double p00 = (double)r0[xa * 3 + ch], p01 = (double)r0[xb * 3 + ch], p10 = (double)r1[xa * 3 + ch], p11 = (double)r1[xb * 3 + ch];
    const double top = p00 * ux + p01 * tx;
    const double bot = p10 * ux + p11 * tx;
    const double cc = top * uy + bot * ty;
    const double t = cc * col[ch] + col[3 + ch];
    const double q = t > 0.0 ? (t > 255.0 ? 255.0 : t) : 0.0;  // clamp(t, 0, 255); a NaN gives 0
    o[ch] = (uint8_t)(int)rint(q);
  }
  return valid;
}

__global__ __launch_bounds__(OL_THREADS) void view_perturb_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint8_t* __restrict__ valid,
                                                                  int* __restrict__ n_revealed, const double* __restrict__ M,
                                                                  const double* __restrict__ colour, int H, int W) {
  __shared__ uint32_t part[OL_THREADS / 64];
  const int b = blockIdx.y;
  const int G = (W + VP_RUN - 1) / VP_RUN;  // runs per image row
  const long t = (long)blockIdx.x * OL_THREADS + threadIdx.x;
  const int y = (int)(t / G), x0 = (int)(t - (long)y * G) * VP_RUN;
  uint32_t revealed = 0;
  if (y < H) {  // no early return: every lane takes part in the wave sum below
    const long view = (long)b * H * W;
    const ol_gptr8 s8 = (ol_gptr8)(src + view * 3);
    const double* m = M + (long)b * 9;
    const double* col = colour + (long)b * 6;
    const long po = view + (long)y * W + x0;  // pixel offset of the run in dst / valid
    uint8_t* o8 = dst + po * 3;
    const int cnt = W - x0 < VP_RUN ? W - x0 : VP_RUN;
    uint8_t by[VP_RUN * 3], ok[VP_RUN];
    if (cnt == VP_RUN) {
#pragma unroll
      for (int j = 0; j < VP_RUN; ++j) ok[j] = vp_pixel(s8, W * 3, m, col, x0 + j, y, H, W, by + j * 3) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < VP_RUN; ++j) revealed += ok[j] ? 0u : 1u;
      if (((uintptr_t)o8 & 3) == 0) {
        uint32_t q[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
          q[i] = (uint32_t)by[i * 4] | ((uint32_t)by[i * 4 + 1] << 8) | ((uint32_t)by[i * 4 + 2] << 16) | ((uint32_t)by[i * 4 + 3] << 24);
        uint32_t* ow = reinterpret_cast<uint32_t*>(o8);
        ow[0] = q[0];
        ow[1] = q[1];
        ow[2] = q[2];
      } else {
#pragma unroll
        for (int i = 0; i < VP_RUN * 3; ++i) o8[i] = by[i];
      }
      if (valid) {
        uint8_t* v8 = valid + po;
        if (((uintptr_t)v8 & 3) == 0) {
          *reinterpret_cast<uint32_t*>(v8) = (uint32_t)ok[0] | ((uint32_t)ok[1] << 8) | ((uint32_t)ok[2] << 16) | ((uint32_t)ok[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < VP_RUN; ++j) v8[j] = ok[j];
        }
      }
    } else {  // the row's last, shorter run
      for (int j = 0; j < cnt; ++j) {
        uint8_t px[3];
        const bool k = vp_pixel(s8, W * 3, m, col, x0 + j, y, H, W, px);
        revealed += k ? 0u : 1u;
        o8[j * 3] = px[0];
        o8[j * 3 + 1] = px[1];
        o8[j * 3 + 2] = px[2];
        if (valid) valid[po + j] = k ? 1 : 0;
      }
    }
  }
  if (n_revealed) {  // the same for every thread of the launch
    const uint32_t s = ol_wave_sum(revealed);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < OL_THREADS / 64; ++w) total += part[w];
      if (total) atomicAdd(n_revealed + b, (int)total);
    }
  }
}

__device__ __forceinline__ void va_store_f16(f16* __restrict__ o, const uint8_t* px, float mul, float add) {
  const f16 z = (f16)0.0f;
  *reinterpret_cast<f16x8*>(o) = f16x8{u8_to_f16_value(px[0], mul, add), u8_to_f16_value(px[1], mul, add), u8_to_f16_value(px[2], mul, add), z, z, z, z, z};
}

// blockIdx.y = frame * 4 + tile; src (stacked) or frames (a pointer table), one of them NULL.  H, W: the TILE's size.
__global__ __launch_bounds__(OL_THREADS) void view_augment_tiled_kernel(const uint8_t* __restrict__ src, const uint8_t* const* __restrict__ frames,
                                                                        uint8_t* __restrict__ dst, f16* __restrict__ dst_f16,
                                                                        uint8_t* __restrict__ valid, int* __restrict__ n_revealed,
                                                                        const double* __restrict__ M, const double* __restrict__ colour, int H, int W,
                                                                        float mul, float add) {
  __shared__ uint32_t part[OL_THREADS / 64];
  const int b = blockIdx.y, i = b >> 2, tile = b & 3;
  const int G = (W + VP_RUN - 1) / VP_RUN;  // runs per tile row
  const long t = (long)blockIdx.x * OL_THREADS + threadIdx.x;
  const int y = (int)(t / G), x0 = (int)(t - (long)y * G) * VP_RUN;
  uint32_t revealed = 0;
  if (y < H) {  // no early return: every lane takes part in the wave sum below
    const int pitch = 2 * W * 3;
    const long frame_px = (long)4 * H * W;
    const long tile_px = (long)(tile >> 1) * H * (2 * W) + (long)(tile & 1) * W;  // the tile's first pixel inside its frame
    const ol_gptr8 s8 = (ol_gptr8)(frames ? frames[i] : src + (long)i * frame_px * 3) + tile_px * 3;
    const double* m = M + (long)b * 9;
    const double* col = colour + (long)b * 6;
    const long po = (long)i * frame_px + tile_px + (long)y * (2 * W) + x0;  // pixel offset of the run in dst / dst_f16 / valid
    const int cnt = W - x0 < VP_RUN ? W - x0 : VP_RUN;
    uint8_t by[VP_RUN * 3], ok[VP_RUN];
    if (cnt == VP_RUN) {
#pragma unroll
      for (int j = 0; j < VP_RUN; ++j) ok[j] = vp_pixel(s8, pitch, m, col, x0 + j, y, H, W, by + j * 3) ? 1 : 0;
#pragma unroll
      for (int j = 0; j < VP_RUN; ++j) revealed += ok[j] ? 0u : 1u;
      if (dst) {
        uint8_t* o8 = dst + po * 3;
        if (((uintptr_t)o8 & 3) == 0) {
          uint32_t* ow = reinterpret_cast<uint32_t*>(o8);
#pragma unroll
          for (int k = 0; k < 3; ++k)
            ow[k] = (uint32_t)by[k * 4] | ((uint32_t)by[k * 4 + 1] << 8) | ((uint32_t)by[k * 4 + 2] << 16) | ((uint32_t)by[k * 4 + 3] << 24);
        } else {
#pragma unroll
          for (int k = 0; k < VP_RUN * 3; ++k) o8[k] = by[k];
        }
      }
      if (dst_f16) {
#pragma unroll
        for (int j = 0; j < VP_RUN; ++j) va_store_f16(dst_f16 + (po + j) * 8, by + j * 3, mul, add);
      }
      if (valid) {
        uint8_t* v8 = valid + po;
        if (((uintptr_t)v8 & 3) == 0) {
          *reinterpret_cast<uint32_t*>(v8) = (uint32_t)ok[0] | ((uint32_t)ok[1] << 8) | ((uint32_t)ok[2] << 16) | ((uint32_t)ok[3] << 24);
        } else {
#pragma unroll
          for (int j = 0; j < VP_RUN; ++j) v8[j] = ok[j];
        }
      }
    } else {  // the tile row's last, shorter run
      for (int j = 0; j < cnt; ++j) {
        uint8_t px[3];
        const bool k = vp_pixel(s8, pitch, m, col, x0 + j, y, H, W, px);
        revealed += k ? 0u : 1u;
        if (dst) {
          uint8_t* o8 = dst + (po + j) * 3;
          o8[0] = px[0];
          o8[1] = px[1];
          o8[2] = px[2];
        }
        if (dst_f16) va_store_f16(dst_f16 + (po + j) * 8, px, mul, add);
        if (valid) valid[po + j] = k ? 1 : 0;
      }
    }
  }
  if (n_revealed) {  // the same for every thread of the launch
    const uint32_t s = ol_wave_sum(revealed);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < OL_THREADS / 64; ++w) total += part[w];
      if (total) atomicAdd(n_revealed + b, (int)total);
    }
  }
}

}  // namespace

extern "C" {

int32_t gn_view_perturb(gn_ctx* ctx, const uint8_t* src, uint8_t* dst, uint8_t* valid, int32_t* n_revealed, const double* M, const double* colour,
                        int32_t B, int32_t H, int32_t W) {
  GN_REQUIRE(ctx && src && dst && M && colour, "gn_view_perturb: null argument");
  GN_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && (int64_t)B * H * W * 3 <= INT32_MAX,
             "gn_view_perturb: B (%d), H (%d), W (%d) must be positive, B at most 65535 and B * H * W * 3 below 2^31", B, H, W);
  const uintptr_t bytes = (uintptr_t)B * H * W * 3, s = (uintptr_t)src, d = (uintptr_t)dst;
  GN_REQUIRE(s + bytes <= d || d + bytes <= s, "gn_view_perturb: dst must not overlap src (a warp reads pixels other threads write)");
  GN_REQUIRE((((uintptr_t)M | (uintptr_t)colour) & 7) == 0 && ((uintptr_t)n_revealed & 3) == 0,
             "gn_view_perturb: M and colour must be 8-byte aligned and n_revealed 4-byte aligned");
  if (n_revealed) GN_HIP(hipMemsetAsync(n_revealed, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  const int64_t threads = (int64_t)H * ((W + VP_RUN - 1) / VP_RUN);
  hipLaunchKernelGGL(view_perturb_kernel, dim3((unsigned)cdiv64(threads, OL_THREADS), (unsigned)B), dim3(OL_THREADS), 0, ctx->stream, src, dst, valid,
                     (int*)n_revealed, M, colour, H, W);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_view_augment_tiled(gn_ctx* ctx, const uint8_t* src, const uint8_t* const* frames, uint8_t* dst, void* dst_f16, uint8_t* valid,
                              int32_t* n_revealed, const double* M, const double* colour, int32_t n, int32_t H, int32_t W, float mul, float add) {
  GN_REQUIRE(ctx && M && colour, "gn_view_augment_tiled: null ctx, M or colour");
  GN_REQUIRE((src != nullptr) != (frames != nullptr), "gn_view_augment_tiled: exactly one of src and frames must be given");
  GN_REQUIRE(dst || dst_f16, "gn_view_augment_tiled: no output given (dst and dst_f16 are both NULL)");
  GN_REQUIRE(n > 0 && H > 0 && W > 0 && (int64_t)n * 4 <= 65535 && (int64_t)n * 4 * H * W * 3 <= INT32_MAX,
             "gn_view_augment_tiled: n (%d), H (%d), W (%d) must be positive, 4 n at most 65535 and n * 2H * 2W * 3 below 2^31", n, H, W);
  GN_REQUIRE((((uintptr_t)M | (uintptr_t)colour | (uintptr_t)frames) & 7) == 0 && ((uintptr_t)n_revealed & 3) == 0 && ((uintptr_t)dst_f16 & 15) == 0,
             "gn_view_augment_tiled: M, colour and frames must be 8-byte aligned, n_revealed 4-byte and dst_f16 16-byte aligned");
  GN_REQUIRE(mul - mul == 0.0f && add - add == 0.0f,  // an infinity or a NaN minus itself is a NaN
"gn_view_augment_tiled: mul and add must be finite");
  if (src && dst) {
    const uintptr_t bytes = (uintptr_t)n * 4 * H * W * 3, s = (uintptr_t)src, d = (uintptr_t)dst;
    GN_REQUIRE(s + bytes <= d || d + bytes <= s, "gn_view_augment_tiled: dst must not overlap src (a warp reads pixels other threads write)");
  }
  if (n_revealed) GN_HIP(hipMemsetAsync(n_revealed, 0, (size_t)n * 4 * sizeof(int32_t), ctx->stream));
  const int64_t threads = (int64_t)H * ((W + VP_RUN - 1) / VP_RUN);
  hipLaunchKernelGGL(view_augment_tiled_kernel, dim3((unsigned)cdiv64(threads, OL_THREADS), (unsigned)(n * 4)), dim3(OL_THREADS), 0, ctx->stream, src,
                     frames, dst, (f16*)dst_f16, valid, (int*)n_revealed, M, colour, H, W, mul, add);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"
