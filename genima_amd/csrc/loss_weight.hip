// Sphere-weighted ControlNet loss (ControlNetTrainer.attach_frozen(..., sphere_loss_weight=)): an extension of the reference, off by default.
// include/genima_hip.h states the three rules; this file is compiled without fma contraction, so every product and sum below is one rounded
// f32 / f64 operation, which tests/sphere_loss_ref.py restates in numpy.
//
// Mask kernel (gn_change_mask).  One thread per pixel, grid-stride over B * H * W.  An NHWC-8 operand on the 16-byte grid is read with one
// 16-byte load per pixel; any other leading dimension takes three 2-byte loads.  The mask pixel leaves as one 16-byte store (channel 0 the
// flag, channels 1..7 zero), so the mask is a plain NHWC-8 tensor for gn_affine_nearest / gn_reflect_pad_crop.
//
// Pool kernel (gn_loss_weight_pool).  One thread per latent pixel walks its F x F block of the mask, reading channel 0 alone (2 bytes: the other
// 14 bytes of a mask pixel say nothing, and neighbouring lanes cover the cache line between them).  The block's counts meet as integers: DPP
// adds inside a wave, LDS between the four waves, one 64-bit vector atomic per block on the word the entry point zeroes on the same stream.
// Integer addition commutes, so the total has the same bits in any arrival order.  A one-thread kernel behind it turns the total into wsum.
// No thread leaves before the fold.
//
// Loss kernel (gn_mse_loss_weighted).  gn_mse_loss's two stages: 256 blocks of 256 threads leave one partial each, one wave adds the partials
// in f64 in a fixed order.  With ld_pred == 8 on the 16-byte grid a thread owns a pixel: one 16-byte load of pred, one 16- or 8-byte load of
// target (ld_target 8 or 4), one 16-byte store of dpred; other layouts take gn_mse_loss's element walk.  The gradient scale is formed in the
// kernel from wsum[0] in device memory: the host never reads it.
//
// Parts kernels (gn_mse_loss_parts; attach_frozen(loss_parts=), ControlNetTrainer.eval_loss).  The UNWEIGHTED squared error of a step split
// into marked / unmarked share per sample and added into the row of a device f64 table the sample's bucket names.  f64 throughout (131 k
// elements per step: not a bandwidth exercise), two stages in a fixed order, no floating-point atomics: two runs give the same bits.
#include "common.h"

#include <math.h>

namespace {

constexpr int LW_THREADS = 256;
constexpr int LW_MAX_BLOCKS = 2048;  // 8 workgroups per CU, grid-stride beyond
constexpr int LW_LOSS_BLOCKS = 256;  // = gn_mse_loss's partial count (same workspace)

template <int CTRL>
__device__ __forceinline__ uint32_t lw_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// common.h's wave_sum on unsigned integers: every lane gets the wave's total; all 64 lanes must be active
__device__ __forceinline__ uint32_t lw_wave_sum(uint32_t v) {
  v += lw_dpp<0xB1>(v);
  v += lw_dpp<0x4E>(v);
  v += lw_dpp<0x141>(v);
  v += lw_dpp<0x140>(v);
  const int b = (int)v;
  return ((uint32_t)__builtin_amdgcn_readlane(b, 0) + (uint32_t)__builtin_amdgcn_readlane(b, 16)) +
         ((uint32_t)__builtin_amdgcn_readlane(b, 32) + (uint32_t)__builtin_amdgcn_readlane(b, 48));
}

// the byte an f16 image value was made from: clamp(rint(x * mul + add), 0, 255), a NaN -> 0 (fmaxf drops it)
__device__ __forceinline__ float lw_byte(f16 x, float mul, float add) {
  return fminf(fmaxf(rintf(__fadd_rn(__fmul_rn((float)x, mul), add)), 0.0f), 255.0f);
}

// the f16 nearest to a * b: the product of two f32 values is exact in f64, so it is rounded ONCE.  gn_mse_loss's `(f16)(gscale * d)` compiles to
// one v_fma_mixlo_f16, which rounds the exact product once as well, so with weight 1 the two kernels agree bit for bit; rounding the product to
// f32 first and then to f16 differs from that by one f16 step in about one element in 500 (measured: 555 of 294 912).
__device__ __forceinline__ f16 lw_mul_to_f16(float a, float b) { return (f16)((double)a * (double)b); }

__device__ __forceinline__ void lw_load3(const f16* __restrict__ p, long px, int ld, bool vec, f16 (&v)[3]) {
  if (vec) {
    const uint4 raw = reinterpret_cast<const uint4*>(p)[px];
    const f16x8 q = *reinterpret_cast<const f16x8*>(&raw);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
  } else {
    const f16* r = p + px * ld;
    v[0] = r[0]; v[1] = r[1]; v[2] = r[2];
  }
}

__global__ __launch_bounds__(LW_THREADS) void change_mask_kernel(const f16* __restrict__ target, const f16* __restrict__ cond, uint4* __restrict__ mask,
                                                                 long pixels, int ld_t, int ld_c, int vec_t, int vec_c, float t_mul, float t_add,
                                                                 float c_mul, float c_add, float threshold) {
  for (long px = (long)blockIdx.x * LW_THREADS + threadIdx.x; px < pixels; px += (long)gridDim.x * LW_THREADS) {
    f16 t[3], c[3];
    lw_load3(target, px, ld_t, vec_t != 0, t);
    lw_load3(cond, px, ld_c, vec_c != 0, c);
    float d = 0.0f;  // exact small integers in f32: at most 3 * 255
#pragma unroll
    for (int k = 0; k < 3; ++k) d = __fadd_rn(d, fabsf(__fsub_rn(lw_byte(t[k], t_mul, t_add), lw_byte(c[k], c_mul, c_add))));
    mask[px] = make_uint4(d > threshold ? 0x3C00u : 0u, 0u, 0u, 0u);  // f16 1.0 in channel 0
  }
}

__global__ __launch_bounds__(LW_THREADS) void loss_weight_pool_kernel(const uint16_t* __restrict__ mask, long ld_m, float* __restrict__ weight,
                                                                      unsigned long long* __restrict__ count_total, long latent_pixels, int H, int W,
                                                                      int h, int w, int F, float lambda) {
  __shared__ uint32_t red[LW_THREADS / 64];
  const float ff = (float)(F * F);
  uint32_t mine = 0;  // <= 256 per latent pixel, <= 2^15 latent pixels per thread (the entry point bounds them): a wave's total fits 32 bits
  const long stride = (long)gridDim.x * LW_THREADS;
  for (long base = (long)blockIdx.x * LW_THREADS; base < latent_pixels; base += stride) {  // block-uniform trip count
    const long lp = base + threadIdx.x;
    if (lp < latent_pixels) {
      const int x = (int)(lp % w);
      const long r = lp / w;
      const int y = (int)(r % h);
      const long b = r / h;
      const uint16_t* p = mask + ((b * H + (long)y * F) * W + (long)x * F) * ld_m;
      uint32_t n = 0;
      for (int fy = 0; fy < F; ++fy)
        for (int fx = 0; fx < F; ++fx) n += (p[((long)fy * W + fx) * ld_m] & 0x7FFFu) != 0 ? 1u : 0u;  // != 0 as f16 compares it: -0 equals 0, a NaN does not
      weight[lp] = __fadd_rn(1.0f, __fmul_rn(lambda, __fdiv_rn((float)n, ff)));
      mine += n;
    }
  }
  const uint32_t s = lw_wave_sum(mine);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long tot = (unsigned long long)red[0] + red[1] + red[2] + red[3];
    if (tot) atomicAdd(count_total, tot);
  }
}

__global__ void loss_weight_wsum_kernel(const long long* __restrict__ count_total, double* __restrict__ wsum, double latent_pixels, double lambda, double ff) {
  if (blockIdx.x == 0 && threadIdx.x == 0) wsum[0] = latent_pixels + lambda * (double)count_total[0] / ff;
}

// VEC: ld_pred == 8, pred / dpred on the 16-byte grid, C <= 8; tvec = 2: target NHWC-8 on the 16-byte grid, 1: NHWC-4 on the 8-byte grid, 0: 2-byte loads
template <bool VEC>
__global__ __launch_bounds__(LW_THREADS) void mse_weighted_partial_kernel(const f16* __restrict__ pred, const f16* __restrict__ target,
                                                                          const float* __restrict__ weight, const double* __restrict__ wsum,
                                                                          f16* __restrict__ dpred, float* __restrict__ part, long pixels, int C, int ldp,
                                                                          int ldt, int tvec, float gscale2) {
  __shared__ float red[LW_THREADS / 64];
  const float gs = __fdiv_rn(gscale2, (float)((double)C * wsum[0]));
  float s = 0.f;
  if constexpr (VEC) {
    for (long px = (long)blockIdx.x * LW_THREADS + threadIdx.x; px < pixels; px += (long)gridDim.x * LW_THREADS) {
      const uint4 rp = reinterpret_cast<const uint4*>(pred)[px];
      const f16x8 p = *reinterpret_cast<const f16x8*>(&rp);
      f16x8 t = {0, 0, 0, 0, 0, 0, 0, 0};
      if (tvec == 2) {
        const uint4 rt = reinterpret_cast<const uint4*>(target)[px];
        t = *reinterpret_cast<const f16x8*>(&rt);
      } else if (tvec == 1) {
        const uint2 rt = reinterpret_cast<const uint2*>(target)[px];
        const f16x4 q = *reinterpret_cast<const f16x4*>(&rt);
        t[0] = q[0]; t[1] = q[1]; t[2] = q[2]; t[3] = q[3];
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < C) t[c] = target[px * ldt + c];
      }
      const float wt = weight[px];
      const float gw = __fmul_rn(gs, wt);
      f16x8 o;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float d = 0.f;
        if (c < C) {
          d = __fsub_rn((float)p[c], (float)t[c]);
          s = __fadd_rn(s, __fmul_rn(__fmul_rn(wt, d), d));
        }
        o[c] = lw_mul_to_f16(gw, d);
      }
      if (dpred) reinterpret_cast<uint4*>(dpred)[px] = *reinterpret_cast<const uint4*>(&o);
    }
  } else {
    for (long i = (long)blockIdx.x * LW_THREADS + threadIdx.x; i < pixels * ldp; i += (long)gridDim.x * LW_THREADS) {
      const long px = i / ldp;
      const int c = (int)(i - px * ldp);
      const float wt = weight[px];
      float d = 0.f;
      if (c < C) {
        d = __fsub_rn((float)pred[i], (float)target[px * ldt + c]);
        s = __fadd_rn(s, __fmul_rn(__fmul_rn(wt, d), d));
      }
      if (dpred) dpred[i] = lw_mul_to_f16(__fmul_rn(gs, wt), d);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// backward.hip's sum_small_kernel with the weighted mean's denominator: one wave, lane l adds part[l], part[l + 64], ... in f64, then a fixed
// butterfly over the lanes
__global__ void mse_weighted_final_kernel(const float* __restrict__ part, const double* __restrict__ wsum, float* __restrict__ out, int n, int C) {
  if (blockIdx.x != 0) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += (double)part[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) out[0] = (float)(s / ((double)C * wsum[0]));
}

// ---- loss parts (gn_mse_loss_parts): a read-out, not a loss.  Stage one: workgroup (b, r) owns the LP_THREADS contiguous latent pixels
// [r * LP_THREADS, (r + 1) * LP_THREADS) of sample b, one pixel per thread.  A thread past the sample's last pixel carries zeros INTO the
// lane tree, so all 64 lanes of every wave take the same fixed butterfly; the four waves meet in LDS and thread 0 adds them in wave order.
constexpr int LP_THREADS = 256;

__device__ __forceinline__ double lp_wave_sum(double v) {  // fixed xor butterfly; all 64 lanes must be active
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(LP_THREADS) void mse_parts_partial_kernel(const f16* __restrict__ pred, const f16* __restrict__ target,
                                                                       const uint16_t* __restrict__ mask, double* __restrict__ part, long hw, int ranges,
                                                                       int w, int C, int ldp, int ldt, int H, int W, long ld_m, int F) {
  __shared__ double red[3][LP_THREADS / 64];
  const long b = blockIdx.x / ranges;
  const long p = (long)(blockIdx.x % ranges) * LP_THREADS + threadIdx.x;
  double S = 0.0, G = 0.0, n_d = 0.0;
  if (p < hw) {
    const long px = b * hw + p;
    const f16* pp = pred + px * ldp;
    const f16* tp = target + px * ldt;
    double e = 0.0;
    for (int c = 0; c < C; ++c) {
      const float d = __fsub_rn((float)pp[c], (float)tp[c]);
      e += (double)d * (double)d;  // the product of two f32 values is exact in f64
    }
    uint32_t n = 0;
    if (mask) {
      const int x = (int)(p % w);
      const long y = p / w;
      const uint16_t* m = mask + ((b * H + y * F) * W + (long)x * F) * ld_m;
      for (int fy = 0; fy < F; ++fy)
        for (int fx = 0; fx < F; ++fx) n += (m[((long)fy * W + fx) * ld_m] & 0x7FFFu) != 0 ? 1u : 0u;  // gn_loss_weight_pool's != 0
    }
    const double s = (double)n / (double)(F * F);
    S = s * e;
    G = (1.0 - s) * e;
    n_d = (double)n;  // an integer below 2^53 all the way to the table: exact
  }
  S = lp_wave_sum(S);
  G = lp_wave_sum(G);
  n_d = lp_wave_sum(n_d);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = S;
    red[1][threadIdx.x >> 6] = G;
    red[2][threadIdx.x >> 6] = n_d;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) part[(long)blockIdx.x * 3 + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
  }
}

// Stage two, one workgroup: thread i adds the partials of samples i, i + LP_THREADS, ... in range order and leaves the sample's sums in its
// first partial; then thread 0 alone adds the samples into their rows, b = 0 .. B - 1.  No atomics: the order is the program's.
__global__ __launch_bounds__(LP_THREADS) void mse_parts_final_kernel(double* __restrict__ part, const int32_t* __restrict__ bucket,
                                                                     double* __restrict__ table, int B, int ranges, int n_buckets, double ff, double hw) {
  if (blockIdx.x != 0) return;
  for (int b = threadIdx.x; b < B; b += LP_THREADS) {
    double* q = part + (long)b * ranges * 3;
    double s = q[0], g = q[1], n = q[2];
    for (int r = 1; r < ranges; ++r) {
      s += q[r * 3L];
      g += q[r * 3L + 1];
      n += q[r * 3L + 2];
    }
    q[0] = s; q[1] = g; q[2] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int b = 0; b < B; ++b) {
      const double* q = part + (long)b * ranges * 3;
      const int32_t k = bucket[b];
      double* row = table + (long)((k >= 0 && k < n_buckets) ? k : n_buckets) * 5;
      row[0] += q[0];
      row[1] += q[1];
      row[2] += q[2] / ff;
      row[3] += hw;
      row[4] += 1.0;
    }
  }
}

inline int64_t lp_ranges(int64_t hw) { return cdiv64(hw, LP_THREADS); }

inline unsigned lw_blocks(int64_t items) {
  const int64_t b = cdiv64(items, LW_THREADS);
  return (unsigned)(b < LW_MAX_BLOCKS ? b : LW_MAX_BLOCKS);
}

}  // namespace

extern "C" {

int32_t gn_change_mask(gn_ctx* ctx, const void* target, const void* cond, void* mask, int32_t B, int32_t H, int32_t W, int32_t ld_t, int32_t ld_c,
                       float t_mul, float t_add, float c_mul, float c_add, int32_t threshold) {
  GN_REQUIRE(ctx && target && cond && mask, "gn_change_mask: null argument");
  GN_REQUIRE(B > 0 && H > 0 && W > 0, "gn_change_mask: B (%d), H (%d), W (%d) must be positive", B, H, W);
  GN_REQUIRE(ld_t >= 3 && ld_c >= 3, "gn_change_mask: ld_t (%d) and ld_c (%d) must be at least 3", ld_t, ld_c);
  GN_REQUIRE(threshold >= 0, "gn_change_mask: threshold (%d) must not be negative", threshold);
  GN_REQUIRE(isfinite(t_mul) && isfinite(t_add) && isfinite(c_mul) && isfinite(c_add), "gn_change_mask: scales and offsets must be finite");
  GN_REQUIRE(((uintptr_t)target & 1) == 0 && ((uintptr_t)cond & 1) == 0 && ((uintptr_t)mask & 15) == 0,
             "gn_change_mask: target / cond must be 2-byte and mask 16-byte aligned");
  const int64_t pixels = (int64_t)B * H * W;
  const int vec_t = ld_t == 8 && ((uintptr_t)target & 15) == 0, vec_c = ld_c == 8 && ((uintptr_t)cond & 15) == 0;
  hipLaunchKernelGGL(change_mask_kernel, dim3(lw_blocks(pixels)), dim3(LW_THREADS), 0, ctx->stream, (const f16*)target, (const f16*)cond, (uint4*)mask,
                     (long)pixels, ld_t, ld_c, vec_t, vec_c, t_mul, t_add, c_mul, c_add, (float)threshold);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_loss_weight_pool(gn_ctx* ctx, const void* mask, int32_t ld_m, float* weight, int64_t* count_total, double* wsum, int32_t B, int32_t H,
                            int32_t W, int32_t h, int32_t w, float lambda) {
  GN_REQUIRE(ctx && mask && weight && count_total && wsum, "gn_loss_weight_pool: null argument");
  GN_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && ld_m >= 1, "gn_loss_weight_pool: B (%d), H (%d), W (%d), h (%d), w (%d), ld_m (%d) must be positive",
             B, H, W, h, w, ld_m);
  GN_REQUIRE(H % h == 0 && W % w == 0 && H / h == W / w && H / h <= 16,
             "gn_loss_weight_pool: H / h (%d / %d) and W / w (%d / %d) must be one whole factor in 1 .. 16", H, h, W, w);
  GN_REQUIRE(lambda >= 0.0f && isfinite(lambda), "gn_loss_weight_pool: lambda must be finite and not negative");  // (a NaN fails the comparison)
  GN_REQUIRE(((uintptr_t)mask & 1) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)count_total & 7) == 0 && ((uintptr_t)wsum & 7) == 0,
             "gn_loss_weight_pool: mask must be 2-byte, weight 4-byte, count_total and wsum 8-byte aligned");
  const int F = H / h;
  const int64_t latent = (int64_t)B * h * w;
  // a wave's count stays in 32 bits: at most 256 per latent pixel, 2^34 / (2048 * 256) = 2^15 latent pixels per thread, 64 lanes
  GN_REQUIRE(latent <= ((int64_t)1 << 34), "gn_loss_weight_pool: B * h * w (%ld) too large", (long)latent);
  GN_HIP(hipMemsetAsync(count_total, 0, sizeof(int64_t), ctx->stream));
  hipLaunchKernelGGL(loss_weight_pool_kernel, dim3(lw_blocks(latent)), dim3(LW_THREADS), 0, ctx->stream, (const uint16_t*)mask, (long)ld_m, weight,
                     (unsigned long long*)count_total, (long)latent, H, W, h, w, F, lambda);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_weight_wsum_kernel, dim3(1), dim3(64), 0, ctx->stream, (const long long*)count_total, wsum, (double)latent, (double)lambda,
                     (double)(F * F));
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_mse_loss_weighted(gn_ctx* ctx, const void* pred, const void* target, const float* weight, const double* wsum, void* dpred, float* loss_out,
                             void* workspace, int64_t pixels, int32_t C, int32_t ld_pred, int32_t ld_target, float grad_scale) {
  GN_REQUIRE(ctx && pred && target && weight && wsum && loss_out && workspace, "gn_mse_loss_weighted: null argument");
  GN_REQUIRE(pixels > 0 && C > 0 && ld_pred >= C && ld_target >= C, "gn_mse_loss_weighted: pixels (%ld), C (%d), ld_pred (%d), ld_target (%d) out of range",
             (long)pixels, C, ld_pred, ld_target);
  GN_REQUIRE(((uintptr_t)wsum & 7) == 0 && ((uintptr_t)weight & 3) == 0 && ((uintptr_t)loss_out & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
             "gn_mse_loss_weighted: wsum must be 8-byte, weight / loss_out / workspace 4-byte aligned");
  const float gscale2 = grad_scale * 2.0f;
  const bool vec = ld_pred == 8 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)dpred & 15) == 0;
  const int tvec = ld_target == 8 && ((uintptr_t)target & 15) == 0 ? 2 : (ld_target == 4 && ((uintptr_t)target & 7) == 0 ? 1 : 0);
  if (vec)
    hipLaunchKernelGGL(mse_weighted_partial_kernel<true>, dim3(LW_LOSS_BLOCKS), dim3(LW_THREADS), 0, ctx->stream, (const f16*)pred, (const f16*)target, weight,
                       wsum, (f16*)dpred, (float*)workspace, (long)pixels, C, ld_pred, ld_target, tvec, gscale2);
  else
    hipLaunchKernelGGL(mse_weighted_partial_kernel<false>, dim3(LW_LOSS_BLOCKS), dim3(LW_THREADS), 0, ctx->stream, (const f16*)pred, (const f16*)target, weight,
                       wsum, (f16*)dpred, (float*)workspace, (long)pixels, C, ld_pred, ld_target, tvec, gscale2);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(mse_weighted_final_kernel, dim3(1), dim3(64), 0, ctx->stream, (const float*)workspace, wsum, loss_out, LW_LOSS_BLOCKS, C);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int64_t gn_mse_loss_parts_workspace_bytes(int32_t B, int32_t h, int32_t w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (int64_t)B * lp_ranges((int64_t)h * w) * 3 * (int64_t)sizeof(double);
}

int32_t gn_mse_loss_parts(gn_ctx* ctx, const void* pred, const void* target, const void* mask, const int32_t* bucket, double* table, void* workspace,
                          int32_t B, int32_t h, int32_t w, int32_t C, int32_t ld_pred, int32_t ld_target, int32_t H, int32_t W, int32_t ld_m,
                          int32_t n_buckets) {
  GN_REQUIRE(ctx && pred && target && bucket && table && workspace, "gn_mse_loss_parts: null argument");
  GN_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && ld_pred > 0 && ld_target > 0,
             "gn_mse_loss_parts: B (%d), h (%d), w (%d), C (%d), ld_pred (%d), ld_target (%d) must be positive", B, h, w, C, ld_pred, ld_target);
  GN_REQUIRE(C <= ld_pred && C <= ld_target, "gn_mse_loss_parts: C (%d) exceeds ld_pred (%d) or ld_target (%d)", C, ld_pred, ld_target);
  GN_REQUIRE(n_buckets >= 1, "gn_mse_loss_parts: n_buckets (%d) must be at least 1", n_buckets);
  int F = 1;
  if (mask) {
    GN_REQUIRE(H > 0 && W > 0 && ld_m > 0, "gn_mse_loss_parts: H (%d), W (%d), ld_m (%d) must be positive with a mask", H, W, ld_m);
    GN_REQUIRE(H % h == 0 && W % w == 0 && H / h == W / w && H / h <= 16,
               "gn_mse_loss_parts: H / h (%d / %d) and W / w (%d / %d) must be one whole factor in 1 .. 16", H, h, W, w);
    F = H / h;
  }
  GN_REQUIRE(((uintptr_t)pred & 1) == 0 && ((uintptr_t)target & 1) == 0 && ((uintptr_t)mask & 1) == 0 && ((uintptr_t)bucket & 3) == 0 &&
                 ((uintptr_t)table & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
             "gn_mse_loss_parts: pred / target / mask must be 2-byte, bucket 4-byte, table and workspace 8-byte aligned");
  const int64_t hw = (int64_t)h * w, ranges = lp_ranges(hw);
  GN_REQUIRE(B * ranges <= 0x7FFFFFFF, "gn_mse_loss_parts: B * h * w (%ld) too large", (long)(B * hw));
  hipLaunchKernelGGL(mse_parts_partial_kernel, dim3((unsigned)(B * ranges)), dim3(LP_THREADS), 0, ctx->stream, (const f16*)pred, (const f16*)target,
                     (const uint16_t*)mask, (double*)workspace, (long)hw, (int)ranges, w, C, ld_pred, ld_target, H, W, (long)ld_m, F);
  GN_LAUNCH_CHECK();
  hipLaunchKernelGGL(mse_parts_final_kernel, dim3(1), dim3(LP_THREADS), 0, ctx->stream, (double*)workspace, bucket, table, B, (int)ranges, n_buckets,
                     (double)(F * F), (double)hw);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"
