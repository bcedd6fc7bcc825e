// 8-bit blockwise AdamW on the flat training buffers (the reference's --use_8bit_adam = bitsandbytes.optim.AdamW8bit,
// diffusion/train_controlnet_genima.py:224, :1163-1175; Dettmers et al., "8-bit Optimizers via Block-wise Quantization").
// Both moments are stored as one code byte per element plus one f32 absmax per quantisation block of <= 256 consecutive elements:
// value = map[code] * absmax, first moment through the signed dynamic map, second through the unsigned one.  The maps are built on
// the host (genima_amd/optim8.py) and staged in LDS; nothing here knows their values, only that they are sorted ascending.
//
// One WAVE per quantisation block (64 lanes x 4 elements), walking a block table (element offset, code offset, length) so that no
// block crosses a parameter boundary.  Per block: dequantise m, v -> the fp32 AdamW update of adamw_kernel (backward.hip: decoupled
// weight decay, bias correction, unscale x clip coefficient from the device scalar, skip on a non-finite gradient, zero_grad, f16
// working copy in the same pass) -> new absmax by a DPP wave reduction (no barrier, no LDS round trip) -> re-quantise to the
// NEAREST code; a value exactly halfway between two codes takes the LOWER index.  A skipped step leaves codes and absmax untouched.
// This file is compiled with -ffp-contract=off (build.py): no fma fusion, IEEE divide / sqrt, so the same operation sequence in f32 on
// any IEEE machine gives the same bits, which is what tests/test_adamw8_gpu.py holds the codes to.
// HBM traffic per element: grad r + w (8), master r + w (8), two codes r + w (4), f16 copy w (2) = 22 bytes (+ 16-byte table row and
// 16 bytes of absmax per block: 0.125 per element); the fp32 pass moves 38.
#include "common.h"

namespace {

struct Adam8Hyper {
  float lr, b1, b2, eps, wd, bc1, bc2, gscale;
};

// index of the entry of the ascending 256-entry `map` nearest to x: 8 halving steps to the last entry <= x, then one neighbour compare
__device__ __forceinline__ uint32_t nearest_code(const float* map, float x) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t s = 128; s >= 1; s >>= 1)
    if (map[lo + s] <= x) lo += s;  // lo + s <= 255 throughout
  const uint32_t hi = lo < 255u ? lo + 1u : 255u;
  return (map[hi] - x) < (x - map[lo]) ? hi : lo;
}

__global__ __launch_bounds__(256) void adamw8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ mc, uint8_t* __restrict__ vc,
                                                     float* __restrict__ mabs, float* __restrict__ vabs, const long long* __restrict__ table,
                                                     int n_blocks, long n, long n_codes, const float* __restrict__ map_s,
                                                     const float* __restrict__ map_u, Adam8Hyper h, const float* __restrict__ clip,
                                                     f16* __restrict__ half_out, int zero_grad) {
  __shared__ float sm[256], su[256];
  sm[threadIdx.x] = map_s[threadIdx.x];
  su[threadIdx.x] = map_u[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, e = lane * 4;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int nwaves = gridDim.x * 4;
  const bool skip = clip && clip[2] != 0.0f;  // non-finite gradients: the step is skipped (GradScaler.step), the gradient still cleared
  const float gs = h.gscale * (clip ? clip[0] : 1.0f);
  const float decay = 1.0f - h.lr * h.wd, omb1 = 1.0f - h.b1, omb2 = 1.0f - h.b2, rbc2 = sqrtf(h.bc2), slr = h.lr / h.bc1;
  for (int b = wave; b < n_blocks; b += nwaves) {  // wave-uniform: every lane of the wave stays in the loop (the reductions need all 64)
    const long off = table[2 * b], w1 = table[2 * b + 1];
    const long coff = w1 >> 9;
    const int len = (int)(w1 & 511);
    if (len < 1 || len > 256 || off < 0 || (off & 3) || off + len > n || coff < 0 || coff + len > n_codes) continue;  // a bad row touches nothing
    const bool full = e + 4 <= len;                        // this lane's four elements all lie inside the block
    const bool packed = full && ((coff & 3) == 0);         // ... and its four codes are one aligned dword
    float* gp = g + off + e;
    float gv[4] = {0.f, 0.f, 0.f, 0.f};
    if (full) {
      const float4 t = *reinterpret_cast<const float4*>(gp);
      gv[0] = t.x; gv[1] = t.y; gv[2] = t.z; gv[3] = t.w;
      if (zero_grad) *reinterpret_cast<float4*>(gp) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < len) {
          gv[j] = gp[j];
          if (zero_grad) gp[j] = 0.0f;
        }
    }
    if (skip) continue;
    float* pp = p + off + e;
    uint8_t* mp = mc + coff + e;
    uint8_t* vp = vc + coff + e;
    float pv[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t cm = 0, cv = 0;
    if (full) {
      const float4 t = *reinterpret_cast<const float4*>(pp);
      pv[0] = t.x; pv[1] = t.y; pv[2] = t.z; pv[3] = t.w;
    }
    if (packed) {
      cm = *reinterpret_cast<const uint32_t*>(mp);
      cv = *reinterpret_cast<const uint32_t*>(vp);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < len) {
          if (!full) pv[j] = pp[j];
          cm |= (uint32_t)mp[j] << (8 * j);
          cv |= (uint32_t)vp[j] << (8 * j);
        }
    }
    const float am0 = mabs[b], av0 = vabs[b];
    float mi[4], vi[4], pn[4];
    float am = 0.0f, av = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e + j < len;
      const float m0 = in ? sm[(cm >> (8 * j)) & 255u] * am0 : 0.0f;
      const float v0 = in ? su[(cv >> (8 * j)) & 255u] * av0 : 0.0f;
      const float gi = gv[j] * gs;
      mi[j] = h.b1 * m0 + omb1 * gi;
      vi[j] = h.b2 * v0 + omb2 * gi * gi;
      const float denom = sqrtf(vi[j]) / rbc2 + h.eps;
      pn[j] = pv[j] * decay - slr * (mi[j] / denom);
      am = fmaxf(am, fabsf(mi[j]));
      av = fmaxf(av, vi[j]);
    }
    am = wave_max(am);
    av = wave_max(av);
    const float rm = am > 0.0f ? 1.0f / am : 0.0f, rv = av > 0.0f ? 1.0f / av : 0.0f;
    uint32_t qm = 0, qv = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qm |= nearest_code(sm, mi[j] * rm) << (8 * j);
      qv |= nearest_code(su, vi[j] * rv) << (8 * j);
    }
    if (full) {
      *reinterpret_cast<float4*>(pp) = make_float4(pn[0], pn[1], pn[2], pn[3]);
      if (half_out) {
        f16x4 hv = {(f16)pn[0], (f16)pn[1], (f16)pn[2], (f16)pn[3]};
        *reinterpret_cast<f16x4*>(half_out + off + e) = hv;
      }
    }
    if (packed) {
      *reinterpret_cast<uint32_t*>(mp) = qm;
      *reinterpret_cast<uint32_t*>(vp) = qv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < len) {
          if (!full) {
            pp[j] = pn[j];
            if (half_out) half_out[off + e + j] = (f16)pn[j];
          }
          mp[j] = (uint8_t)(qm >> (8 * j));
          vp[j] = (uint8_t)(qv >> (8 * j));
        }
    }
    if (lane == 0) {
      mabs[b] = am;
      vabs[b] = av;
    }
  }
}

}  // namespace

int32_t gn_adamw8_flat(gn_ctx* ctx, float* param, float* grad, int64_t n, void* m_codes, void* v_codes, int64_t n_codes, float* m_absmax,
                       float* v_absmax, const int64_t* block_table, int32_t n_blocks, const float* map_signed, const float* map_unsigned, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* clip_dev, float grad_scale, void* half_out,
                       int32_t zero_grad) {
  GN_REQUIRE(ctx && param && grad && m_codes && v_codes && m_absmax && v_absmax && block_table && map_signed && map_unsigned && n > 0 && n_codes > 0 &&
                 n_blocks > 0 && step >= 1,
             "gn_adamw8_flat: bad arguments");
  GN_REQUIRE((((uintptr_t)param | (uintptr_t)grad) & 15) == 0 && (((uintptr_t)half_out) & 7) == 0 && (((uintptr_t)m_codes | (uintptr_t)v_codes) & 3) == 0 &&
                 (((uintptr_t)block_table) & 15) == 0,
             "gn_adamw8_flat: param / grad must be 16-byte aligned, half_out 8-byte, the code buffers 4-byte, the block table 16-byte");
  Adam8Hyper h;
  h.lr = lr; h.b1 = beta1; h.b2 = beta2; h.eps = eps; h.wd = weight_decay; h.gscale = grad_scale;
  h.bc1 = (float)(1.0 - pow((double)beta1, (double)step));  // f64, rounded once: the step size of gn_adamw_flat (backward.hip)
  h.bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  const int want = (n_blocks + 3) / 4;
  const int grid = want < 2048 ? want : 2048;  // persistent: 8 workgroups of 4 waves per CU walk the table
  hipLaunchKernelGGL(adamw8_kernel, dim3(grid), dim3(256), 0, ctx->stream, param, grad, (uint8_t*)m_codes, (uint8_t*)v_codes, m_absmax, v_absmax,
                     (const long long*)block_table, n_blocks, (long)n, (long)n_codes, map_signed, map_unsigned, h, clip_dev, (f16*)half_out, zero_grad);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
