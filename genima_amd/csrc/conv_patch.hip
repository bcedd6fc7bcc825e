// 3x3 convolution from an LDS-resident input patch in 64-channel groups, 128 x 160 output tiles (gfx950): conv_gn.hip's scheme for the
// UNet / ControlNet ResNet convs at 320 / 640 output channels, with their time shift and their concatenated (two-source) input.
//
//   out[b, y, x, :] = bias + shift[b, :] + sum_{tap, c} act(X[b, y + dy - 1, x + dx - 1, c] * scale[b, c] + shift_gn[b, c]) * w[:, tap * Cin + c]  (+ residual)
//   X = x  or the virtual concat [x | x2] along channels (C1 + C2 = Cin);  scsh == NULL: plain conv
//
// diffusers ResnetBlock2D: norm1 -> SiLU -> conv1 (+ time_emb_proj shift) and norm2 -> SiLU -> conv2 (+ residual).  The implicit GEMM
// (gemm.hip, tile <128, 160, 4, 1>) stages every input pixel nine times: per 64-wide K tile a workgroup pulls 16 KB of A and 20 KB of W from L2
// into LDS.  Here
//   * a workgroup owns an 8 x 16 tile of output pixels (128 GEMM rows) x 160 output channels: four waves as 4 x 1, one 32 x 160 wave tile each;
//   * the 10 x 18 input patch of a 64-channel group (180 pixels x 128 bytes = 23 KB: 23 LDS-DMA instructions of 8 pixels) is staged ONCE and
//     all nine taps read their A fragments from it -- A is 2.5 KB per K tile instead of 16 KB.  A group's patch comes from x or from x2 by a
//     wave-uniform choice; the eight 16-byte chunks of a pixel are XOR-swizzled by (patch column >> 1): pixels are 128 bytes apart, so the
//     column's low bit already picks the half of the 64 banks and 16 neighbouring columns land on 16 different 16-byte bank slots;
//   * GroupNorm-apply + SiLU run on the patch in LDS, once per staged element, in f32, rounded to f16 where gn_apply_kernel (norm.hip) rounds;
//     pixels outside the image stay zero (the conv pads the NORMALISED tensor), and a halo row outside the sample is outside the image;
//   * only the weights stream: [160 x 64] K tiles (20 KB) of the packed [Cout][9 * Cin] weight through a 2-stage LDS-DMA ring, K order
//     (group, tap, channel) -- gn_gemm's weight, no new packing; a different summation order than gn_gemm's (tap, channel).
// LDS (160 KB per CU): 23 KB patch + 2 x 20 KB weights = 63 KB -> two workgroups of four waves per CU; one's patch load + normalisation runs
// under the other's nine K tiles (180 MFMAs per wave and group).  64 x 64 at B = 8: 512 workgroups = two per CU in one round; 32 x 32: 256
// workgroups, one per CU -- nothing covers its patch loads there.  A second patch buffer (86 KB, one workgroup per CU, the next group's patch
// DMA'd beside the weight tiles and normalised between the MFMA groups) was raced at both levels and lost to this form at every shape
// (DESIGN.md section 3.7), so it is not kept.
// Epilogue: bias, per-sample time shift, residual -- gn_gemm's order, all in f32, one rounding -- 16-byte row stores.
// Every workgroup is independent: no atomics, no hand-off between workgroups, no persistent grid.  No scratch (checked in the .s: 0 spills).
#include "gemm_common.h"

namespace {

constexpr int CP_TH = 8, CP_TW = 16;                      // output tile (pixels)
constexpr int CP_PW = CP_TW + 2;                          // patch row pitch (halo included)
constexpr int CP_NPIX = (CP_TH + 2) * CP_PW;              // 180
constexpr int CP_CG = 64;                                 // channels per patch (one channel group): 128-byte pixels
constexpr int CP_NDMA = (CP_NPIX + 7) / 8;                // 23 DMA instructions of 8 pixels (the last one half used)
constexpr int CP_PATCH = CP_NDMA * 1024;                  // 23552 bytes per patch buffer
constexpr int CP_BN = 160;                                // output channels per workgroup
constexpr int CP_WT = CP_BN * 128;                        // one weight K tile [160 rows x 64 k]: 20480 bytes
static_assert(2 * (CP_PATCH + 2 * CP_WT) <= 160 * 1024, "two workgroups per CU");

typedef unsigned u32x4p __attribute__((ext_vector_type(4)));

struct CpParams {
  const f16* x;
  const f16* x2;       // second source of the virtual concat or nullptr
  const float* scsh;   // [B][Cin][2] (scale, shift) by concatenated channel, or nullptr: plain conv
  const f16* w;        // [Cout][9 * Cin]
  const f16* bias;     // [Cout] or nullptr
  const f16* shift;    // [B, ldshift] or nullptr
  const f16* res;      // [B * H * W, ldr] or nullptr
  f16* out;            // [B * H * W, ldo]
  long ldr, ldo, ldshift;
  int B, H, W, C1, C2, Cin, Cout, silu;
  int tiles_x, tiles_y, tiles_n;
  unsigned x_bytes, x2_bytes, w_bytes;
};

__device__ __forceinline__ void conv3x3_patch_body(const CpParams& p, unsigned char* smem) {
  constexpr int TN = CP_BN / 32;  // 32 x 32 MFMA tiles across the wave's 160 channels
  constexpr int W_OFF = CP_PATCH;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;

  // XCD-aware block -> tile map as conv_gn.hip: the N tiles of one patch side by side, then the next patch along the image row
  const int bid = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tile_n = bid % p.tiles_n;
  int t = bid / p.tiles_n;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int b = t / p.tiles_y;
  const int y0 = ty * CP_TH, x0 = tx * CP_TW, n0 = tile_n * CP_BN;

  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x2 ? p.x2 : p.x), 0, (int)p.x2_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);

  // ---- weight loader (gemm_dma_kernel's: 8 rows x 128 bytes per instruction, the XOR swizzle of lds_swz<128> on the source side);
  // 20 instructions per K tile, five per wave
  const int lr = lane >> 3;
  const int wchunk = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);
  const long ldw = 9l * p.Cin;
  unsigned woff[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) woff[i] = (unsigned)(((long)(n0 + 8 * (wave + 4 * i) + lr) * ldw + wchunk * 8) * 2);
  auto dma_w = [&](int stage, int kelem) __attribute__((always_inline)) {
    unsigned char* Ws = smem + W_OFF + stage * CP_WT;
#pragma unroll
    for (int i = 0; i < TN; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Ws + (wave + 4 * i) * 1024), 16, woff[i] + (unsigned)kelem * 2u, 0, 0, 0);
  };

  // ---- patch loader: instruction tt stages pixels 8 tt .. 8 tt + 7; lane q lands at physical chunk q & 7 of pixel 8 tt + (q >> 3) and
  // therefore fetches logical chunk (q & 7) ^ key(patch column).  Pixels outside the image (and past the patch's end) land as zeros
  auto dma_patch = [&](unsigned char* P, int g, int tt) __attribute__((always_inline)) {
    const int idx = 8 * tt + (lane >> 3);
    const int pr = idx / CP_PW, pc = idx - pr * CP_PW;
    const int gy = y0 - 1 + pr, gx = x0 - 1 + pc;
    const bool ok = idx < CP_NPIX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    const int lc = (lane & 7) ^ ((pc >> 1) & 7);
    const long pix = ((long)b * p.H + gy) * p.W + gx;
    const int c0 = g * CP_CG;
    if (c0 < p.C1) {  // (wave-uniform)
      unsigned voff = ok ? (unsigned)((pix * p.C1 + c0 + lc * 8) * 2) : kOOB;
      GN_PIN(voff);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(P + tt * 1024), 16, voff, 0, 0, 0);
    } else {
      unsigned voff = ok ? (unsigned)((pix * p.C2 + (c0 - p.C1) + lc * 8) * 2) : kOOB;
      GN_PIN(voff);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x2, (lds_ptr_t)(P + tt * 1024), 16, voff, 0, 0, 0);
    }
  };

  // ---- GroupNorm-apply (+ SiLU) on pixels [p0, p1) of a patch, in place.  A thread keeps ONE logical 16-byte chunk (8 channels: their
  // scale / shift live in registers) and walks the pixels 32 apart; the 8 threads of a pixel cover its 128 bytes
  float gsc[8], gsh[8];
  auto load_scsh = [&](int g) __attribute__((always_inline)) {
    const f32x4* sp = reinterpret_cast<const f32x4*>(p.scsh + ((long)b * p.Cin + g * CP_CG + (tid & 7) * 8) * 2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 s4 = sp[e];
      gsc[2 * e] = s4[0]; gsh[2 * e] = s4[1]; gsc[2 * e + 1] = s4[2]; gsh[2 * e + 1] = s4[3];
    }
  };
  auto norm_range = [&](unsigned char* P, int p0, int p1) __attribute__((always_inline)) {
    const int lcn = tid & 7;
    for (int idx = p0 + (tid >> 3); idx < p1; idx += 32) {
      const int pr = idx / CP_PW, pcx = idx - pr * CP_PW;
      const int gy = y0 - 1 + pr, gx = x0 - 1 + pcx;
      if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
        unsigned char* q = P + idx * 128 + ((lcn ^ ((pcx >> 1) & 7)) << 4);
        const f16x8 v = *reinterpret_cast<const f16x8*>(q);
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float yv = (float)v[e] * gsc[e] + gsh[e];
          if (p.silu) yv = yv * __builtin_amdgcn_rcpf(1.0f + __expf(-yv));  // SiLU on v_rcp_f32, as conv_gn.hip
          o[e] = (f16)yv;
        }
        *reinterpret_cast<f16x8*>(q) = o;
      }
    }
  };

  // ---- A fragment addressing: GEMM row m = 16 py + px of the tile; its tap (dy, dx) pixel sits at patch index (py + dy) * 18 + px + dx
  const int m = wave * 32 + l31;
  const int pidx0 = (m >> 4) * CP_PW + (m & 15);

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  // residual row of this lane's pixel, requested ahead of the K loop (raw 16-byte pieces; the lane swap waits for the data: epilogue)
  const long orow = ((long)b * p.H + y0 + (m >> 4)) * p.W + x0 + (m & 15);
  u32x4p rraw[TN][2];
  if (p.res) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) rraw[j][h] = *reinterpret_cast<const u32x4p*>(p.res + orow * p.ldr + n0 + j * 32 + 16 * h + 8 * hi);
  }

  const int ngroups = p.Cin / CP_CG;
  // ---- group 0: patch + first weight tile, normalisation
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (wave + 4 * i < CP_NDMA) dma_patch(smem, 0, wave + 4 * i);
  dma_w(0, 0);
  if (p.scsh) load_scsh(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (p.scsh) {
    norm_range(smem, 0, CP_NPIX);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }

  int T = 0;  // K tile counter: weight ring stage = T & 1
  for (int g = 0; g < ngroups; ++g) {
    const bool more = g + 1 < ngroups;
    for (int tap = 0; tap < 9; ++tap, ++T) {
      // the next K tile's weights land under this tile's MFMAs (the next group's tap 0 behind tap 8)
      if (tap < 8) dma_w((T + 1) & 1, (tap + 1) * p.Cin + g * CP_CG);
      else if (more) dma_w((T + 1) & 1, (g + 1) * CP_CG);
      const int dy = tap / 3, dx = tap - dy * 3;
      const int key = (((l31 & 15) + dx) >> 1) & 7;  // swizzle key of the tapped pixel = its patch column >> 1
      const unsigned char* arow = smem + (pidx0 + dy * CP_PW + dx) * 128;
      const unsigned char* Ws = smem + W_OFF + (T & 1) * CP_WT;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int cl = kk * 2 + hi;  // logical 16-byte chunk of the pixel's 64 channels
        const f16x8 fa = *reinterpret_cast<const f16x8*>(arow + ((cl ^ key) << 4));
        f16x8 fw[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) fw[j] = *reinterpret_cast<const f16x8*>(Ws + lds_swz<128>(j * 32 + l31, cl));
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[j], fa, acc[j], 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) {  // every wave is done with this group's patch (the barrier above): the next one over it
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (wave + 4 * i < CP_NDMA) dma_patch(smem, g + 1, wave + 4 * i);
      if (p.scsh) load_scsh(g + 1);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (p.scsh) {
        norm_range(smem, 0, CP_NPIX);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue: + bias + time shift (+ residual) -> f16, 16-byte row stores (lanes l / l + 32 trade halves, as gemm_common.h's wide path)
  f16* orw = p.out + orow * p.ldo;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + j * 32;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = acc[j][e];
    if (p.bias) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x4 bb = *reinterpret_cast<const f16x4*>(p.bias + nb + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * g + e] += (float)bb[e];
      }
    }
    if (p.shift) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f16x4 ss = *reinterpret_cast<const f16x4*>(p.shift + (long)b * p.ldshift + nb + 8 * g + 4 * hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * g + e] += (float)ss[e];
      }
    }
    if (p.res) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4p r = rraw[j][h];
        const auto r0 = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false);
        const uint2 lo = make_uint2(r0[0], r1[0]), hi2 = make_uint2(r0[1], r1[1]);
        const f16x4 ga = *reinterpret_cast<const f16x4*>(&lo), gb = *reinterpret_cast<const f16x4*>(&hi2);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[8 * h + e] += (float)ga[e]; v[8 * h + 4 + e] += (float)gb[e]; }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      f16x4 ha, hb;
#pragma unroll
      for (int e = 0; e < 4; ++e) { ha[e] = (f16)v[4 * g + e]; hb[e] = (f16)v[4 * g + 4 + e]; }
      const uint2 ua = *reinterpret_cast<const uint2*>(&ha), ub = *reinterpret_cast<const uint2*>(&hb);
      const auto r0 = __builtin_amdgcn_permlane32_swap(ua.x, ub.x, false, false);
      const auto r1 = __builtin_amdgcn_permlane32_swap(ua.y, ub.y, false, false);
      *reinterpret_cast<u32x4p*>(orw + nb + 8 * g + 8 * hi) = u32x4p{r0[0], r1[0], r0[1], r1[1]};
    }
  }
}

// (the kernel's ONE LDS object: see tblock.hip on hipcc's vmcnt drains)
__global__ __launch_bounds__(256, 2) void conv3x3_patch_kernel(const CpParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CP_PATCH + 2 * CP_WT];
  conv3x3_patch_body(p, smem);
}

}  // namespace

extern "C" int32_t gn_conv3x3_patch_supported(int32_t B, int32_t H, int32_t W, int32_t C1, int32_t C2, int32_t Cout) {
  return B > 0 && H > 0 && W > 0 && H % CP_TH == 0 && W % CP_TW == 0 && C1 > 0 && C2 >= 0 && (C1 + C2) % CP_CG == 0 && (C2 == 0 || C1 % CP_CG == 0) &&
                 Cout > 0 && Cout % CP_BN == 0 && (int64_t)B * H * W * C1 * 2 < 0xFFFFFF00ll && (int64_t)B * H * W * C2 * 2 < 0xFFFFFF00ll &&
                 (int64_t)Cout * 9 * (C1 + C2) * 2 < 0xFFFFFF00ll
             ? 1 : 0;
}

extern "C" int32_t gn_conv3x3_patch(gn_ctx* ctx, const gn_conv3x3_patch_desc* d) {
  GN_REQUIRE(ctx && d && d->x && d->w && d->out, "gn_conv3x3_patch: null ctx / x / w / out");
  GN_REQUIRE((d->C2 == 0) == (d->x2 == nullptr), "gn_conv3x3_patch: x2 and C2 must be given together");
  GN_REQUIRE(gn_conv3x3_patch_supported(d->B, d->H, d->W, d->C1, d->C2, d->Cout),
             "gn_conv3x3_patch: needs H %% 8 == 0, W %% 16 == 0, (C1 + C2) %% 64 == 0, C1 %% 64 == 0 with x2, Cout %% 160 == 0 (got %dx%d, %d + %d -> %d); use gn_gemm otherwise",
             d->H, d->W, d->C1, d->C2, d->Cout);
  GN_REQUIRE(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->x2 & 15) == 0 && ((uintptr_t)d->w & 15) == 0 && ((uintptr_t)d->out & 15) == 0 && d->ldo % 8 == 0 && d->ldo >= d->Cout,
             "gn_conv3x3_patch: x / x2 / w / out must be 16-byte aligned, ldo a multiple of 8 and >= Cout");
  if (d->residual) GN_REQUIRE(((uintptr_t)d->residual & 15) == 0 && d->ldr % 8 == 0 && d->ldr >= d->Cout, "gn_conv3x3_patch: residual alignment / stride");
  if (d->shift) GN_REQUIRE(((uintptr_t)d->shift & 7) == 0 && d->ldshift % 4 == 0 && d->ldshift >= d->Cout, "gn_conv3x3_patch: shift alignment / stride");
  if (d->bias) GN_REQUIRE(((uintptr_t)d->bias & 7) == 0, "gn_conv3x3_patch: bias must be 8-byte aligned");
  if (d->scsh) GN_REQUIRE(((uintptr_t)d->scsh & 15) == 0, "gn_conv3x3_patch: scsh must be 16-byte aligned");
  GN_REQUIRE(d->act == GN_ACT_NONE || d->act == GN_ACT_SILU, "gn_conv3x3_patch: act (applied after the affine, before the conv) must be NONE or SILU");
  CpParams p;
  p.x = (const f16*)d->x; p.x2 = (const f16*)d->x2; p.scsh = (const float*)d->scsh; p.w = (const f16*)d->w; p.bias = (const f16*)d->bias;
  p.shift = (const f16*)d->shift; p.res = (const f16*)d->residual; p.out = (f16*)d->out;
  p.ldr = d->ldr; p.ldo = d->ldo; p.ldshift = d->ldshift;
  p.B = d->B; p.H = d->H; p.W = d->W; p.C1 = d->C1; p.C2 = d->C2; p.Cin = d->C1 + d->C2; p.Cout = d->Cout; p.silu = d->act == GN_ACT_SILU ? 1 : 0;
  p.tiles_x = d->W / CP_TW; p.tiles_y = d->H / CP_TH; p.tiles_n = d->Cout / CP_BN;
  p.x_bytes = (unsigned)((uint64_t)d->B * d->H * d->W * d->C1 * 2); p.x2_bytes = (unsigned)((uint64_t)d->B * d->H * d->W * d->C2 * 2);
  p.w_bytes = (unsigned)((uint64_t)d->Cout * 9 * p.Cin * 2);
  const long nblocks = (long)d->B * p.tiles_x * p.tiles_y * p.tiles_n;
  hipLaunchKernelGGL(conv3x3_patch_kernel, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, p);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
