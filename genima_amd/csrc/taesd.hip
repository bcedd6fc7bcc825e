// diffusers AutoencoderTinyBlock at 64 channels as ONE launch (gfx950):
//
//   out = relu(conv3(relu(conv2(relu(conv1(x))))) + x)      3x3 convs, stride 1, padding 1, NHWC f16, f32 accumulation
//
// Every block of the TAESD / TAESDXL encoder has this form (identity skip).  As three gn_gemm conv launches the 512^2 stage moves each
// 64-channel activation through HBM five times per block (x read twice, two intermediates written and read back) and the implicit-GEMM
// tiles, built for N >= 128, run at N = 64.  Here:
//   * a workgroup (8 waves) owns a 16 x 16 tile of output pixels x all 64 channels;
//   * its 22 x 22 input patch (3-pixel halo) is DMA'd into LDS ONCE (`buffer_load ... lds`; pixels outside the image land as zeros);
//   * conv1 computes the 20 x 20 ring-2 region into LDS region A, conv2 the 18 x 18 ring-1 region from A over the input patch (the
//     patch is dead by then), conv3 the 16 x 16 tile from it; the identity skip re-reads x from global (L2: the patch was just read).
//     Each intermediate is rounded to f16 and ReLU'd exactly as the unfused route stores it, and is ZERO at pixels outside the image:
//     every conv zero-pads its own input, so a halo pixel outside the image is padding at every stage, not the conv of padding;
//   * only the weights stream: one tap of one conv ([64 out][64 in], 8 KB) per step, 27 steps, register-staged into a 2-slot LDS ring
//     (221 KB per tile, served from L2).
// LDS: patch 61 KB (60.5 KB + the last DMA's 8-pixel overhang) + region A 50 KB + weight ring 16 KB = 127 KB: one workgroup per CU,
// 8 waves (2 per SIMD).  Recompute: (400 + 324 + 256) / (3 x 256) = 1.28x the tile's MACs.
// GEMM form of each conv: rows = 32-pixel runs of the region in raster order (the last run of a region is clamped, its rows are not
// stored), columns = output channels; MFMA 32x32x16 f16 with the weights as the A operand, so a lane ends with 16 channels of ONE pixel.
// Wave w takes output-channel half w & 1 and runs (w >> 1) + 4 j: conv1 13 runs (4 rounds), conv2 11 (3), conv3 8 (2).
// LDS layout of a region (pitch = its width, 128 B per pixel): the 16-byte channel chunk c of the pixel at linear index a, region row r,
// sits in slot c ^ (((a >> 1) - r) & 7).  Checked exhaustively for all nine taps of all three convs: the four 16-lane groups of every
// ds_read_b128 fragment read hit 16 distinct slots of the 256-byte bank row (the plain (a >> 1) key is 2-way at the region's row breaks); the conflicts measured below come from elsewhere (stores: DESIGN.md 3.5).
// Measured (MI355X, tools/bench_taesd.py, B = 8): 1349 us at 512^2 against 1033 us for the three gn_gemm launches, 327 vs 247 us at 256^2 --
// LDS-bound (1.6 LDS instructions per MFMA, SQ_LDS_BANK_CONFLICT 9.5 % of LDS cycles), so the graphs route is opt-in (GN_TINY_BLOCK=1).
#include "gemm_common.h"

namespace {

constexpr int TB_T = 16;                    // output tile (pixels per side)
constexpr int TB_PX = TB_T + 6;             // 22: input patch
constexpr int TB_PA = TB_T + 4;             // 20: conv1's region (A)
constexpr int TB_PB = TB_T + 2;             // 18: conv2's region (B, over the patch)
constexpr int TB_A_OFF = 61 * 1024;         // the patch's 61 DMA instructions of 8 pixels (484 pixels + 4 overhang) end here
constexpr int TB_W_OFF = TB_A_OFF + TB_PA * TB_PA * 128;
constexpr int TB_LDS = TB_W_OFF + 2 * 64 * 128;
static_assert(TB_PX * TB_PX * 128 <= TB_A_OFF && (TB_PX * TB_PX + 7) / 8 * 1024 <= TB_A_OFF, "patch overlaps region A");
static_assert(TB_PB * TB_PB * 128 <= TB_A_OFF, "conv2's region must fit in the patch's place");
static_assert(TB_LDS <= 160 * 1024, "one workgroup per CU");

struct TbParams {
  const f16* x;
  const f16* w[3];     // packed [64][9 * 64], K order (tap, channel)
  const f16* bias[3];  // [64]
  f16* out;
  int B, H, W, tiles_x, tiles_y;
  unsigned x_bytes;
};

// byte offset of 16-byte chunk `c` of the pixel at linear index `a`, region row `r` (swizzle: header)
__device__ __forceinline__ int tb_off(int a, int r, int c) { return a * 128 + ((c ^ (((a >> 1) - r) & 7)) << 4); }

__device__ __forceinline__ void tb_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// one weight step: tap `tap` of conv `k` ([64 rows][64 channels], 16 bytes per thread)
__device__ __forceinline__ f16x8 tb_load_w(const TbParams& p, int step, int tid) {
  const int k = step / 9, tap = step - 9 * k;
  return *reinterpret_cast<const f16x8*>(p.w[k] + (tid >> 3) * (9 * 64) + tap * 64 + (tid & 7) * 8);
}
__device__ __forceinline__ void tb_store_w(unsigned char* smem, int step, int tid, f16x8 v) {
  *reinterpret_cast<f16x8*>(smem + TB_W_OFF + (step & 1) * 8192 + lds_swz<128>(tid >> 3, tid & 7)) = v;
}

// acc[j] = conv over the 9 taps of conv `k` (steps 9k .. 9k + 8) for the wave's runs (w >> 1) + 4 j of an WO-wide, NPIX-pixel output
// region whose input region (pitch WO + 2) sits at `src`.  Each step ends with a barrier; the next step's weights land under the MFMAs.
template <int WO, int NPIX, int JM>
__device__ __forceinline__ void tb_conv(const TbParams& p, unsigned char* smem, const unsigned char* src, int k, f32x16 (&acc)[JM]) {
  constexpr int WI = WO + 2, NT = (NPIX + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5, nh = wave & 1;
  int base[JM], prow[JM];
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int m = min(((wave >> 1) + 4 * j) * 32 + l31, NPIX - 1);
    prow[j] = m / WO;
    base[j] = prow[j] * WI + (m - prow[j] * WO);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
  }
  for (int tap = 0; tap < 9; ++tap) {
    const int step = 9 * k + tap;
    f16x8 wn;
    if (step + 1 < 27) wn = tb_load_w(p, step + 1, tid);
    const int dy = tap / 3, dx = tap - 3 * dy;
    const unsigned char* Ws = smem + TB_W_OFF + (step & 1) * 8192;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + hi;
      const f16x8 fw = *reinterpret_cast<const f16x8*>(Ws + lds_swz<128>(nh * 32 + l31, c));
#pragma unroll
      for (int j = 0; j < JM; ++j) {
        if ((wave >> 1) + 4 * j < NT) {
          const f16x8 fa = *reinterpret_cast<const f16x8*>(src + tb_off(base[j] + dy * WI + dx, prow[j] + dy, c));
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw, fa, acc[j], 0, 0, 0);
        }
      }
    }
    if (step + 1 < 27) tb_store_w(smem, step + 1, tid, wn);
    tb_sync();
  }
}

// relu(acc + bias) -> f16 into an LDS region (WO wide, NPIX pixels, origin (oy, ox) in the image); zero outside the image
template <int WO, int NPIX, int JM>
__device__ __forceinline__ void tb_store_region(const TbParams& p, unsigned char* dst, const f16* bias, int oy, int ox, const f32x16 (&acc)[JM]) {
  constexpr int NT = (NPIX + 31) / 32;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5, nh = wave & 1;
  f16x4 bb[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bb[g] = *reinterpret_cast<const f16x4*>(bias + nh * 32 + 8 * g + 4 * hi);
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int m = ((wave >> 1) + 4 * j) * 32 + l31;
    if ((wave >> 1) + 4 * j < NT && m < NPIX) {
      const int py = m / WO, px = m - py * WO;
      const bool in = (unsigned)(oy + py) < (unsigned)p.H && (unsigned)(ox + px) < (unsigned)p.W;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = in ? (f16)fmaxf(acc[j][4 * g + e] + (float)bb[g][e], 0.0f) : (f16)0.0f;
        *reinterpret_cast<f16x4*>(dst + tb_off(m, py, nh * 4 + g) + 8 * hi) = o;
      }
    }
  }
}

__global__ __launch_bounds__(512, 1) void tiny_block_kernel(const TbParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[TB_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // XCD-aware block -> tile map (xcd_tile_id): an XCD walks a contiguous run of tiles, so neighbours share halos in one L2
  const int bid = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tx = bid % p.tiles_x;
  const int t = bid / p.tiles_x;
  const int ty = t % p.tiles_y;
  const int b = t / p.tiles_y;
  const int y0 = ty * TB_T, x0 = tx * TB_T;

  // ---- the 22 x 22 patch: 61 DMA instructions of 8 pixels x 128 bytes; lane q lands in slot q & 7 of pixel 8 t + (q >> 3) and so
  // fetches that pixel's logical chunk (q & 7) ^ key.  Pixels outside the image (and the 4 overhang pixels) read as zeros.
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int tt = wave + 8 * i;
    if (tt < 61) {
      const int a = 8 * tt + (lane >> 3);
      const int r = a / TB_PX, c = a - r * TB_PX;
      const int gy = y0 - 3 + r, gx = x0 - 3 + c;
      const bool ok = a < TB_PX * TB_PX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
      const int lc = (lane & 7) ^ (((a >> 1) - r) & 7);
      unsigned voff = ok ? (unsigned)(((((long)b * p.H + gy) * p.W + gx) * 64 + lc * 8) * 2) : kOOB;
      GN_PIN(voff);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(smem + tt * 1024), 16, voff, 0, 0, 0);
    }
  }
  tb_store_w(smem, 0, tid, tb_load_w(p, 0, tid));
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  {  // conv1: patch -> region A (20 x 20, origin (y0 - 2, x0 - 2))
    f32x16 acc[4];
    tb_conv<TB_PA, TB_PA * TB_PA, 4>(p, smem, smem, 0, acc);
    tb_store_region<TB_PA, TB_PA * TB_PA, 4>(p, smem + TB_A_OFF, p.bias[0], y0 - 2, x0 - 2, acc);
    tb_sync();
  }
  {  // conv2: region A -> region B (18 x 18, origin (y0 - 1, x0 - 1)) over the patch
    f32x16 acc[3];
    tb_conv<TB_PB, TB_PB * TB_PB, 3>(p, smem, smem + TB_A_OFF, 1, acc);
    tb_store_region<TB_PB, TB_PB * TB_PB, 3>(p, smem, p.bias[1], y0 - 1, x0 - 1, acc);
    tb_sync();
  }

  // conv3: region B -> the tile, + bias + x, relu, to global.  The skip's x rows are requested before the K loop.
  const int l31 = lane & 31, hi = lane >> 5, nh = wave & 1;
  long prow[2];
  bool in[2];
  f16x4 res[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = ((wave >> 1) + 4 * j) * 32 + l31;
    const int gy = y0 + (m >> 4), gx = x0 + (m & 15);
    in[j] = gy < p.H && gx < p.W;
    prow[j] = (((long)b * p.H + gy) * p.W + gx) * 64 + nh * 32 + 4 * hi;
#pragma unroll
    for (int g = 0; g < 4; ++g) res[j][g] = in[j] ? *reinterpret_cast<const f16x4*>(p.x + prow[j] + 8 * g) : f16x4{};
  }
  f32x16 acc[2];
  tb_conv<TB_T, TB_T * TB_T, 2>(p, smem, smem, 2, acc);
  f16x4 bb[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bb[g] = *reinterpret_cast<const f16x4*>(p.bias[2] + nh * 32 + 8 * g + 4 * hi);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (in[j]) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (f16)fmaxf(acc[j][4 * g + e] + (float)bb[g][e] + (float)res[j][g][e], 0.0f);
        *reinterpret_cast<f16x4*>(p.out + prow[j] + 8 * g) = o;
      }
    }
  }
}

}  // namespace

extern "C" int32_t gn_tiny_block_supported(int32_t C, int32_t H, int32_t W) { return C == 64 && H > 0 && W > 0 ? 1 : 0; }

extern "C" int32_t gn_tiny_block(gn_ctx* ctx, const void* x, const void* const w[3], const void* const bias[3], void* out, int32_t B, int32_t H,
                                 int32_t W, int32_t C) {
  GN_REQUIRE(ctx && x && w && bias && out, "gn_tiny_block: null ctx / x / w / bias / out");
  GN_REQUIRE(B > 0 && gn_tiny_block_supported(C, H, W), "gn_tiny_block: needs C == 64 and B, H, W > 0 (got B %d, %dx%d, C %d)", B, H, W, C);
  const uint64_t bytes = (uint64_t)B * H * W * C * 2;
  GN_REQUIRE(bytes < 0xFFFFFF00ull, "gn_tiny_block: x is %llu bytes; the patch loads address it with 32-bit offsets", (unsigned long long)bytes);
  GN_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "gn_tiny_block: x / out must be 16-byte aligned");
  GN_REQUIRE((const char*)out + bytes <= (const char*)x || (const char*)x + bytes <= (const char*)out,
             "gn_tiny_block: out must not overlap x (neighbouring tiles read x's halo)");
  TbParams p;
  for (int k = 0; k < 3; ++k) {
    GN_REQUIRE(w[k] && bias[k], "gn_tiny_block: null weight / bias %d", k);
    GN_REQUIRE(((uintptr_t)w[k] & 15) == 0 && ((uintptr_t)bias[k] & 7) == 0, "gn_tiny_block: weights must be 16-byte, biases 8-byte aligned");
    p.w[k] = (const f16*)w[k];
    p.bias[k] = (const f16*)bias[k];
  }
  p.x = (const f16*)x;
  p.out = (f16*)out;
  p.B = B; p.H = H; p.W = W;
  p.tiles_x = (W + TB_T - 1) / TB_T;
  p.tiles_y = (H + TB_T - 1) / TB_T;
  p.x_bytes = (unsigned)bytes;
  const long nblocks = (long)B * p.tiles_x * p.tiles_y;
  GN_REQUIRE(nblocks < 0x7FFFFFFFl, "gn_tiny_block: too many tiles");
  hipLaunchKernelGGL(tiny_block_kernel, dim3((unsigned)nblocks), dim3(512), 0, ctx->stream, p);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
