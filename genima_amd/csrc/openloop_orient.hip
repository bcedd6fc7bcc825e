// The orientation read-out of the open-loop evaluation (genima_amd/openloop.py OpenLoopEval(orientation=)): the cost of a generated sphere
// window against the TRUE sphere re-drawn at K candidate rotations about its own frame.  include/genima_hip.h (gn_openloop_orientation)
// states the rule.
//
// Grid: x = candidate k, y = sphere slot s, z = scored view (sample * V + view; only the n_valid scored samples are launched): one workgroup
// per (window, candidate), 256 threads.  The first `count` threads bring the view's spheres into eye space with render_common.h's
// sphere_to_lds -- thread s from a private copy of its sphere whose rotation is Rs * R_k, composed in f64 left to right -- and leave them in
// LDS, so a candidate's pixels are shade_pixel's, bit for bit what gn_render_spheres draws from the same table.  The threads then stride over
// the window's at most 256 x 256 pixels as openloop_sphere_kernel does; a pixel's `occupied` byte is loaded first and a clear one casts no
// ray.  A thread sees at most 256 pixels, so its squared-error sums (<= 256 * 195 075) fit 32 bits; they go through the wave sum as a 24-bit
// low part and a high part, the four waves' totals meet in LDS as 64-bit values and thread 0 stores the window's four values with plain
// stores: the workgroup owns its row, so there is no atomic and no zeroing pass.  No thread leaves before the fold.
// Built with -ffp-contract=off, as every file that includes render_common.h.
#include "openloop_common.h"
#include "render_common.h"

namespace {

constexpr int OL_ORI_COLS = 4;
constexpr int OL_ORI_K_MAX = 64;
constexpr int OL_SHIFT_MAX = 127;

struct OriParams {
  const uint8_t* gen;
  const uint8_t* gt;
  const uint8_t* occupied;
  const int32_t* win;
  const float* cams;
  const float* spheres;
  const int32_t* tex_index;
  const int32_t* count;
  const uint8_t* atlas;
  const float* rot;
  const int32_t* shift;
  unsigned long long* out;
  int V, H, W, S, K, T, th, tw, samples, tiled, row0;
};

__global__ __launch_bounds__(OL_THREADS) void openloop_orientation_kernel(const OriParams p) {
  __shared__ SphereLds sph[MAX_SPHERES];
  __shared__ unsigned long long part[OL_THREADS / 64][OL_ORI_COLS];
  const int k = blockIdx.x, s = blockIdx.y;
  const long view = blockIdx.z;
  const int b = (int)(view / p.V), v = (int)(view - (long)b * p.V);
  const float* __restrict__ cam = p.cams + view * CAM_FLOATS;
  int n = p.count[view];
  n = n < 0 ? 0 : (n > p.S ? p.S : n);
  if ((int)threadIdx.x < n) {
    float q[SPHERE_FLOATS];
    const float* __restrict__ sp = p.spheres + (view * p.S + threadIdx.x) * SPHERE_FLOATS;
#pragma unroll
    for (int i = 0; i < SPHERE_FLOATS; ++i) q[i] = sp[i];
    if ((int)threadIdx.x == s) {  // Rs * R_k: f64 products of f32 values, added left to right, rounded once
      const float* __restrict__ R = p.rot + (long)k * 9;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double r0 = (double)sp[i * 4], r1 = (double)sp[i * 4 + 1], r2 = (double)sp[i * 4 + 2];
#pragma unroll
        for (int l = 0; l < 3; ++l) q[i * 4 + l] = (float)((r0 * (double)R[l] + r1 * (double)R[3 + l]) + r2 * (double)R[6 + l]);
      }
    }
    sphere_to_lds(sph[threadIdx.x], cam, q, p.tex_index[view * p.S + threadIdx.x], p.T, p.W, p.H);
  }
  __syncthreads();

  const int W = p.W, H = p.H;
  const int32_t* wp = p.win + (view * p.S + s) * 4;
  // clamped into the image and to OL_WIN_MAX per side, as openloop_sphere_kernel clamps: no address below depends on the table's values being sane
  const int x0 = ol_clamp(wp[0], 0, W), y0 = ol_clamp(wp[1], 0, H);
  const int w = ol_clamp(ol_clamp(wp[2], 0, W) - x0, 0, OL_WIN_MAX), h = ol_clamp(ol_clamp(wp[3], 0, H) - y0, 0, OL_WIN_MAX);
  const uint32_t npix = (uint32_t)w * (uint32_t)h;
  int dx = 0, dy = 0;
  if (p.shift) {
    const int32_t* sh = p.shift + (view * p.S + s) * 2;
    dx = ol_clamp(sh[0], -OL_SHIFT_MAX, OL_SHIFT_MAX), dy = ol_clamp(sh[1], -OL_SHIFT_MAX, OL_SHIFT_MAX);
  }
  const long vo = view * H;                                                  // first row of the view in gt / occupied
  const long go = p.tiled ? ((long)b * 2 * H + (long)(v >> 1) * H) : vo;    // ... and in gen
  const long gw = p.tiled ? 2L * W : (long)W, gx = p.tiled ? (long)(v & 1) * W : 0L;
  const SphereAtlas atlas{p.atlas, p.T, p.th, p.tw};
  uint32_t se_gen = 0, n_gen = 0, se_gt = 0, n_gt = 0;
  for (uint32_t i = threadIdx.x; i < npix; i += OL_THREADS) {
    const uint32_t ly = i / (uint32_t)w, lx = i - ly * (uint32_t)w;
    const int x = x0 + (int)lx, y = y0 + (int)ly;
    const long po = (vo + y) * W + x;
    if (((ol_gptr8)p.occupied)[po] == 0) continue;
    uint8_t c8[3];
    shade_pixel(sph, n, atlas, cam, p.samples, x, y, c8[0], c8[1], c8[2]);
    const int c[3] = {c8[0], c8[1], c8[2]};
    const ol_gptr8 t8 = (ol_gptr8)(p.gt + po * 3);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int d = c[j] - (int)t8[j];
      se_gt += (uint32_t)(d * d);
    }
    n_gt += 1;
    const int xs = x + dx, ys = y + dy;
    if (xs >= 0 && xs < W && ys >= 0 && ys < H) {  // inside the view's own H x W (its own tile, when tiled)
      const ol_gptr8 g8 = (ol_gptr8)(p.gen + ((go + ys) * gw + gx + xs) * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int d = c[j] - (int)g8[j];
        se_gen += (uint32_t)(d * d);
      }
      n_gen += 1;
    }
  }
  const int wave = threadIdx.x >> 6;
  {
    const uint32_t glo = ol_wave_sum(se_gen & 0xFFFFFFu), ghi = ol_wave_sum(se_gen >> 24), gn = ol_wave_sum(n_gen);
    const uint32_t tlo = ol_wave_sum(se_gt & 0xFFFFFFu), thi = ol_wave_sum(se_gt >> 24), tn = ol_wave_sum(n_gt);
    if ((threadIdx.x & 63) == 0) {
      part[wave][0] = (unsigned long long)glo + ((unsigned long long)ghi << 24);
      part[wave][1] = gn;
      part[wave][2] = (unsigned long long)tlo + ((unsigned long long)thi << 24);
      part[wave][3] = tn;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* o = p.out + (((((long)(p.row0 + b) * p.V + v) * p.S + s) * p.K + k) * OL_ORI_COLS);
#pragma unroll
    for (int j = 0; j < OL_ORI_COLS; ++j) {
      unsigned long long t = 0;
#pragma unroll
      for (int q = 0; q < OL_THREADS / 64; ++q) t += part[q][j];
      o[j] = t;
    }
  }
}

}  // namespace

extern "C" int32_t gn_openloop_orientation(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* occupied, const int32_t* win,
                                           const int32_t* win_host, const float* cams, const float* spheres, const int32_t* tex_index, const int32_t* count,
                                           const uint8_t* atlas, const float* rot, const int32_t* shift, uint64_t* ori_out, int32_t B, int32_t V, int32_t H,
                                           int32_t W, int32_t S, int32_t K, int32_t T, int32_t th, int32_t tw, int32_t samples, int32_t tiled, int32_t row0,
                                           int32_t n_valid, int32_t rows) {
  GN_REQUIRE(ctx && gen && gt && occupied && win && cams && spheres && tex_index && count && atlas && rot && ori_out, "gn_openloop_orientation: null argument");
  GN_REQUIRE(B > 0 && B <= 65535 && V > 0 && V <= 65535 && (int64_t)B * V <= 65535 && H > 0 && W > 0 && (int64_t)H * W * 3 <= INT32_MAX,
             "gn_openloop_orientation: B (%d), V (%d), H (%d), W (%d) out of range (B * V <= 65535)", B, V, H, W);
  GN_REQUIRE(S >= 1 && S <= MAX_SPHERES, "gn_openloop_orientation: S (%d) must lie in [1, %d]", S, MAX_SPHERES);
  GN_REQUIRE(K >= 1 && K <= OL_ORI_K_MAX, "gn_openloop_orientation: K (%d) must lie in [1, %d]", K, OL_ORI_K_MAX);
  GN_REQUIRE(samples == 1 || samples == 4, "gn_openloop_orientation: samples (%d) must be 1 or 4", samples);
  GN_REQUIRE(T > 0 && th > 0 && tw > 0, "gn_openloop_orientation: the atlas is [T][th][tw][4] with T (%d), th (%d), tw (%d) > 0", T, th, tw);
  GN_REQUIRE(!tiled || V == 4, "gn_openloop_orientation: the tiled layout holds 4 views, got V = %d", V);
  GN_REQUIRE(n_valid >= 0 && n_valid <= B && row0 >= 0 && (int64_t)row0 + n_valid <= rows,
             "gn_openloop_orientation: n_valid (%d) must lie in [0, B = %d] and rows row0 (%d) .. row0 + n_valid inside the table's %d", n_valid, B, row0, rows);
  GN_REQUIRE((((uintptr_t)win | (uintptr_t)win_host | (uintptr_t)cams | (uintptr_t)spheres | (uintptr_t)tex_index | (uintptr_t)count | (uintptr_t)atlas |
               (uintptr_t)rot | (uintptr_t)shift) & 3) == 0 && ((uintptr_t)ori_out & 7) == 0,
             "gn_openloop_orientation: win, win_host, cams, spheres, tex_index, count, atlas, rot and shift must be 4-byte and ori_out 8-byte aligned");
  if (win_host) {
    const int32_t rc = ol_check_windows("gn_openloop_orientation", win_host, (int64_t)B * V * S, W, H);
    if (rc != GN_OK) return rc;
  }
  if (n_valid == 0) return GN_OK;
  OriParams p;
  p.gen = gen, p.gt = gt, p.occupied = occupied, p.win = win, p.cams = cams, p.spheres = spheres, p.tex_index = tex_index, p.count = count;
  p.atlas = atlas, p.rot = rot, p.shift = shift, p.out = (unsigned long long*)ori_out;
  p.V = V, p.H = H, p.W = W, p.S = S, p.K = K, p.T = T, p.th = th, p.tw = tw, p.samples = samples, p.tiled = tiled ? 1 : 0, p.row0 = row0;
  hipLaunchKernelGGL(openloop_orientation_kernel, dim3((unsigned)K, (unsigned)S, (unsigned)(n_valid * V)), dim3(OL_THREADS), 0, ctx->stream, p);
  GN_LAUNCH_CHECK();
  return GN_OK;
}
