// Scores of the open-loop evaluation (genima_amd/openloop.py OpenLoopEval): a generated image against the rendered ground truth under the
// renderer's `occupied` mask, and a predicted action chunk against the demo's.  include/genima_hip.h states both rules.
//
// Image kernel.  Grid: x = blocks of 4-pixel threads over one view (a thread owns pixels x0 .. x0 + 3 of one image row), y = view, z = sample
// (only the n_valid scored ones are launched).  A thread whose three addresses sit on the dword grid and whose four pixels lie inside the row
// loads 12 + 12 + 4 bytes as 3 + 3 + 1 dwords; a row tail (W % 4) and a row that starts off the grid (W * 3 % 4 != 0) take byte loads.  Every
// sum is an integer: a thread's fit 32 bits (<= 4 * 3 * 255^2), a block's too (x 256), so the block folds them with DPP adds and one LDS
// hand-off between its four waves, and five 64-bit vector atomics per block add them to the view's row, which the entry point zeroed on the
// same stream.  Integer addition commutes, so the bits do not depend on the order the blocks arrive in.  No thread leaves before the fold.
//
// Sphere kernel.  Grid: x = sphere, y = view, z = sample (only the n_valid scored ones): one workgroup per window, 256 threads striding its
// at most 256 x 256 pixels (pixel i of the window -> ly = i / w, lx = i - ly * w), byte loads (windows are small and their rows start anywhere).
// A thread sees at most 256 pixels, so 14 of its 16 sums fit 32 bits, and so does a wave's total of them (<= 64 * 256 * 765 * 255 = 3.2e9);
// the two second moments (<= 256 * 765 * 130 050 = 2.5e10) are 64-bit per thread and go through the wave sum as a 24-bit low part and a high
// part.  The four waves' totals meet in LDS as 64-bit values; threads 0 .. 16 add them and store the window's 17 values with plain stores: the
// workgroup owns its row, so there is no atomic, no memset, and an empty window writes its 17 zeros itself.  No thread leaves before the fold.
//
// Action kernel.  One thread per (sample, chunk position): the A - 1 joint terms in index order in f32 (this file is compiled without fma
// contraction, so a term is one subtraction, one multiplication and one addition, each rounded), then the gripper flag.
//
// Executed-action kernel (gn_openloop_exec_metrics).  One thread per transition: the action kernel's joint sum and gripper rule on the action an
// execution mode executes at that step (gn_openloop_exec_actions' output; that kernel is in ensemble.hip, beside the rule it replays), and the
// joint-space jump from the step before, of the executed and of the demo's action.  A thread reads rows n - 1 and n, writes row n.
//
// Triangulation kernel (gn_openloop_triangulate).  One thread per (transition, group, kind), one launch over the whole table after the last
// batch: the thread walks the at most 8 views twice -- once to sum the normal equations of the closest point to the used rays, once for the
// residuals at the solved point -- and rebuilds each ray from the tables both times instead of keeping eight of them in scratch.  All f64, no
// contraction (this file's flag), the 3x3 system through its adjugate in one written order; the thread stores its own eight values.
#include "openloop_common.h"

namespace {

struct ol_acc {
  uint32_t v[5];  // se_in, n_in, se_out, n_out, wrap_sq
};

__device__ __forceinline__ void ol_pixel(ol_acc& a, const uint8_t* g, const uint8_t* t, uint8_t occ) {
  uint32_t se = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int d = (int)g[c] - (int)t[c];
    se += (uint32_t)(d * d);
    const uint32_t w = (uint32_t)d & 255u;
    a.v[4] += (w * w) & 255u;
  }
  if (occ) {
    a.v[0] += se;
    a.v[1] += 1;
  } else {
    a.v[2] += se;
    a.v[3] += 1;
  }
}

__global__ __launch_bounds__(OL_THREADS) void openloop_image_kernel(const uint8_t* __restrict__ gen, const uint8_t* __restrict__ gt,
                                                                    const uint8_t* __restrict__ occupied, unsigned long long* __restrict__ out, int V,
                                                                    int H, int W, int tiled, int row0) {
  __shared__ uint32_t part[OL_THREADS / 64][5];
  const int b = blockIdx.z, v = blockIdx.y;
  const int G = (W + 3) >> 2;  // 4-pixel groups per image row
  const long t = (long)blockIdx.x * OL_THREADS + threadIdx.x;
  const int y = (int)(t / G), x0 = (int)(t - (long)y * G) * 4;
  ol_acc a = {{0, 0, 0, 0, 0}};
  if (y < H) {
    const long view = (long)b * V + v;
    const long po = (view * H + y) * W + x0;  // pixel offset in gt / occupied
    const long pg = tiled ? (((long)b * 2 * H + (long)(v >> 1) * H + y) * (2L * W) + (long)(v & 1) * W + x0) : po;
    const ol_gptr8 g8 = (ol_gptr8)(gen + pg * 3), t8 = (ol_gptr8)(gt + po * 3), o8 = (ol_gptr8)(occupied + po);
    uint8_t gb[12], tb[12], ob[4];
    int cnt = W - x0 < 4 ? W - x0 : 4;
    if (cnt == 4 && (((uintptr_t)g8 | (uintptr_t)t8 | (uintptr_t)o8) & 3) == 0) {
      const ol_gptr32 gw = (ol_gptr32)g8, tw = (ol_gptr32)t8;
      const uint32_t gq[3] = {gw[0], gw[1], gw[2]}, tq[3] = {tw[0], tw[1], tw[2]}, oq = *(ol_gptr32)o8;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        gb[i] = (uint8_t)(gq[i >> 2] >> ((i & 3) * 8));
        tb[i] = (uint8_t)(tq[i >> 2] >> ((i & 3) * 8));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) ob[j] = (uint8_t)(oq >> (j * 8));
#pragma unroll
      for (int j = 0; j < 4; ++j) ol_pixel(a, gb + j * 3, tb + j * 3, ob[j]);
    } else {
      for (int j = 0; j < cnt; ++j) {
        const uint8_t gp[3] = {g8[j * 3], g8[j * 3 + 1], g8[j * 3 + 2]}, tp[3] = {t8[j * 3], t8[j * 3 + 1], t8[j * 3 + 2]};
        ol_pixel(a, gp, tp, o8[j]);
      }
    }
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint32_t s = ol_wave_sum(a.v[i]);
    if ((threadIdx.x & 63) == 0) part[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < OL_THREADS / 64; ++w) s += part[w][threadIdx.x];
    if (s) atomicAdd(out + ((long)(row0 + b) * V + v) * 5 + threadIdx.x, (unsigned long long)s);
  }
}

constexpr int OL_SPH_COLS = 17;

__global__ __launch_bounds__(OL_THREADS) void openloop_sphere_kernel(const uint8_t* __restrict__ gen, const uint8_t* __restrict__ gt,
                                                                     const uint8_t* __restrict__ cond, const uint8_t* __restrict__ occupied,
                                                                     const int32_t* __restrict__ win, unsigned long long* __restrict__ out, int V, int H,
                                                                     int W, int S, int tiled, int threshold, int row0) {
  __shared__ unsigned long long part[OL_THREADS / 64][OL_SPH_COLS - 1];
  const int s = blockIdx.x, v = blockIdx.y, b = blockIdx.z;
  const long view = (long)b * V + v;
  const int32_t* wp = win + (view * S + s) * 4;
  // clamped into the image and to OL_WIN_MAX per side: no address below depends on the table's values being sane
  const int x0 = ol_clamp(wp[0], 0, W), y0 = ol_clamp(wp[1], 0, H);
  const int w = ol_clamp(ol_clamp(wp[2], 0, W) - x0, 0, OL_WIN_MAX), h = ol_clamp(ol_clamp(wp[3], 0, H) - y0, 0, OL_WIN_MAX);
  const uint32_t n = (uint32_t)w * (uint32_t)h;
  const long vo = view * H;                                                    // first row of the view in gt / cond / occupied
  const long go = tiled ? ((long)b * 2 * H + (long)(v >> 1) * H) : vo;        // ... and in gen
  const long gw = tiled ? 2L * W : (long)W, gx = tiled ? (long)(v & 1) * W : 0L;
  uint32_t a[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // columns 1-3, 5-7, 9-16
  unsigned long long m2g = 0, m2t = 0;                         // columns 4 and 8
  for (uint32_t i = threadIdx.x; i < n; i += OL_THREADS) {
    const uint32_t ly = i / (uint32_t)w, lx = i - ly * (uint32_t)w;
    const int x = x0 + (int)lx, y = y0 + (int)ly;
    const long po = (vo + y) * W + x;
    const ol_gptr8 g8 = (ol_gptr8)(gen + ((go + y) * gw + gx + x) * 3), t8 = (ol_gptr8)(gt + po * 3), c8 = (ol_gptr8)(cond + po * 3);
    const int g[3] = {g8[0], g8[1], g8[2]}, t[3] = {t8[0], t8[1], t8[2]}, c[3] = {c8[0], c8[1], c8[2]};
    const uint8_t occ = ((ol_gptr8)occupied)[po];
    int dg = 0, dt = 0;
    uint32_t se = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dg += abs(g[k] - c[k]);
      dt += abs(t[k] - c[k]);
      se += (uint32_t)((g[k] - t[k]) * (g[k] - t[k]));
    }
    const uint32_t ag = dg > threshold ? (uint32_t)(dg - threshold) : 0u, at = dt > threshold ? (uint32_t)(dt - threshold) : 0u;
    const uint32_t r2 = lx * lx + ly * ly;
    a[0] += ag;
    a[1] += ag * lx;
    a[2] += ag * ly;
    m2g += (unsigned long long)(ag * r2);  // <= 765 * 130 050: the product fits 32 bits
    a[3] += at;
    a[4] += at * lx;
    a[5] += at * ly;
    m2t += (unsigned long long)(at * r2);
    if (occ) {
      a[6] += 1;
      a[7] += se;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[8 + k] += (uint32_t)g[k];
        a[11 + k] += (uint32_t)t[k];
      }
    }
  }
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  // LDS slot = column - 1
  constexpr int slot[14] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15};
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const uint32_t t = ol_wave_sum(a[i]);
    if (lead) part[wave][slot[i]] = t;
  }
  {
    const uint32_t glo = ol_wave_sum((uint32_t)m2g & 0xFFFFFFu), ghi = ol_wave_sum((uint32_t)(m2g >> 24));
    const uint32_t tlo = ol_wave_sum((uint32_t)m2t & 0xFFFFFFu), thi = ol_wave_sum((uint32_t)(m2t >> 24));
    if (lead) {
      part[wave][3] = (unsigned long long)glo + ((unsigned long long)ghi << 24);
      part[wave][7] = (unsigned long long)tlo + ((unsigned long long)thi << 24);
    }
  }
  __syncthreads();
  if (threadIdx.x < OL_SPH_COLS) {
    unsigned long long t = n;  // column 0: the window's area
    if (threadIdx.x > 0) {
      t = 0;
#pragma unroll
      for (int k = 0; k < OL_THREADS / 64; ++k) t += part[k][threadIdx.x - 1];
    }
    out[((((long)(row0 + b) * V + v) * S + s) * OL_SPH_COLS) + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(OL_THREADS) void openloop_action_kernel(const f16* __restrict__ a_hat, long ld_hat, long bs_hat, const float* __restrict__ actions,
                                                                     const float* __restrict__ joint_scale, float* __restrict__ out, int T, int A, int row0,
                                                                     int n) {
  const int i = blockIdx.x * OL_THREADS + threadIdx.x;  // (sample, chunk position)
  if (i >= n) return;
  const int b = i / T, t = i - b * T;
  const f16* h = a_hat + (long)b * bs_hat + (long)t * ld_hat;
  const float* a = actions + (long)i * A;
  float sum = 0.0f;
  for (int j = 0; j < A - 1; ++j) {
    const float d = fabsf((float)h[j] - a[j]);
    sum += joint_scale ? joint_scale[j] * d : d;
  }
  float* o = out + ((long)(row0 + b) * T + t) * 2;
  o[0] = sum;
  o[1] = (((float)h[A - 1] > 0.0f) == (a[A - 1] > 0.5f)) ? 1.0f : 0.0f;
}

// sum_j scale[j] * |x[j] - y[j]| over the J joints in index order: one subtraction, one multiplication, one addition per term
__device__ __forceinline__ float ol_joint_l1(const float* x, const float* y, const float* __restrict__ scale, int J) {
  float sum = 0.0f;
  for (int j = 0; j < J; ++j) {
    const float d = fabsf(x[j] - y[j]);
    sum += scale ? scale[j] * d : d;
  }
  return sum;
}

__global__ __launch_bounds__(OL_THREADS) void openloop_exec_metrics_kernel(const float* __restrict__ exec, const float* __restrict__ demo,
                                                                           const int32_t* __restrict__ first_tr, const float* __restrict__ joint_scale,
                                                                           float* __restrict__ out, int N, int A) {
  const int n = blockIdx.x * OL_THREADS + threadIdx.x;
  if (n >= N) return;
  const float *x = exec + (long)n * A, *d = demo + (long)n * A;
  const bool first = n == 0 || first_tr[n] >= n;  // an episode's first step (a damaged entry above n reads as one too: row n - 1 is never needed then)
  float* o = out + (long)n * 4;
  o[0] = ol_joint_l1(x, d, joint_scale, A - 1);
  o[1] = ((x[A - 1] > 0.0f) == (d[A - 1] > 0.5f)) ? 1.0f : 0.0f;
  o[2] = first ? 0.0f : ol_joint_l1(x, x - A, joint_scale, A - 1);
  o[3] = first ? 0.0f : ol_joint_l1(d, d - A, joint_scale, A - 1);
}

// ---- triangulation (gn_openloop_triangulate) ----
constexpr int OL_TRI_COLS = 8;

struct ol_ray {
  double o[3], d[3];  // origin (the camera position), unit direction
  double u, v;        // the observation: the centroid in image coordinates
  double fx, fy, cx, cy, R[9];
};

// The observation and the ray of view v for group (n, g), or false where the view is not used.  Called by both passes over the views: the
// same statements on the same inputs, so both see the same bits.  A slot outside [0, S) reads as -1: no table value becomes an address
// unclamped.
__device__ __forceinline__ bool ol_tri_ray(const unsigned long long* __restrict__ sph, const int32_t* __restrict__ win, const float* __restrict__ cams,
                                           const int32_t* __restrict__ slot, long n, int g, int v, int kind, double min_ratio, int V, int S, int G,
                                           ol_ray& r) {
  const int s = slot[(n * G + g) * V + v];
  if (s < 0 || s >= S) return false;
  const long row = (n * V + v) * S + s;
  const unsigned long long* q = sph + row * OL_SPH_COLS;
  const double gen_m = (double)q[1], gt_m = (double)q[5];
  if (!(gt_m > 0.0)) return false;
  if (kind == 0 && !(gen_m > 0.0 && gen_m >= min_ratio * gt_m)) return false;
  const int o = kind == 0 ? 1 : 5;
  const double m = kind == 0 ? gen_m : gt_m;
  const int32_t* w = win + row * 4;
  r.u = ((double)w[0] + (double)q[o + 1] / m) + 0.5;
  r.v = ((double)w[1] + (double)q[o + 2] / m) + 0.5;
  const float* c = cams + (n * V + v) * 18;
  r.fx = (double)c[0], r.fy = (double)c[1], r.cx = (double)c[2], r.cy = (double)c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r.R[i * 3 + j] = (double)c[4 + i * 4 + j];
    r.o[i] = (double)c[4 + i * 4 + 3];
  }
  const double dx = (r.u - r.cx) / r.fx, dy = (r.cy - r.v) / r.fy;  // gn_render_spheres' ray through (u, v): pose * (dx, dy, -1)
  double e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) e[i] = (r.R[i * 3] * dx + r.R[i * 3 + 1] * dy) - r.R[i * 3 + 2];
  const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) r.d[i] = e[i] / len;
  return true;
}

__global__ __launch_bounds__(OL_THREADS) void openloop_triangulate_kernel(const unsigned long long* __restrict__ sph, const int32_t* __restrict__ win,
                                                                          const float* __restrict__ cams, const int32_t* __restrict__ slot,
                                                                          const double* __restrict__ centre, double* __restrict__ out, double min_ratio,
                                                                          double min_det, int N, int V, int S, int G) {
  const long i = (long)blockIdx.x * OL_THREADS + threadIdx.x;  // (n, g, kind)
  if (i >= (long)N * G * 2) return;
  const int kind = (int)(i & 1), g = (int)((i >> 1) % G);
  const long n = (i >> 1) / G;
  // A = sum (I - d d^T), b = sum (I - d d^T) o, over the used views in index order
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0, b0 = 0, b1 = 0, b2 = 0;
  int used = 0;
  ol_ray r;
  for (int v = 0; v < V; ++v) {
    if (!ol_tri_ray(sph, win, cams, slot, n, g, v, kind, min_ratio, V, S, G, r)) continue;
    ++used;
    const double t = (r.d[0] * r.o[0] + r.d[1] * r.o[1]) + r.d[2] * r.o[2];
    a00 += 1.0 - r.d[0] * r.d[0];
    a01 -= r.d[0] * r.d[1];
    a02 -= r.d[0] * r.d[2];
    a11 += 1.0 - r.d[1] * r.d[1];
    a12 -= r.d[1] * r.d[2];
    a22 += 1.0 - r.d[2] * r.d[2];
    b0 += r.o[0] - t * r.d[0];
    b1 += r.o[1] - t * r.d[1];
    b2 += r.o[2] - t * r.d[2];
  }
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double res[OL_TRI_COLS] = {(double)used, nan, nan, nan, nan, nan, nan, 0.0};
  if (used >= 2) {
    // the adjugate of the symmetric A, one fixed order of operations
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double m = ((a00 + a11) + a22) / 3.0;
    const double cond = det / ((m * m) * m);
    res[7] = cond;
    if (cond >= min_det) {  // a NaN stays unsolved
      const double x[3] = {((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det, ((c02 * b0 + c12 * b1) + c22 * b2) / det};
      const double* c = centre + (n * G + g) * 3;
      const double e0 = x[0] - c[0], e1 = x[1] - c[1], e2 = x[2] - c[2];
      double ray2 = 0.0, px2 = 0.0;
      for (int v = 0; v < V; ++v) {
        if (!ol_tri_ray(sph, win, cams, slot, n, g, v, kind, min_ratio, V, S, G, r)) continue;
        const double w0 = x[0] - r.o[0], w1 = x[1] - r.o[1], w2 = x[2] - r.o[2];
        const double t = (w0 * r.d[0] + w1 * r.d[1]) + w2 * r.d[2];
        const double p0 = w0 - t * r.d[0], p1 = w1 - t * r.d[1], p2 = w2 - t * r.d[2];
        ray2 += (p0 * p0 + p1 * p1) + p2 * p2;
        // the reprojection: render.sphere_windows' formulas, p = R^T (x - o), z = -p.z
        const double q0 = (r.R[0] * w0 + r.R[3] * w1) + r.R[6] * w2, q1 = (r.R[1] * w0 + r.R[4] * w1) + r.R[7] * w2;
        const double z = -((r.R[2] * w0 + r.R[5] * w1) + r.R[8] * w2);
        const double du = (r.cx + r.fx * q0 / z) - r.u, dv = (r.cy - r.fy * q1 / z) - r.v;
        px2 += z > 0.0 ? du * du + dv * dv : nan;  // a point at or behind a used camera has no reprojection
      }
      res[1] = x[0], res[2] = x[1], res[3] = x[2];
      res[4] = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
      res[5] = sqrt(ray2 / (double)used);
      res[6] = sqrt(px2 / (double)used);
    }
  }
  double* o = out + i * OL_TRI_COLS;
#pragma unroll
  for (int k = 0; k < OL_TRI_COLS; ++k) o[k] = res[k];
}

}  // namespace

extern "C" {

int32_t gn_openloop_image_metrics(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* occupied, uint64_t* img_out, int32_t B, int32_t V,
                                  int32_t H, int32_t W, int32_t tiled, int32_t row0, int32_t n_valid, int32_t rows) {
  GN_REQUIRE(ctx && gen && gt && occupied && img_out, "gn_openloop_image_metrics: null argument");
  GN_REQUIRE(B > 0 && B <= 65535 && V > 0 && V <= 65535 && H > 0 && W > 0 && (int64_t)H * W * 3 <= INT32_MAX,
             "gn_openloop_image_metrics: B (%d), V (%d), H (%d), W (%d) out of range", B, V, H, W);
  GN_REQUIRE(!tiled || V == 4, "gn_openloop_image_metrics: the tiled layout holds 4 views, got V = %d", V);
  GN_REQUIRE(n_valid >= 0 && n_valid <= B && row0 >= 0 && (int64_t)row0 + n_valid <= rows,
             "gn_openloop_image_metrics: n_valid (%d) must lie in [0, B = %d] and rows row0 (%d) .. row0 + n_valid inside the table's %d", n_valid, B, row0, rows);
  GN_REQUIRE(((uintptr_t)img_out & 7) == 0, "gn_openloop_image_metrics: img_out must be 8-byte aligned");
  if (n_valid == 0) return GN_OK;
  GN_HIP(hipMemsetAsync(img_out + (int64_t)row0 * V * 5, 0, (size_t)n_valid * V * 5 * sizeof(uint64_t), ctx->stream));
  const int64_t threads = (int64_t)H * ((W + 3) / 4);
  hipLaunchKernelGGL(openloop_image_kernel, dim3((unsigned)cdiv64(threads, OL_THREADS), (unsigned)V, (unsigned)n_valid), dim3(OL_THREADS), 0, ctx->stream, gen,
                     gt, occupied, (unsigned long long*)img_out, V, H, W, tiled ? 1 : 0, row0);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_sphere_metrics(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* cond, const uint8_t* occupied, const int32_t* win,
                                   const int32_t* win_host, uint64_t* sph_out, int32_t B, int32_t V, int32_t H, int32_t W, int32_t S, int32_t tiled,
                                   int32_t threshold, int32_t row0, int32_t n_valid, int32_t rows) {
  GN_REQUIRE(ctx && gen && gt && cond && occupied && win && sph_out, "gn_openloop_sphere_metrics: null argument");
  GN_REQUIRE(B > 0 && B <= 65535 && V > 0 && V <= 65535 && H > 0 && W > 0 && (int64_t)H * W * 3 <= INT32_MAX,
             "gn_openloop_sphere_metrics: B (%d), V (%d), H (%d), W (%d) out of range", B, V, H, W);
  GN_REQUIRE(S >= 1 && S <= 8, "gn_openloop_sphere_metrics: S (%d) must lie in [1, 8]", S);
  GN_REQUIRE(threshold >= 0, "gn_openloop_sphere_metrics: threshold (%d) must not be negative", threshold);
  GN_REQUIRE(!tiled || V == 4, "gn_openloop_sphere_metrics: the tiled layout holds 4 views, got V = %d", V);
  GN_REQUIRE(n_valid >= 0 && n_valid <= B && row0 >= 0 && (int64_t)row0 + n_valid <= rows,
             "gn_openloop_sphere_metrics: n_valid (%d) must lie in [0, B = %d] and rows row0 (%d) .. row0 + n_valid inside the table's %d", n_valid, B, row0, rows);
  GN_REQUIRE(((uintptr_t)win & 3) == 0 && ((uintptr_t)win_host & 3) == 0 && ((uintptr_t)sph_out & 7) == 0,
             "gn_openloop_sphere_metrics: win must be 4-byte and sph_out 8-byte aligned");
  if (win_host) {
    const int32_t rc = ol_check_windows("gn_openloop_sphere_metrics", win_host, (int64_t)B * V * S, W, H);
    if (rc != GN_OK) return rc;
  }
  if (n_valid == 0) return GN_OK;
  hipLaunchKernelGGL(openloop_sphere_kernel, dim3((unsigned)S, (unsigned)V, (unsigned)n_valid), dim3(OL_THREADS), 0, ctx->stream, gen, gt, cond, occupied, win,
                     (unsigned long long*)sph_out, V, H, W, S, tiled ? 1 : 0, threshold, row0);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_action_metrics(gn_ctx* ctx, const void* a_hat, int64_t ld_hat, int64_t bs_hat, const float* actions, const float* joint_scale,
                                   float* act_out, int32_t B, int32_t T, int32_t A, int32_t row0, int32_t n_valid, int32_t rows) {
  GN_REQUIRE(ctx && a_hat && actions && act_out, "gn_openloop_action_metrics: null argument");
  GN_REQUIRE(B > 0 && T > 0 && A >= 2 && (int64_t)B * T <= (1 << 24), "gn_openloop_action_metrics: B (%d), T (%d), A (%d) out of range", B, T, A);
  GN_REQUIRE(ld_hat >= A && bs_hat >= (int64_t)(T - 1) * ld_hat + A, "gn_openloop_action_metrics: a_hat pitch %ld / sample stride %ld too small for T = %d, A = %d",
             (long)ld_hat, (long)bs_hat, T, A);
  GN_REQUIRE(n_valid >= 0 && n_valid <= B && row0 >= 0 && (int64_t)row0 + n_valid <= rows,
             "gn_openloop_action_metrics: n_valid (%d) must lie in [0, B = %d] and rows row0 (%d) .. row0 + n_valid inside the table's %d", n_valid, B, row0, rows);
  GN_REQUIRE((((uintptr_t)a_hat) & 1) == 0 && (((uintptr_t)actions | (uintptr_t)joint_scale | (uintptr_t)act_out) & 3) == 0,
             "gn_openloop_action_metrics: misaligned argument");
  if (n_valid == 0) return GN_OK;
  const int n = n_valid * T;
  hipLaunchKernelGGL(openloop_action_kernel, dim3((unsigned)cdiv64(n, OL_THREADS)), dim3(OL_THREADS), 0, ctx->stream, (const f16*)a_hat, (long)ld_hat,
                     (long)bs_hat, actions, joint_scale, act_out, T, A, row0, n);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_exec_metrics(gn_ctx* ctx, const float* exec, const float* demo, const int32_t* first_tr, const float* joint_scale, float* out, int32_t N,
                                 int32_t A) {
  GN_REQUIRE(ctx && exec && demo && first_tr && out, "gn_openloop_exec_metrics: null argument");
  GN_REQUIRE(N > 0 && A >= 2 && (int64_t)N * A <= INT32_MAX, "gn_openloop_exec_metrics: N (%d), A (%d) out of range", N, A);
  GN_REQUIRE((((uintptr_t)exec | (uintptr_t)demo | (uintptr_t)first_tr | (uintptr_t)joint_scale | (uintptr_t)out) & 3) == 0,
             "gn_openloop_exec_metrics: misaligned argument");
  hipLaunchKernelGGL(openloop_exec_metrics_kernel, dim3((unsigned)cdiv64(N, OL_THREADS)), dim3(OL_THREADS), 0, ctx->stream, exec, demo, first_tr, joint_scale,
                     out, N, A);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_triangulate(gn_ctx* ctx, const uint64_t* sph, const int32_t* win, const float* cams, const int32_t* slot, const double* centre,
                                const int32_t* slot_host, const int32_t* win_host, double* out, double min_ratio, double min_det, int32_t N, int32_t V,
                                int32_t S, int32_t G) {
  GN_REQUIRE(ctx && sph && win && cams && slot && centre && out, "gn_openloop_triangulate: null argument");
  GN_REQUIRE(N >= 0 && V >= 2 && V <= 8 && S >= 1 && S <= 8 && G >= 1 && G <= 8 && (int64_t)N * V * S * OL_SPH_COLS <= INT32_MAX,
             "gn_openloop_triangulate: N (%d) must not be negative, V (%d) must lie in [2, 8], S (%d) and G (%d) in [1, 8]", N, V, S, G);
  GN_REQUIRE(min_ratio >= 0.0 && min_det > 0.0, "gn_openloop_triangulate: min_ratio (%g) must be >= 0 and min_det (%g) > 0", min_ratio, min_det);
  GN_REQUIRE((((uintptr_t)sph | (uintptr_t)centre | (uintptr_t)out) & 7) == 0 &&
                 (((uintptr_t)win | (uintptr_t)cams | (uintptr_t)slot | (uintptr_t)slot_host | (uintptr_t)win_host) & 3) == 0,
             "gn_openloop_triangulate: sph, centre and out must be 8-byte, win, cams, slot and the host copies 4-byte aligned");
  if (slot_host) {
    for (int64_t i = 0; i < (int64_t)N * G * V; ++i)
      GN_REQUIRE(slot_host[i] >= -1 && slot_host[i] < S, "gn_openloop_triangulate: slot %ld = %d must lie in [-1, S = %d)", (long)i, slot_host[i], S);
  }
  if (win_host) {
    for (int64_t i = 0; i < (int64_t)N * V * S; ++i) {
      const int32_t* q = win_host + i * 4;
      GN_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[2] >= q[0] && q[3] >= q[1] && q[2] - q[0] <= OL_WIN_MAX && q[3] - q[1] <= OL_WIN_MAX,
                 "gn_openloop_triangulate: window %ld = (%d, %d, %d, %d) must have 0 <= x0 <= x1, 0 <= y0 <= y1 and at most %d per side", (long)i, q[0], q[1],
                 q[2], q[3], OL_WIN_MAX);
    }
  }
  if (N == 0) return GN_OK;
  hipLaunchKernelGGL(openloop_triangulate_kernel, dim3((unsigned)cdiv64((int64_t)N * G * 2, OL_THREADS)), dim3(OL_THREADS), 0, ctx->stream,
                     (const unsigned long long*)sph, win, cams, slot, centre, out, min_ratio, min_det, N, V, S, G);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"
