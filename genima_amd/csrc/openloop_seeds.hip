// The seed axis of the open-loop evaluation (genima_amd/openloop.py OpenLoopEval(seeds=R)): two reductions over the R generator seeds a run
// was repeated with, one launch each over the finished tables after the last batch.  include/genima_hip.h states both rules.
//
// Sphere kernel (gn_openloop_seed_spheres).  One thread per (transition, view, sphere), 256 per workgroup.  The thread walks the R seeds'
// rows of the sphere table twice, in seed order: once for the count and the sums of the centroids and the mass ratios, once for the squared
// distances to the mean, to the true centroid and the largest of them.  Both passes rebuild a seed's centroid from the table with the same
// statements (seed_centroid below), so both see the same bits and nothing is kept per seed.  All f64; a column of the table stays below
// 6.6e12, so its conversion is exact.  The thread stores its own eight values.
//
// Action kernel (gn_openloop_seed_actions).  One thread per (transition, chunk position).  Per joint j the R f16 values are widened and added
// in seed order in f32, the sum is multiplied by inv_R, and the deviations from that mean are added in a second walk over the seeds; column 3
// re-runs gn_openloop_action_metrics' own joint sum per seed -- the same statement under the same flag -- and averages the R results in seed
// order.  The thread stores its own four values.
//
// Both: plain loads and stores, no atomics, no zeroing pass, no sqrt and no exp; this file is built with -ffp-contract=off like openloop.hip,
// so a term is one rounded operation after another and every run gives the same bits.
#include "openloop_common.h"

namespace {

constexpr int OLS_SPH_COLS = 17;  // gn_openloop_sphere_metrics' row
constexpr int OLS_OUT_COLS = 8;
constexpr int OLS_MAX_SEEDS = 64;

// Seed r's centroid and mass ratio for one sphere, or false where the seed did not find it (gn_openloop_triangulate's rule for kind 0).
__device__ __forceinline__ bool seed_centroid(const unsigned long long* __restrict__ q, double gt_m, double min_ratio, double& cx, double& cy,
                                              double& ratio) {
  const double gen_m = (double)q[1];
  if (!(gen_m > 0.0 && gt_m > 0.0 && gen_m >= min_ratio * gt_m)) return false;
  cx = (double)q[2] / gen_m;
  cy = (double)q[3] / gen_m;
  ratio = gen_m / gt_m;
  return true;
}

__global__ __launch_bounds__(OL_THREADS) void openloop_seed_spheres_kernel(const unsigned long long* __restrict__ sph, double* __restrict__ out,
                                                                           double min_ratio, int R, long rows) {
  const long i = (long)blockIdx.x * OL_THREADS + threadIdx.x;  // (n, v, s)
  if (i >= rows) return;
  const long seed_stride = rows * OLS_SPH_COLS;
  const unsigned long long* q0 = sph + i * OLS_SPH_COLS;  // seed 0's row: the ground-truth columns are the same for every seed
  const double gt_m = (double)q0[5];
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double res[OLS_OUT_COLS] = {0.0, nan, nan, nan, nan, nan, nan, nan};
  int k = 0;
  double sx = 0.0, sy = 0.0, sq = 0.0, cx, cy, ratio;
  for (int r = 0; r < R; ++r) {
    if (!seed_centroid(q0 + (long)r * seed_stride, gt_m, min_ratio, cx, cy, ratio)) continue;
    ++k;
    sx += cx;
    sy += cy;
    sq += ratio;
  }
  res[0] = (double)k;
  if (k > 0) {  // hence gt_m > 0
    const double kd = (double)k;
    const double mx = sx / kd, my = sy / kd, mq = sq / kd;
    const double tx = (double)q0[6] / gt_m, ty = (double)q0[7] / gt_m;
    double spread = 0.0, shift = 0.0, qvar = 0.0, worst = 0.0;
    for (int r = 0; r < R; ++r) {
      if (!seed_centroid(q0 + (long)r * seed_stride, gt_m, min_ratio, cx, cy, ratio)) continue;
      const double ax = cx - mx, ay = cy - my, bx = cx - tx, by = cy - ty, dq = ratio - mq;
      const double d2 = bx * bx + by * by;
      spread += ax * ax + ay * ay;
      shift += d2;
      qvar += dq * dq;
      worst = d2 > worst ? d2 : worst;
    }
    res[1] = mx - tx;
    res[2] = my - ty;
    res[3] = spread / kd;
    res[4] = shift / kd;
    res[5] = mq;
    res[6] = qvar / kd;
    res[7] = worst;
  }
  double* o = out + i * OLS_OUT_COLS;
#pragma unroll
  for (int c = 0; c < OLS_OUT_COLS; ++c) o[c] = res[c];
}

__global__ __launch_bounds__(OL_THREADS) void openloop_seed_actions_kernel(const f16* __restrict__ chunks, long ld, const float* __restrict__ demo,
                                                                           const float* __restrict__ joint_scale, float* __restrict__ out, float inv_R,
                                                                           int R, long rows, int A) {
  const long i = (long)blockIdx.x * OL_THREADS + threadIdx.x;  // (n, t)
  if (i >= rows) return;
  const f16* h0 = chunks + i * ld;  // seed 0's row; seed r's lies r * seed_stride further
  const long seed_stride = rows * ld;
  const float* a = demo + i * A;
  float err_mean = 0.0f, mad = 0.0f;
  for (int j = 0; j < A - 1; ++j) {
    float s = 0.0f;
    for (int r = 0; r < R; ++r) s += (float)h0[(long)r * seed_stride + j];
    const float mean = s * inv_R;
    float dev = 0.0f;
    for (int r = 0; r < R; ++r) dev += fabsf((float)h0[(long)r * seed_stride + j] - mean);
    const float d = fabsf(mean - a[j]), m = dev * inv_R;
    err_mean += joint_scale ? joint_scale[j] * d : d;
    mad += joint_scale ? joint_scale[j] * m : m;
  }
  float grip = 0.0f, errs = 0.0f;
  for (int r = 0; r < R; ++r) {
    const f16* h = h0 + (long)r * seed_stride;
    grip += (float)h[A - 1];
    float sum = 0.0f;  // gn_openloop_action_metrics' joint sum of seed r, statement for statement
    for (int j = 0; j < A - 1; ++j) {
      const float d = fabsf((float)h[j] - a[j]);
      sum += joint_scale ? joint_scale[j] * d : d;
    }
    errs += sum;
  }
  float* o = out + i * 4;
  o[0] = err_mean;
  o[1] = ((grip * inv_R > 0.0f) == (a[A - 1] > 0.5f)) ? 1.0f : 0.0f;
  o[2] = mad;
  o[3] = errs * inv_R;
}

}  // namespace

extern "C" {

int32_t gn_openloop_seed_spheres(gn_ctx* ctx, const uint64_t* sph, double* out, double min_ratio, int32_t R, int32_t N, int32_t V, int32_t S) {
  GN_REQUIRE(ctx && sph && out, "gn_openloop_seed_spheres: null argument");
  GN_REQUIRE(R >= 1 && R <= OLS_MAX_SEEDS, "gn_openloop_seed_spheres: R (%d) must lie in [1, %d]", R, OLS_MAX_SEEDS);
  GN_REQUIRE(N >= 0 && V >= 2 && V <= 8 && S >= 1 && S <= 8 && (int64_t)N * V * S * OLS_SPH_COLS <= INT32_MAX,
             "gn_openloop_seed_spheres: N (%d) must not be negative, V (%d) must lie in [2, 8], S (%d) in [1, 8]", N, V, S);
  GN_REQUIRE(min_ratio >= 0.0, "gn_openloop_seed_spheres: min_ratio (%g) must be >= 0", min_ratio);
  GN_REQUIRE((((uintptr_t)sph | (uintptr_t)out) & 7) == 0, "gn_openloop_seed_spheres: sph and out must be 8-byte aligned");
  if (N == 0) return GN_OK;
  const int64_t rows = (int64_t)N * V * S;
  hipLaunchKernelGGL(openloop_seed_spheres_kernel, dim3((unsigned)cdiv64(rows, OL_THREADS)), dim3(OL_THREADS), 0, ctx->stream,
                     (const unsigned long long*)sph, out, min_ratio, R, (long)rows);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_seed_actions(gn_ctx* ctx, const void* chunks, int32_t ld, const float* demo, const float* joint_scale, float* out, float inv_R,
                                 int32_t R, int32_t N, int32_t T, int32_t A) {
  GN_REQUIRE(ctx && chunks && demo && out, "gn_openloop_seed_actions: null argument");
  GN_REQUIRE(R >= 1 && R <= OLS_MAX_SEEDS, "gn_openloop_seed_actions: R (%d) must lie in [1, %d]", R, OLS_MAX_SEEDS);
  GN_REQUIRE(N > 0 && T > 0 && A >= 2 && (int64_t)N * T <= (1 << 24), "gn_openloop_seed_actions: N (%d), T (%d), A (%d) out of range", N, T, A);
  GN_REQUIRE(ld >= A && (int64_t)R * N * T * ld <= INT32_MAX, "gn_openloop_seed_actions: row pitch ld (%d) < A (%d), or the table is too large", ld, A);
  GN_REQUIRE(inv_R == (float)(1.0 / (double)R), "gn_openloop_seed_actions: inv_R (%g) must be (float)(1.0 / R), R = %d", (double)inv_R, R);
  GN_REQUIRE((((uintptr_t)chunks) & 1) == 0 && (((uintptr_t)demo | (uintptr_t)joint_scale | (uintptr_t)out) & 3) == 0,
             "gn_openloop_seed_actions: misaligned argument");
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(openloop_seed_actions_kernel, dim3((unsigned)cdiv64(rows, OL_THREADS)), dim3(OL_THREADS), 0, ctx->stream, (const f16*)chunks,
                     (long)ld, demo, joint_scale, out, inv_R, R, (long)rows, A);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"
