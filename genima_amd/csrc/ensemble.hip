// Temporal ensembling of overlapping action chunks on the device (the ACT paper's rule, generalised from one executed action per call to h):
// the controller's recorded program ends in this one launch, the ring of recent chunks never leaves the device, and only `steps` / `reset`
// change between replays.
//
// State blob, per batch row (row pitch gn_action_ensemble_state_bytes / B):
//   float   ring[K][T][A]   the last K chunks
//   int32_t start[K]        environment step at which each slot's chunk starts, -1 = empty
//   int32_t head            the slot the next chunk goes into (= the oldest one)
//   int32_t magic           ENS_MAGIC once the row's bookkeeping has been written: a blob the caller zeroed reads as "every slot empty"
//
// One workgroup per batch row: it reads the row's bookkeeping, decides the new one in LDS, and only then (behind a workgroup barrier) writes it
// back; ring data is written to the slot being replaced alone, whose values the output pass takes from `chunk` itself -- so no thread reads
// a word another thread of the launch writes, and no other workgroup touches the row.  Plain loads and stores, no atomics.
//
// gn_openloop_exec_actions (further down) replays the same rule over the table of chunks an open-loop evaluation has kept: it lives in this
// file so that both kernels are compiled under the same contraction flags, and both take their weighted mean from ensemble_common.h.
#include "common.h"
#include "ensemble_common.h"

namespace {

constexpr int32_t ENS_MAGIC = 0x454E5331;  // "ENS1"
constexpr int ENS_MAX_K = 1024;  // start[] of a row in LDS

__host__ __device__ inline int64_t ens_row_bytes(int64_t T, int64_t A, int64_t K) { return (4 * (K * T * A + K + 2) + 15) / 16 * 16; }

// One row's call, by its workgroup: the bookkeeping, the new chunk into the slot it replaces, the h output rows.  fresh(off, a) is the new chunk's
// value at chunk position off, dimension a -- NOT read back from the ring, whose slot w this launch writes.
template <typename NEW>
__device__ __forceinline__ void ens_row_call(char* row, int32_t* s_start, int t, bool reset, float* out_row, int T, int A, int K, int h, float m,
                                             NEW&& fresh) {
  const int tid = threadIdx.x;
  float* ring = (float*)row;
  int32_t* start = (int32_t*)(row + 4l * K * T * A);
  const bool empty = reset || start[K + 1] != ENS_MAGIC;
  const int w = empty ? 0 : (int)((uint32_t)start[K] % (uint32_t)K);  // the slot the new chunk replaces (modulo: a damaged head stays in bounds)
  for (int k = tid; k < K; k += ENS_THREADS) s_start[k] = k == w ? t : (empty ? -1 : start[k]);
  __syncthreads();  // every thread has read the old bookkeeping
  for (int k = tid; k < K; k += ENS_THREADS) start[k] = s_start[k];
  if (tid == 0) {
    start[K] = (w + 1) % K;
    start[K + 1] = ENS_MAGIC;
  }
  float* mine = ring + (long)w * T * A;
  for (int e = tid; e < T * A; e += ENS_THREADS) mine[e] = fresh(e / A, e % A);
  for (int e = tid; e < h * A; e += ENS_THREADS) {
    const int so = e / A, a = e % A;
    const long s = (long)t + so;
    // rank among the slots that cover s, oldest first: the ring order from the slot behind w round to w is the order of insertion
    const float mean = ens_weighted_mean(K, m, nullptr, [&](int j, float& v) {
      const int k = (w + j + 1) % K;
      const int st = s_start[k];
      const long off = s - st;
      if (st < 0 || off < 0 || off >= T) return false;
      v = k == w ? fresh((int)off, a) : ring[((long)k * T + off) * A + a];
      return true;
    });
    out_row[(long)so * A + a] = mean;  // the new chunk covers every target step (h <= T): den >= its weight > 0
  }
}

template <typename TC>
__global__ __launch_bounds__(ENS_THREADS) void action_ensemble_kernel(const TC* __restrict__ chunk, char* __restrict__ state,
                                                                     const int32_t* __restrict__ steps, const uint8_t* __restrict__ reset,
                                                                     float* __restrict__ out, int T, int A, int ld, int K, int h, float m,
                                                                     long row_bytes) {
  __shared__ int32_t s_start[ENS_MAX_K];
  const int b = blockIdx.x;
  const TC* ck = chunk + (long)b * T * ld;
  ens_row_call(state + (long)b * row_bytes, s_start, steps[b], reset[b] != 0, out + (long)b * h * A, T, A, K, h, m,
               [&](int off, int a) { return ens_load(ck + (long)off * ld + a); });
}

// The same call over the combination of R sampled chunks (include/genima_hip.h, gn_action_ensemble_samples_f16): the workgroup stages the row's
// samples as f32 in LDS, combines them there (ensemble_common.h) and hands the combined chunk to ens_row_call out of LDS.
__global__ __launch_bounds__(ENS_THREADS) void action_ensemble_samples_kernel(const f16* __restrict__ chunk, long bs, long ss, int R, float inv_R,
                                                                             int combine, char* __restrict__ state,
                                                                             const int32_t* __restrict__ steps, const uint8_t* __restrict__ reset,
                                                                             float* __restrict__ out, int32_t* __restrict__ pick_out,
                                                                             float* __restrict__ spread_out, int T, int A, int ld, int K, int h,
                                                                             float m, long row_bytes) {
  __shared__ int32_t s_start[ENS_MAX_K];
  __shared__ float s_x[ENS_MAX_STAGED];
  __shared__ float s_part[ENS_PARTS];
  __shared__ int s_pick;
  const int b = blockIdx.x, tid = threadIdx.x, n = T * A;
  const f16* ck = chunk + (long)b * bs;
  for (int r = 0; r < R; ++r)
    for (int e = tid; e < n; e += ENS_THREADS) s_x[r * n + e] = ens_load(ck + (long)r * ss + (long)(e / A) * ld + e % A);
  __syncthreads();
  float spread;
  const int pick = ens_combine_samples(s_x, R, n, inv_R, combine, s_part, &s_pick, spread);
  if (tid == 0) {
    if (pick_out) pick_out[b] = pick;
    if (spread_out) spread_out[b] = spread;
  }
  ens_row_call(state + (long)b * row_bytes, s_start, steps[b], reset[b] != 0, out + (long)b * h * A, T, A, K, h, m,
               [&](int off, int a) { return s_x[off * A + a]; });
}

// What every launch of the row kernels refuses (include/genima_hip.h); align: the chunk's element size.
int32_t check_ensemble(gn_ctx* ctx, const char* who, const void* chunk, const void* state, const int32_t* steps, const uint8_t* reset, const float* out,
                       int32_t B, int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m, size_t align) {
  GN_REQUIRE(ctx && chunk && state && steps && reset && out, "%s: null argument", who);
  GN_REQUIRE(B > 0 && T > 0 && A > 0 && (int64_t)T * A <= (1 << 24) && (int64_t)B * T * ld <= INT32_MAX, "%s: B (%d), T (%d), A (%d) out of range", who, B, T, A);
  GN_REQUIRE(ld >= A, "%s: row pitch ld (%d) < A (%d)", who, ld, A);
  GN_REQUIRE(h >= 1 && h <= T, "%s: execution horizon h (%d) must lie in 1 .. T (%d)", who, h, T);
  GN_REQUIRE((K == 1 || K >= (T + h - 1) / h) && K <= ENS_MAX_K, "%s: K (%d) must be 1 (the new chunk alone) or lie in ceil(T / h) = %d .. %d", who, K,
             (T + h - 1) / h, ENS_MAX_K);
  GN_REQUIRE(m >= 0.f && m == m, "%s: m (%g) must be >= 0", who, (double)m);
  GN_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)steps & 3) == 0 && ((uintptr_t)chunk & (align - 1)) == 0,
             "%s: misaligned pointer (state: 16 bytes)", who);
  return GN_OK;
}

template <typename TC>
int32_t launch_ensemble(gn_ctx* ctx, const char* who, const TC* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B,
                        int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  if (int32_t e = check_ensemble(ctx, who, chunk, state, steps, reset, out, B, T, A, ld, K, h, m, sizeof(TC))) return e;
  hipLaunchKernelGGL(action_ensemble_kernel<TC>, dim3((unsigned)B), dim3(ENS_THREADS), 0, ctx->stream, chunk, (char*)state, steps, reset, out, T, A, ld, K,
                     h, m, (long)ens_row_bytes(T, A, K));
  GN_LAUNCH_CHECK();
  return GN_OK;
}

// What the sample arguments add to a refusal: `rows` samples rows of pitch bs, R samples of pitch ss in each, every sample [T][ld].
int32_t check_samples(const char* who, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine, int32_t rows, int32_t T, int32_t A, int32_t ld) {
  GN_REQUIRE(R >= 1 && R <= ENS_MAX_SAMPLES, "%s: R (%d) must lie in [1, %d]", who, R, ENS_MAX_SAMPLES);
  GN_REQUIRE((int64_t)R * T * A <= ENS_MAX_STAGED, "%s: R * T * A = %ld is more than the %d values a workgroup stages", who, (long)((int64_t)R * T * A),
             ENS_MAX_STAGED);
  GN_REQUIRE(inv_R == (float)(1.0 / (double)R), "%s: inv_R (%g) must be (float)(1.0 / R), R = %d", who, (double)inv_R, R);
  GN_REQUIRE(combine == 0 || combine == 1, "%s: combine (%d) must be 0 (mean) or 1 (medoid)", who, combine);
  const int64_t span = (int64_t)(T - 1) * ld + A;  // the elements of one sample from its first to its last
  const bool row_major = bs >= (int64_t)(R - 1) * ss + span, sample_major = ss >= (int64_t)(rows - 1) * bs + span;
  GN_REQUIRE(bs >= 0 && ss >= 0 && (R == 1 || ss >= span) && (rows == 1 || bs >= span) && (R == 1 || rows == 1 || row_major || sample_major),
             "%s: the strides (row %ld, sample %ld) make samples of %ld elements overlap", who, (long)bs, (long)ss, (long)span);
  GN_REQUIRE((int64_t)(rows - 1) * bs + (int64_t)(R - 1) * ss + span <= INT32_MAX, "%s: the sample table is too large", who);
  return GN_OK;
}

// The table replay of openloop_exec_actions_kernel with the value of (transition row, chunk position, dimension) left to the caller: value(row, off, a).
template <typename V>
__device__ __forceinline__ void openloop_exec_replay(const int32_t* __restrict__ first_tr, float* __restrict__ exec, int32_t* __restrict__ n_calls, int N,
                                                     int T, int A, int h, int agg, float m, V&& value) {
  const long e = (long)blockIdx.x * ENS_THREADS + threadIdx.x;
  if (e >= (long)N * A) return;
  const int n = (int)(e / A), a = (int)(e - (long)n * A);
  const int f0 = first_tr[n];
  const int f = f0 < 0 ? 0 : (f0 > n ? n : f0);  // a damaged table stays inside the buffer
  const int s = n - f, r = s % h, t = s - r;
  const int jmax = agg ? (T - 1 - r) / h : 0;  // r <= h - 1 <= T - 1: the oldest call that could still cover s started jmax calls before t
  int used;
  const float mean = ens_weighted_mean(jmax + 1, m, &used, [&](int j, float& v) {
    const int u = t - (jmax - j) * h;
    if (u < 0) return false;  // before the episode began
    v = value(f + u, s - u, a);
    return true;
  });
  exec[e] = mean;  // the call at t itself always takes part
  if (n_calls && a == 0) n_calls[n] = used;
}

// The ensemble rule replayed over an evaluation's table of chunks (include/genima_hip.h, gn_openloop_exec_actions).  One thread per (transition n,
// action dimension a); plain loads and stores, a thread writes exec[n][a] alone (and n_calls[n] where a == 0) and reads rows f .. n of `chunks`
// only: f is clamped into [0, n], u <= t <= s = n - f, and the offset s - u = s % h + (jmax - j) h <= T - 1 by the choice of jmax.
__global__ __launch_bounds__(ENS_THREADS) void openloop_exec_actions_kernel(const f16* __restrict__ chunks, const int32_t* __restrict__ first_tr,
                                                                           float* __restrict__ exec, int32_t* __restrict__ n_calls, int N, int T, int A,
                                                                           int ld, int h, int agg, float m) {
  openloop_exec_replay(first_tr, exec, n_calls, N, T, A, h, agg, m,
                       [&](int row, int off, int a) { return ens_load(chunks + ((long)row * T + off) * ld + a); });
}

// gn_openloop_exec_actions_samples, first launch (medoid only): one workgroup per transition stages its R samples and stores the pick.
__global__ __launch_bounds__(ENS_THREADS) void openloop_sample_picks_kernel(const f16* __restrict__ chunks, long ns, long ss, int R,
                                                                           int32_t* __restrict__ pick_out, int T, int A, int ld) {
  __shared__ float s_x[ENS_MAX_STAGED];
  __shared__ float s_part[ENS_PARTS];
  __shared__ int s_pick;
  const int tid = threadIdx.x, n = T * A;
  const f16* ck = chunks + (long)blockIdx.x * ns;
  for (int r = 0; r < R; ++r)
    for (int e = tid; e < n; e += ENS_THREADS) s_x[r * n + e] = ens_load(ck + (long)r * ss + (long)(e / A) * ld + e % A);
  __syncthreads();
  const int pick = ens_medoid_pick(s_x, R, n, s_part, &s_pick);
  if (tid == 0) pick_out[blockIdx.x] = pick;
}

// Second launch: the replay over the combined chunk of every transition -- the mean rebuilt per element by ens_sample_mean, or the sample the
// first launch picked.  `picks` (medoid) is read only; `pick_fill` (mean, or NULL) gets -1 from the thread of dimension 0.
__global__ __launch_bounds__(ENS_THREADS) void openloop_exec_actions_samples_kernel(const f16* __restrict__ chunks, long ns, long ss, int R, float inv_R,
                                                                                   const int32_t* __restrict__ picks, int32_t* __restrict__ pick_fill,
                                                                                   const int32_t* __restrict__ first_tr, float* __restrict__ exec,
                                                                                   int32_t* __restrict__ n_calls, int N, int T, int A, int ld, int h,
                                                                                   int agg, float m) {
  openloop_exec_replay(first_tr, exec, n_calls, N, T, A, h, agg, m, [&](int row, int off, int a) {
    const f16* p = chunks + (long)row * ns + (long)off * ld + a;
    if (picks) {
      const int k = picks[row];
      return ens_load(p + (long)(k < 0 ? 0 : (k >= R ? R - 1 : k)) * ss);  // (what the first launch wrote lies in 0 .. R - 1)
    }
    return ens_sample_mean(R, inv_R, [&](int r) { return ens_load(p + (long)r * ss); });
  });
  const long e = (long)blockIdx.x * ENS_THREADS + threadIdx.x;
  if (pick_fill && e < (long)N * A && e % A == 0) pick_fill[e / A] = -1;
}

}  // namespace

extern "C" {

int64_t gn_action_ensemble_state_bytes(int32_t B, int32_t T, int32_t A, int32_t K) {
  if (B <= 0 || T <= 0 || A <= 0 || K <= 0 || K > ENS_MAX_K || (int64_t)T * A > (1 << 24)) return -1;
  return (int64_t)B * ens_row_bytes(T, A, K);
}

int32_t gn_action_ensemble(gn_ctx* ctx, const float* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B, int32_t T,
                           int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  return launch_ensemble(ctx, "gn_action_ensemble", chunk, state, steps, reset, out, B, T, A, ld, K, h, m);
}

int32_t gn_action_ensemble_f16(gn_ctx* ctx, const void* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B, int32_t T,
                               int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  return launch_ensemble(ctx, "gn_action_ensemble_f16", (const f16*)chunk, state, steps, reset, out, B, T, A, ld, K, h, m);
}

int32_t gn_openloop_exec_actions(gn_ctx* ctx, const void* chunks, const int32_t* first_tr, float* exec, int32_t* n_calls, int32_t N, int32_t T,
                                 int32_t A, int32_t ld, int32_t h, int32_t temporal_agg, float m) {
  GN_REQUIRE(ctx && chunks && first_tr && exec, "gn_openloop_exec_actions: null argument");
  GN_REQUIRE(N > 0 && T > 0 && A >= 2 && (int64_t)N * A <= INT32_MAX, "gn_openloop_exec_actions: N (%d), T (%d), A (%d) out of range", N, T, A);
  GN_REQUIRE(ld >= A, "gn_openloop_exec_actions: row pitch ld (%d) < A (%d)", ld, A);
  GN_REQUIRE(h >= 1 && h <= T, "gn_openloop_exec_actions: execution horizon h (%d) must lie in 1 .. T (%d)", h, T);
  GN_REQUIRE(m >= 0.f && m == m, "gn_openloop_exec_actions: m (%g) must be >= 0", (double)m);
  GN_REQUIRE((((uintptr_t)chunks) & 1) == 0 && (((uintptr_t)first_tr | (uintptr_t)exec | (uintptr_t)n_calls) & 3) == 0,
             "gn_openloop_exec_actions: misaligned argument");
  hipLaunchKernelGGL(openloop_exec_actions_kernel, dim3((unsigned)cdiv64((int64_t)N * A, ENS_THREADS)), dim3(ENS_THREADS), 0, ctx->stream, (const f16*)chunks,
                     first_tr, exec, n_calls, N, T, A, ld, h, temporal_agg ? 1 : 0, m);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_action_ensemble_samples_f16(gn_ctx* ctx, const void* chunk, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine, void* state,
                                       const int32_t* steps, const uint8_t* reset, float* out, int32_t* pick_out, float* spread_out, int32_t B, int32_t T,
                                       int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  const char* who = "gn_action_ensemble_samples_f16";
  if (int32_t e = gn_check_action_ensemble_samples(ctx, who, chunk, bs, ss, R, inv_R, combine, state, steps, reset, out, pick_out, spread_out, B, T, A, ld, K,
                                                   h, m))
    return e;
  hipLaunchKernelGGL(action_ensemble_samples_kernel, dim3((unsigned)B), dim3(ENS_THREADS), 0, ctx->stream, (const f16*)chunk, (long)bs, (long)ss, R, inv_R,
                     combine, (char*)state, steps, reset, out, pick_out, spread_out, T, A, ld, K, h, m, (long)ens_row_bytes(T, A, K));
  GN_LAUNCH_CHECK();
  return GN_OK;
}

int32_t gn_openloop_exec_actions_samples(gn_ctx* ctx, const void* chunks, int64_t ns, int64_t ss, int32_t R, float inv_R, int32_t combine,
                                         const int32_t* first_tr, float* exec, int32_t* n_calls, int32_t* pick_out, int32_t N, int32_t T, int32_t A,
                                         int32_t ld, int32_t h, int32_t temporal_agg, float m) {
  const char* who = "gn_openloop_exec_actions_samples";
  GN_REQUIRE(ctx && chunks && first_tr && exec, "%s: null argument", who);
  GN_REQUIRE(N > 0 && T > 0 && A >= 2 && (int64_t)N * A <= INT32_MAX, "%s: N (%d), T (%d), A (%d) out of range", who, N, T, A);
  GN_REQUIRE(ld >= A, "%s: row pitch ld (%d) < A (%d)", who, ld, A);
  GN_REQUIRE(h >= 1 && h <= T, "%s: execution horizon h (%d) must lie in 1 .. T (%d)", who, h, T);
  GN_REQUIRE(m >= 0.f && m == m, "%s: m (%g) must be >= 0", who, (double)m);
  if (int32_t e = check_samples(who, ns, ss, R, inv_R, combine, N, T, A, ld)) return e;
  GN_REQUIRE(!combine || pick_out, "%s: the medoid rule hands its picks from the first launch to the second through pick_out", who);
  GN_REQUIRE((((uintptr_t)chunks) & 1) == 0 && (((uintptr_t)first_tr | (uintptr_t)exec | (uintptr_t)n_calls | (uintptr_t)pick_out) & 3) == 0,
             "%s: misaligned argument", who);
  if (combine) {
    hipLaunchKernelGGL(openloop_sample_picks_kernel, dim3((unsigned)N), dim3(ENS_THREADS), 0, ctx->stream, (const f16*)chunks, (long)ns, (long)ss, R, pick_out,
                       T, A, ld);
    GN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(openloop_exec_actions_samples_kernel, dim3((unsigned)cdiv64((int64_t)N * A, ENS_THREADS)), dim3(ENS_THREADS), 0, ctx->stream,
                     (const f16*)chunks, (long)ns, (long)ss, R, inv_R, combine ? (const int32_t*)pick_out : nullptr, combine ? nullptr : pick_out, first_tr,
                     exec, n_calls, N, T, A, ld, h, temporal_agg ? 1 : 0, m);
  GN_LAUNCH_CHECK();
  return GN_OK;
}

}  // extern "C"

// Every refusal of gn_action_ensemble_samples_f16, without the launch: gn_program_record_action_ensemble_samples (api.hip) asks it at record time.
int32_t gn_check_action_ensemble_samples(gn_ctx* ctx, const char* who, const void* chunk, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine,
                                         const void* state, const int32_t* steps, const uint8_t* reset, const float* out, const int32_t* pick_out,
                                         const float* spread_out, int32_t B, int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  if (int32_t e = check_ensemble(ctx, who, chunk, state, steps, reset, out, B, T, A, ld, K, h, m, sizeof(f16))) return e;
  if (int32_t e = check_samples(who, bs, ss, R, inv_R, combine, B, T, A, ld)) return e;
  GN_REQUIRE((((uintptr_t)pick_out | (uintptr_t)spread_out) & 3) == 0, "%s: misaligned pick_out / spread_out", who);
  return GN_OK;
}
