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
constexpr int ENS_THREADS = 256;
constexpr int ENS_MAX_K = 1024;  // start[] of a row in LDS

__host__ __device__ inline int64_t ens_row_bytes(int64_t T, int64_t A, int64_t K) { return (4 * (K * T * A + K + 2) + 15) / 16 * 16; }

template <typename TC>
__global__ __launch_bounds__(ENS_THREADS) void action_ensemble_kernel(const TC* __restrict__ chunk, char* __restrict__ state,
                                                                     const int32_t* __restrict__ steps, const uint8_t* __restrict__ reset,
                                                                     float* __restrict__ out, int T, int A, int ld, int K, int h, float m,
                                                                     long row_bytes) {
  __shared__ int32_t s_start[ENS_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x;
  char* row = state + (long)b * row_bytes;
  float* ring = (float*)row;
  int32_t* start = (int32_t*)(row + 4l * K * T * A);
  const TC* ck = chunk + (long)b * T * ld;
  const int t = steps[b];
  const bool fresh = reset[b] != 0 || start[K + 1] != ENS_MAGIC;
  const int w = fresh ? 0 : (int)((uint32_t)start[K] % (uint32_t)K);  // the slot the new chunk replaces (modulo: a damaged head stays in bounds)
  for (int k = tid; k < K; k += ENS_THREADS) s_start[k] = k == w ? t : (fresh ? -1 : start[k]);
  __syncthreads();  // every thread has read the old bookkeeping
  for (int k = tid; k < K; k += ENS_THREADS) start[k] = s_start[k];
  if (tid == 0) {
    start[K] = (w + 1) % K;
    start[K + 1] = ENS_MAGIC;
  }
  float* mine = ring + (long)w * T * A;
  for (int e = tid; e < T * A; e += ENS_THREADS) mine[e] = ens_load(ck + (long)(e / A) * ld + e % A);
  for (int e = tid; e < h * A; e += ENS_THREADS) {
    const int so = e / A, a = e % A;
    const long s = (long)t + so;
    // rank among the slots that cover s, oldest first: the ring order from the slot behind w round to w is the order of insertion
    const float mean = ens_weighted_mean(K, m, nullptr, [&](int j, float& v) {
      const int k = (w + j + 1) % K;
      const int st = s_start[k];
      const long off = s - st;
      if (st < 0 || off < 0 || off >= T) return false;
      v = k == w ? ens_load(ck + off * ld + a) : ring[((long)k * T + off) * A + a];
      return true;
    });
    out[((long)b * h + so) * A + a] = mean;  // the new chunk covers every target step (h <= T): den >= its weight > 0
  }
}

template <typename TC>
int32_t launch_ensemble(gn_ctx* ctx, const char* who, const TC* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B,
                        int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  GN_REQUIRE(ctx && chunk && state && steps && reset && out, "%s: null argument", who);
  GN_REQUIRE(B > 0 && T > 0 && A > 0 && (int64_t)T * A <= (1 << 24) && (int64_t)B * T * ld <= INT32_MAX, "%s: B (%d), T (%d), A (%d) out of range", who, B, T, A);
  GN_REQUIRE(ld >= A, "%s: row pitch ld (%d) < A (%d)", who, ld, A);
  GN_REQUIRE(h >= 1 && h <= T, "%s: execution horizon h (%d) must lie in 1 .. T (%d)", who, h, T);
  GN_REQUIRE((K == 1 || K >= (T + h - 1) / h) && K <= ENS_MAX_K, "%s: K (%d) must be 1 (the new chunk alone) or lie in ceil(T / h) = %d .. %d", who, K,
             (T + h - 1) / h, ENS_MAX_K);
  GN_REQUIRE(m >= 0.f && m == m, "%s: m (%g) must be >= 0", who, (double)m);
  GN_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)steps & 3) == 0 && ((uintptr_t)chunk & (sizeof(TC) - 1)) == 0,
             "%s: misaligned pointer (state: 16 bytes)", who);
  hipLaunchKernelGGL(action_ensemble_kernel<TC>, dim3((unsigned)B), dim3(ENS_THREADS), 0, ctx->stream, chunk, (char*)state, steps, reset, out, T, A, ld, K,
                     h, m, (long)ens_row_bytes(T, A, K));
  GN_LAUNCH_CHECK();
  return GN_OK;
}

// The ensemble rule replayed over an evaluation's table of chunks (include/genima_hip.h, gn_openloop_exec_actions).  One thread per (transition n,
// action dimension a); plain loads and stores, a thread writes exec[n][a] alone (and n_calls[n] where a == 0) and reads rows f .. n of `chunks`
// only: f is clamped into [0, n], u <= t <= s = n - f, and the offset s - u = s % h + (jmax - j) h <= T - 1 by the choice of jmax.
__global__ __launch_bounds__(ENS_THREADS) void openloop_exec_actions_kernel(const f16* __restrict__ chunks, const int32_t* __restrict__ first_tr,
                                                                           float* __restrict__ exec, int32_t* __restrict__ n_calls, int N, int T, int A,
                                                                           int ld, int h, int agg, float m) {
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
    v = ens_load(chunks + ((long)(f + u) * T + (s - u)) * ld + a);
    return true;
  });
  exec[e] = mean;  // the call at t itself always takes part
  if (n_calls && a == 0) n_calls[n] = used;
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

}  // extern "C"
