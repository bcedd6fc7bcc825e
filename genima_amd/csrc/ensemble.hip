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
#include "common.h"

namespace {

constexpr int32_t ENS_MAGIC = 0x454E5331;  // "ENS1"
constexpr int ENS_THREADS = 256;
constexpr int ENS_MAX_K = 1024;  // start[] of a row in LDS

__host__ __device__ inline int64_t ens_row_bytes(int64_t T, int64_t A, int64_t K) { return (4 * (K * T * A + K + 2) + 15) / 16 * 16; }

__device__ __forceinline__ float ens_load(const float* p) { return *p; }
__device__ __forceinline__ float ens_load(const f16* p) { return (float)*p; }

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
    float num = 0.f, den = 0.f;
    int i = 0;  // rank among the slots that cover s, oldest first: the ring order from the slot behind w round to w is the order of insertion
    for (int j = 1; j <= K; ++j) {
      const int k = (w + j) % K;
      const int st = s_start[k];
      const long off = s - st;
      if (st < 0 || off < 0 || off >= T) continue;
      const float v = k == w ? ens_load(ck + off * ld + a) : ring[((long)k * T + off) * A + a];
      const float wt = i == 0 ? 1.0f : expf(-m * (float)i);
      num += wt * v;
      den += wt;
      ++i;
    }
    out[((long)b * h + so) * A + a] = num / den;  // the new chunk covers every target step (h <= T): den >= its weight > 0
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

}  // extern "C"
