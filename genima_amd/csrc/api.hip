// C-ABI plumbing of libgenima_hip.so: context, thread-local error string, op programs (record / replay / hipGraph), events.
#include <stdarg.h>
#include <string.h>

#include <functional>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

static thread_local char g_err[1024] = "";

void gn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

// A recorded op is the eager entry point bound to its arguments (Kernel).  The three ops that gn_program_get_gemm / set_* read and rewrite after
// recording keep a typed payload in the Op instead and are dispatched by kind: a closure must not point into gn_program::ops (the vector
// reallocates).  Stream control: ops after Fork go to the program's side stream until Main; Join makes main wait for it.
enum class Kind { Kernel, Gemm, AddMulti, Memset, Fork, Main, Join };

struct AddMultiOp {
  const void* a[GN_ADD_MULTI_MAX]; const void* b[GN_ADD_MULTI_MAX]; void* out[GN_ADD_MULTI_MAX]; int64_t n[GN_ADD_MULTI_MAX]; int32_t count;
  int32_t C[GN_ADD_MULTI_MAX]; gn_stats_sink sink[GN_ADD_MULTI_MAX]; int32_t has_sink;  // GroupNorm bridge (gn_program_set_sink)
};

struct MemsetOp { void* ptr; int64_t bytes; };

struct Op {
  Kind kind;
  const char* name;                         // the gn_ entry point a replay calls (error text)
  std::function<int32_t(gn_ctx*)> launch;   // Kernel
  union { AddMultiOp addm; gn_gemm_desc gemm; MemsetOp ms; };  // AddMulti / Gemm / Memset (the largest first: Op{} zeroes all of it)
};

static Op make_op(Kind kind, const char* name) {
  static_assert(sizeof(AddMultiOp) >= sizeof(gn_gemm_desc) && sizeof(AddMultiOp) >= sizeof(MemsetOp), "the union's first member covers the others");
  Op op{};
  op.kind = kind;
  op.name = name;
  return op;
}

// An array argument, copied into the closure and handed to the entry point as a pointer to the copy: the caller's arrays are temporaries
// (ctypes arrays that die when gn_program_add_* returns).
template <class T, size_t N>
struct Arr {
  T v[N];
  explicit Arr(const T* s) { for (size_t i = 0; i < N; ++i) v[i] = s[i]; }
  operator const T*() const { return v; }
};

// an argument binds to a parameter of exactly its own type (no conversion on the way into the closure or out of it); an Arr to a pointer to its elements
template <class A, class P> constexpr bool binds = std::is_same<A, P>::value;
template <class T, size_t N, class P> constexpr bool binds<Arr<T, N>, P> = std::is_same<const T*, P>::value;

}  // namespace

struct Segment { int64_t first, last; };  // op range [first, last) marked at record time (gn_program_begin_segment / end_segment)
struct CapturedGraph { hipGraph_t graph; hipGraphExec_t exec; int64_t ops; };

struct gn_program {
  gn_ctx* ctx;
  std::vector<Op> ops;
  // guarded segments: a FULL replay skips the kernel ops of a disabled segment (their outputs are still there from the replay that ran them);
  // stream markers always act, and an explicit op range runs exactly what it names
  std::vector<Segment> segs;
  int64_t open_seg = -1;           // op index where the open segment began, or -1
  uint64_t enabled = ~0ull;        // bit s: segment s runs
  int64_t last_run_ops = 0;        // kernel ops the last full replay issued (gn_program_last_run_ops)
  std::map<uint64_t, CapturedGraph> graphs;  // one captured graph per set of enabled flags that was launched
  hipGraphExec_t exec = nullptr;   // non-null once captured (the graph of the flags at gn_program_capture)
  hipStream_t side = nullptr;          // second stream for independent sub-graphs (ControlNet next to the UNet encoder)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

static void drop_graphs(gn_program* p) {
  for (auto& kv : p->graphs) {
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
  }
  p->graphs.clear();
  p->exec = nullptr;
}

// does a full replay skip op i?  (segments do not nest and are recorded in op order)
static bool op_skipped(const gn_program* p, int64_t i) {
  for (size_t s = 0; s < p->segs.size(); ++s)
    if (i >= p->segs[s].first && i < p->segs[s].last) return !((p->enabled >> s) & 1ull);
  return false;
}

static int32_t run_op(gn_ctx* ctx, const Op& op) {
  switch (op.kind) {
    case Kind::Kernel: return op.launch(ctx);
    case Kind::Gemm: return gn_launch_gemm(ctx, &op.gemm);
    case Kind::AddMulti:
      if (op.addm.has_sink) return gn_add_multi_stats(ctx, op.addm.a, op.addm.b, op.addm.out, op.addm.n, op.addm.C, op.addm.sink, op.addm.count);
      return gn_add_multi(ctx, op.addm.a, op.addm.b, op.addm.out, op.addm.n, op.addm.count);
    case Kind::Memset: return gn_memset(ctx, op.ms.ptr, op.ms.bytes);
    default: gn_set_error("gn_program: %s is not a kernel op", op.name); return GN_ERR_INVALID;
  }
}

// every gn_program_add_* ends here: exactly one op appended (stream markers included -- the callers index the list), none when refused
static int32_t push(gn_program* p, const char* who, Op op) {
  GN_REQUIRE(p, "%s: null program", who);
  p->ops.push_back(std::move(op));
  return GN_OK;
}

// record `fn(ctx, args...)`: the arguments are captured by value and checked against fn's own declaration
template <class... P, class... A>
static int32_t record(gn_program* p, const char* who, const char* name, int32_t (*fn)(gn_ctx*, P...), A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "argument count differs from the entry point's");
  static_assert((binds<A, P> && ...), "an argument's type differs from the entry point's parameter");
  Op op = make_op(Kind::Kernel, name);
  op.launch = [fn, args...](gn_ctx* ctx) { return fn(ctx, args...); };
  return push(p, who, std::move(op));
}
// RECORD(gn_X, args...) inside gn_program_add_X(gn_program* p, ...)
#define RECORD(fn, ...) record(p, __func__, #fn, fn, __VA_ARGS__)

// the descriptor ops that nothing patches after recording: the closure owns a copy of *d
template <class D>
static int32_t record_desc(gn_program* p, const char* who, const char* name, int32_t (*fn)(gn_ctx*, const D*), const D* d) {
  GN_REQUIRE(p && d, "%s: null argument", who);
  Op op = make_op(Kind::Kernel, name);
  op.launch = [fn, desc = *d](gn_ctx* ctx) { return fn(ctx, &desc); };
  return push(p, who, std::move(op));
}

extern "C" {

int32_t gn_version(void) { return 101; }  // 101: gn_gemm_desc grew (sink, norm_in, norm_out; round 5) + tile 25, gn_gemm_plan_valid, GN_STATS_SHIFT_SQ (round 6)
const char* gn_last_error(void) { return g_err; }

int32_t gn_ctx_create(int32_t device, void* stream, gn_ctx** out) {
  GN_REQUIRE(out, "gn_ctx_create: null out");
  int n = 0;
  GN_HIP(hipGetDeviceCount(&n));
  GN_REQUIRE(device >= 0 && device < n, "gn_ctx_create: device %d out of range (%d visible)", device, n);
  GN_HIP(hipSetDevice(device));
  if (gn_ppp_pool_init(device) != GN_OK) return GN_ERR_HIP;  // the persistent GEMM's hand-off flags (1 MB, zeroed once; never allocated inside a capture)
  gn_ctx* c = new gn_ctx();
  c->device = device;
  c->stream = (hipStream_t)stream;
  *out = c;
  return GN_OK;
}
int32_t gn_ctx_destroy(gn_ctx* ctx) {
  delete ctx;
  return GN_OK;
}
int32_t gn_ctx_set_stream(gn_ctx* ctx, void* stream) {
  GN_REQUIRE(ctx, "gn_ctx_set_stream: null ctx");
  ctx->stream = (hipStream_t)stream;
  return GN_OK;
}

int32_t gn_gemm(gn_ctx* ctx, const gn_gemm_desc* d) {
  GN_REQUIRE(ctx, "gn_gemm: null ctx");
  return gn_launch_gemm(ctx, d);
}
int32_t gn_attention_fwd(gn_ctx* ctx, const gn_attn_desc* d) {
  GN_REQUIRE(ctx, "gn_attention_fwd: null ctx");
  return gn_launch_attention(ctx, d);
}
int32_t gn_tblock(gn_ctx* ctx, const gn_tblock_desc* d) {
  GN_REQUIRE(ctx, "gn_tblock: null ctx");
  return gn_launch_tblock(ctx, d);
}
int32_t gn_groupnorm_fwd(gn_ctx* ctx, const gn_groupnorm_desc* d) {
  GN_REQUIRE(ctx, "gn_groupnorm_fwd: null ctx");
  return gn_launch_groupnorm(ctx, d);
}

// ---- programs ---------------------------------------------------------------------------------------------------------
int32_t gn_program_create(gn_ctx* ctx, gn_program** out) {
  GN_REQUIRE(ctx && out, "gn_program_create: null argument");
  gn_program* p = new gn_program();
  p->ctx = ctx;
  *out = p;
  return GN_OK;
}
int32_t gn_program_destroy(gn_program* p) {
  if (p) {
    drop_graphs(p);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    if (p->side) (void)hipStreamDestroy(p->side);
    delete p;
  }
  return GN_OK;
}
int32_t gn_program_add_gemm(gn_program* p, const gn_gemm_desc* d) {
  GN_REQUIRE(p && d, "gn_program_add_gemm: null argument");
  Op op = make_op(Kind::Gemm, "gn_gemm");
  op.gemm = *d;
  return push(p, __func__, std::move(op));
}
int32_t gn_program_add_attention(gn_program* p, const gn_attn_desc* d) { return record_desc(p, __func__, "gn_attention_fwd", gn_launch_attention, d); }
int32_t gn_program_add_tblock(gn_program* p, const gn_tblock_desc* d) { return record_desc(p, __func__, "gn_tblock", gn_launch_tblock, d); }
int32_t gn_program_add_conv3x3_gn(gn_program* p, const gn_conv3x3_gn_desc* d) { return record_desc(p, __func__, "gn_conv3x3_gn", gn_conv3x3_gn, d); }
int32_t gn_program_add_conv3x3_patch(gn_program* p, const gn_conv3x3_patch_desc* d) {
  return record_desc(p, __func__, "gn_conv3x3_patch", gn_conv3x3_patch, d);
}
int32_t gn_program_add_groupnorm(gn_program* p, const gn_groupnorm_desc* d) { return record_desc(p, __func__, "gn_groupnorm_fwd", gn_launch_groupnorm, d); }
int32_t gn_program_add_tiny_block(gn_program* p, const void* x, const void* const w[3], const void* const bias[3], void* out, int32_t B,
                                 int32_t H, int32_t W, int32_t C) {
  GN_REQUIRE(w && bias, "gn_program_add_tiny_block: null weight / bias array");
  GN_REQUIRE(x && out && B > 0 && gn_tiny_block_supported(C, H, W), "gn_program_add_tiny_block: null x / out or unsupported shape (B %d, %dx%d, C %d)", B, H,
             W, C);
  return RECORD(gn_tiny_block, x, Arr<const void*, 3>(w), Arr<const void*, 3>(bias), out, B, H, W, C);
}
int32_t gn_program_add_layernorm(gn_program* p, const void* x, const void* gamma, const void* beta, void* y, int64_t M, int32_t C, float eps) {
  return RECORD(gn_layernorm_fwd, x, gamma, beta, y, M, C, eps);
}
int32_t gn_program_add_timestep_embedding(gn_program* p, const float* t, void* out, int32_t B, int32_t dim, int32_t flip, float freq_shift) {
  return RECORD(gn_timestep_embedding, t, out, B, dim, flip, freq_shift);
}
int32_t gn_program_add_scale_pad(gn_program* p, const void* x, void* out, int64_t pixels, int32_t C, int32_t Cpad, float scale) {
  return RECORD(gn_scale_pad, x, out, pixels, C, Cpad, scale);
}
int32_t gn_program_add_scale_cat_pad(gn_program* p, const void* x, const void* x2, void* out, int64_t pixels, int32_t C, int32_t ld1,
                                     int32_t C2, int32_t ld2, int32_t Cpad, float scale, float scale2) {
  return RECORD(gn_scale_cat_pad, x, x2, out, pixels, C, ld1, C2, ld2, Cpad, scale, scale2);
}
int32_t gn_program_add_euler_step(gn_program* p, void* x, const void* eps, int64_t pixels, int32_t C, int32_t ld_eps, float sigma, float sigma_next) {
  return RECORD(gn_euler_step, x, eps, pixels, C, ld_eps, sigma, sigma_next);
}
int32_t gn_program_add_image_f16_to_u8(gn_program* p, const void* in, uint8_t* out, int64_t pixels, int32_t ld) {
  return RECORD(gn_image_f16_to_u8, in, out, pixels, ld);
}
int32_t gn_program_add_image_u8_to_f16(gn_program* p, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad, float mul, float add) {
  return RECORD(gn_image_u8_to_f16, in, out, pixels, Cpad, mul, add);
}
int32_t gn_program_add_add(gn_program* p, const void* a, const void* b, void* out, int64_t n) { return RECORD(gn_add, a, b, out, n); }
int32_t gn_program_add_add_multi(gn_program* p, const void* const* a, const void* const* b, void* const* out, const int64_t* n, int32_t count) {
  GN_REQUIRE(p && a && b && out && n && count >= 1 && count <= GN_ADD_MULTI_MAX, "gn_program_add_add_multi: 1 .. %d tensors", GN_ADD_MULTI_MAX);
  Op op = make_op(Kind::AddMulti, "gn_add_multi");
  for (int i = 0; i < count; ++i) { op.addm.a[i] = a[i]; op.addm.b[i] = b[i]; op.addm.out[i] = out[i]; op.addm.n[i] = n[i]; }
  op.addm.count = count;
  return push(p, __func__, std::move(op));
}
int32_t gn_program_add_film(gn_program* p, const void* x, void* out, const void* gamma, const void* beta, int64_t ld_film,
                            int64_t rows_per_film, int64_t rows, int32_t C, int32_t act) {
  return RECORD(gn_film, x, out, gamma, beta, ld_film, rows_per_film, rows, C, act);
}
int32_t gn_program_add_act(gn_program* p, const void* x, void* out, int64_t n, int32_t act) { return RECORD(gn_act, x, out, n, act); }
int32_t gn_program_add_embedding(gn_program* p, const int32_t* ids, const void* tok, const void* pos, void* out, int32_t B, int32_t L, int32_t D) {
  return RECORD(gn_embedding, ids, tok, pos, out, B, L, D);
}
int32_t gn_program_add_softmax_rows(gn_program* p, void* x, int64_t rows, int32_t cols, int32_t ld, float scale) {
  return RECORD(gn_softmax_rows, x, rows, cols, ld, scale);
}
int32_t gn_program_add_maxpool3x3s2(gn_program* p, const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C) {
  return RECORD(gn_maxpool3x3s2, x, y, B, H, W, C);
}
int32_t gn_program_add_image_normalize_u8(gn_program* p, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad, float m0,
                                          float m1, float m2, float a0, float a1, float a2) {
  return RECORD(gn_image_normalize_u8, in, out, pixels, Cpad, m0, m1, m2, a0, a1, a2);
}
int32_t gn_program_add_gather_rows(gn_program* p, const void* x, const int32_t* idx, void* out, int32_t B, int32_t L, int32_t D) {
  return RECORD(gn_gather_rows, x, idx, out, B, L, D);
}
int32_t gn_program_add_copy4d(gn_program* p, const void* in, void* out, const int64_t* sizes, const int64_t* in_strides,
                              const int64_t* out_strides, int32_t L) {
  GN_REQUIRE(sizes && in_strides && out_strides, "gn_program_add_copy4d: null argument");
  return RECORD(gn_copy4d, in, out, Arr<int64_t, 4>(sizes), Arr<int64_t, 4>(in_strides), Arr<int64_t, 4>(out_strides), L);
}
int32_t gn_program_add_argmax_rows_i32(gn_program* p, const int32_t* x, int32_t* out, int32_t rows, int32_t cols) {
  return RECORD(gn_argmax_rows_i32, x, out, rows, cols);
}
int32_t gn_program_add_add_noise(gn_program* p, const void* x0, const void* noise, const float* sqrt_ac, const float* sqrt_1mac, void* out, int32_t B,
                                 int64_t per_sample) {
  return RECORD(gn_add_noise, x0, noise, sqrt_ac, sqrt_1mac, out, B, per_sample);
}
int32_t gn_program_add_action_ensemble(gn_program* p, const void* chunk, int32_t chunk_f16, void* state, const int32_t* steps, const uint8_t* reset, float* out,
                                       int32_t B, int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  // the arguments that make the launch refuse are refused here, not at the first replay (possibly in the middle of a hipGraph capture)
  GN_REQUIRE(chunk && state && steps && reset && out && B > 0 && T > 0 && A > 0 && ld >= A && h >= 1 && h <= T && (K == 1 || K >= (T + h - 1) / h) && m >= 0.f &&
                 gn_action_ensemble_state_bytes(B, T, A, K) > 0,
             "gn_program_add_action_ensemble: bad arguments (B %d, T %d, A %d, ld %d, K %d, h %d, m %g)", B, T, A, ld, K, h, (double)m);
  if (chunk_f16) return RECORD(gn_action_ensemble_f16, chunk, state, steps, reset, out, B, T, A, ld, K, h, m);
  return RECORD(gn_action_ensemble, (const float*)chunk, state, steps, reset, out, B, T, A, ld, K, h, m);
}
int32_t gn_program_record_action_ensemble_samples(gn_program* p, const void* chunk, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine, void* state,
                                               const int32_t* steps, const uint8_t* reset, float* out, int32_t* pick_out, float* spread_out, int32_t B,
                                               int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m) {
  GN_REQUIRE(p, "%s: null program", __func__);
  // its state advances on every call: a replay that skipped it would execute a stale ring
  GN_REQUIRE(p->open_seg < 0, "%s: recorded inside a guarded segment", __func__);
  // as above: what makes the launch refuse is refused here
  if (int32_t e = gn_check_action_ensemble_samples(p->ctx, __func__, chunk, bs, ss, R, inv_R, combine, state, steps, reset, out, pick_out, spread_out, B, T, A,
                                                   ld, K, h, m))
    return e;
  GN_REQUIRE(gn_action_ensemble_state_bytes(B, T, A, K) > 0, "%s: bad shape (B %d, T %d, A %d, K %d)", __func__, B, T, A, K);
  return RECORD(gn_action_ensemble_samples_f16, chunk, bs, ss, R, inv_R, combine, state, steps, reset, out, pick_out, spread_out, B, T, A, ld, K, h, m);
}
int32_t gn_program_add_fork(gn_program* p) { return push(p, __func__, make_op(Kind::Fork, "fork")); }
int32_t gn_program_add_main(gn_program* p) { return push(p, __func__, make_op(Kind::Main, "main")); }
int32_t gn_program_add_join(gn_program* p) { return push(p, __func__, make_op(Kind::Join, "join")); }
int64_t gn_program_num_ops(const gn_program* p) { return p ? (int64_t)p->ops.size() : 0; }

// in-call tile tuning (genima_amd/incall_tune.py): read back a recorded gn_gemm op, and replace its tile / K split (+ the workspace its
// split-K partial sums use).  A tile never changes the summation order along K; a K split does (as documented on gn_gemm_desc).
int32_t gn_program_get_gemm(const gn_program* p, int64_t op, gn_gemm_desc* out) {
  GN_REQUIRE(p && out && op >= 0 && op < (int64_t)p->ops.size(), "gn_program_get_gemm: bad argument");
  if (p->ops[(size_t)op].kind != Kind::Gemm) return GN_ERR_INVALID;  // (no error text: callers probe every op)
  *out = p->ops[(size_t)op].gemm;
  return GN_OK;
}
int32_t gn_program_set_gemm_plan(gn_program* p, int64_t op, int32_t tile, int32_t splitk, void* workspace) {
  GN_REQUIRE(p && op >= 0 && op < (int64_t)p->ops.size() && p->ops[(size_t)op].kind == Kind::Gemm, "gn_program_set_gemm_plan: op %ld is not a gn_gemm", (long)op);
  GN_REQUIRE(!p->exec, "gn_program_set_gemm_plan: the program is captured (re-capture after tuning)");
  GN_REQUIRE(tile >= 0 && tile <= GN_NUM_GEMM_TILES && splitk >= 0, "gn_program_set_gemm_plan: tile %d (0 = heuristic, 1 .. %d) / splitk %d out of range", tile, GN_NUM_GEMM_TILES, splitk);
  gn_gemm_desc d = p->ops[(size_t)op].gemm;  // validated on a copy: a refused plan leaves the recorded op as it was
  d.tile = tile; d.splitk = splitk;
  if (workspace) d.workspace = workspace;
  GN_REQUIRE(gn_gemm_workspace_bytes(&d) == 0 || d.workspace, "gn_program_set_gemm_plan: this plan splits K and needs a workspace");
  // the fusions attached to the op must survive the new plan (gn_launch_gemm would refuse it at replay, possibly in the middle of a hipGraph capture):
  // norm_out lives in the split-K reduce, norm_in in the ring tiles, the plan must name the tile that will run
  if (!gn_gemm_plan_valid(&d)) {
    char why[600];
    snprintf(why, sizeof(why), "%s", g_err);  // (gn_set_error formats into g_err itself)
    gn_set_error("gn_program_set_gemm_plan: tile %d / splitk %d refused for op %ld: %s", tile, splitk, (long)op, why);
    return GN_ERR_INVALID;
  }
  p->ops[(size_t)op].gemm = d;
  return GN_OK;
}

int32_t gn_program_set_sink(gn_program* p, int64_t op, int32_t index, const gn_stats_sink* sink, int32_t channels) {
  GN_REQUIRE(p && sink && op >= 0 && op < (int64_t)p->ops.size(), "gn_program_set_sink: bad argument");
  GN_REQUIRE(!p->exec, "gn_program_set_sink: the program is captured");
  Op& o = p->ops[(size_t)op];
  if (o.kind == Kind::Gemm) {
    GN_REQUIRE(index == 0 && !o.gemm.sink.stats, "gn_program_set_sink: a gn_gemm op has one output and takes one sink");
    GN_REQUIRE(o.gemm.out_mode == GN_OUT_ROWMAJOR && !o.gemm.out2 && o.gemm.act != GN_ACT_GEGLU && !o.gemm.fp8 && (o.gemm.batch <= 1 || o.gemm.up_phases),
               "gn_program_set_sink: this gn_gemm does not write a plain row-major f16 tensor");
    o.gemm.sink = *sink;
    return GN_OK;
  }
  if (o.kind == Kind::AddMulti) {
    GN_REQUIRE(index >= 0 && index < o.addm.count && !o.addm.sink[index].stats && channels > 0 && channels % 8 == 0 && o.addm.n[index] % channels == 0,
               "gn_program_set_sink: bad gn_add_multi tensor index / channel count");
    for (int i = 0; i < o.addm.count; ++i)
      if (o.addm.C[i] == 0) o.addm.C[i] = 8;  // tensors without a sink: any row shape
    o.addm.C[index] = channels;
    o.addm.sink[index] = *sink;
    o.addm.has_sink = 1;
    return GN_OK;
  }
  gn_set_error("gn_program_set_sink: op %ld is neither a gn_gemm nor a gn_add_multi", (long)op);
  return GN_ERR_INVALID;
}
int32_t gn_program_set_norm_out(gn_program* p, int64_t op, const gn_norm_out* n) {
  GN_REQUIRE(p && n && n->y && op >= 0 && op < (int64_t)p->ops.size() && p->ops[(size_t)op].kind == Kind::Gemm, "gn_program_set_norm_out: op %ld is not a gn_gemm", (long)op);
  GN_REQUIRE(!p->exec, "gn_program_set_norm_out: the program is captured");
  gn_gemm_desc d = p->ops[(size_t)op].gemm;
  GN_REQUIRE(!d.norm_out.y, "gn_program_set_norm_out: this gn_gemm already normalises its output");
  d.norm_out = *n;
  GN_REQUIRE(gn_gemm_norm_out_supported(&d), "gn_program_set_norm_out: the recorded problem / plan does not take norm_out");
  p->ops[(size_t)op].gemm = d;
  return GN_OK;
}
int32_t gn_program_set_memset_bytes(gn_program* p, int64_t op, int64_t bytes) {
  GN_REQUIRE(p && op >= 0 && op < (int64_t)p->ops.size() && p->ops[(size_t)op].kind == Kind::Memset && bytes > 0 && bytes <= p->ops[(size_t)op].ms.bytes,
             "gn_program_set_memset_bytes: op %ld is not a memset of at least %ld bytes", (long)op, (long)bytes);
  GN_REQUIRE(!p->exec, "gn_program_set_memset_bytes: the program is captured");
  p->ops[(size_t)op].ms.bytes = bytes;
  return GN_OK;
}
int64_t gn_desc_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(gn_gemm_desc);
    case 1: return (int64_t)sizeof(gn_attn_desc);
    case 2: return (int64_t)sizeof(gn_groupnorm_desc);
    case 3: return (int64_t)sizeof(gn_tblock_desc);
    case 4: return (int64_t)sizeof(gn_conv3x3_gn_desc);
    case 5: return (int64_t)sizeof(gn_stats_sink);
    case 6: return (int64_t)sizeof(gn_norm_in);
    case 7: return (int64_t)sizeof(gn_norm_out);
    case 8: return (int64_t)sizeof(gn_conv3x3_patch_desc);
    case 9: return (int64_t)sizeof(gn_replay_gather_desc);
    case 10: return (int64_t)sizeof(gn_replay_render_desc);
    default: return -1;
  }
}
int32_t gn_program_add_memset(gn_program* p, void* ptr, int64_t bytes) {
  GN_REQUIRE(ptr && bytes > 0, "gn_program_add_memset: null / empty");
  Op op = make_op(Kind::Memset, "gn_memset");
  op.ms.ptr = ptr;
  op.ms.bytes = bytes;
  return push(p, __func__, std::move(op));
}

static uint64_t seg_mask(const gn_program* p) { return p->segs.size() >= 64 ? ~0ull : ((1ull << p->segs.size()) - 1ull); }

static int32_t ensure_side_stream(gn_program* p) {
  if (!p->side) {
    GN_HIP(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
    GN_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    GN_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
  }
  return GN_OK;
}

int32_t gn_program_run(gn_program* p, int64_t first, int64_t last) {
  GN_REQUIRE(p, "gn_program_run: null program");
  const int64_t n = (int64_t)p->ops.size();
  const bool full = first == 0 && last < 0;  // the whole program by default: honours the segment flags; an explicit range does not
  if (last < 0 || last > n) last = n;
  GN_REQUIRE(first >= 0 && first <= last, "gn_program_run: bad range [%ld, %ld)", (long)first, (long)last);
  GN_REQUIRE(p->open_seg < 0, "gn_program_run: a segment is still open (gn_program_end_segment)");
  const bool guarded = full && !p->segs.empty() && (p->enabled & seg_mask(p)) != seg_mask(p);
  int64_t issued = 0;
  // stream-control ops only act on whole-program replays; a sub-range (per-op timing) runs serially on the context's stream
  const bool two_streams = first == 0 && last == n;
  hipStream_t main_stream = p->ctx->stream;
  bool forked = false;  // side stream has work the main stream has not waited for
  int32_t rc = GN_OK;
  for (int64_t i = first; i < last && rc == GN_OK; ++i) {
    const Op& op = p->ops[(size_t)i];
    if (op.kind == Kind::Fork || op.kind == Kind::Main || op.kind == Kind::Join) {
      if (!two_streams) continue;
      if (op.kind == Kind::Fork) {
        if (guarded) {
          // a side section whose every kernel is skipped is not opened: an empty branch would hand the next join the same predecessors twice
          // (the join in front of it already ordered the side stream's work), and there is nothing to overlap
          bool any = false;
          for (int64_t j = i + 1; j < last && !any; ++j) {
            const Kind t = p->ops[(size_t)j].kind;
            if (t == Kind::Fork || t == Kind::Main || t == Kind::Join) break;
            any = !op_skipped(p, j);
          }
          if (!any) continue;
        }
        rc = ensure_side_stream(p);
        if (rc != GN_OK) break;
        if (hipEventRecord(p->ev_fork, main_stream) != hipSuccess || hipStreamWaitEvent(p->side, p->ev_fork, 0) != hipSuccess) {
          gn_set_error("gn_program_run: fork failed"); rc = GN_ERR_HIP; break;
        }
        p->ctx->stream = p->side;
        forked = true;
      } else if (op.kind == Kind::Main) {
        p->ctx->stream = main_stream;
      } else if (forked) {
        p->ctx->stream = main_stream;
        if (hipEventRecord(p->ev_join, p->side) != hipSuccess || hipStreamWaitEvent(main_stream, p->ev_join, 0) != hipSuccess) {
          gn_set_error("gn_program_run: join failed"); rc = GN_ERR_HIP; break;
        }
        forked = false;
      }
      continue;
    }
    if (guarded && op_skipped(p, i)) continue;
    rc = run_op(p->ctx, op);
    ++issued;
    if (rc != GN_OK) {
      char tmp[900];
      snprintf(tmp, sizeof(tmp), "%s", g_err);
      gn_set_error("op %ld (%s): %s", (long)i, op.name, tmp);
    }
  }
  p->ctx->stream = main_stream;
  if (forked) {  // never leave the side stream dangling (also required to end a stream capture)
    (void)hipEventRecord(p->ev_join, p->side);
    (void)hipStreamWaitEvent(main_stream, p->ev_join, 0);
  }
  if (full) p->last_run_ops = issued;
  return rc;
}

// capture the whole program under the current segment flags into the graph cache
static int32_t capture_current(gn_program* p, CapturedGraph** out) {
  GN_REQUIRE(p->ctx->stream != nullptr, "gn_program_capture: needs a non-default stream");
  GN_HIP(hipStreamBeginCapture(p->ctx->stream, hipStreamCaptureModeThreadLocal));
  int32_t rc = gn_program_run(p, 0, -1);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(p->ctx->stream, &g);
  if (rc != GN_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) { gn_set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e)); return GN_ERR_HIP; }
  hipGraphExec_t x = nullptr;
  e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); gn_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e)); return GN_ERR_HIP; }
  CapturedGraph& c = p->graphs[p->enabled & seg_mask(p)];
  c.graph = g; c.exec = x; c.ops = p->last_run_ops;
  *out = &c;
  return GN_OK;
}

int32_t gn_program_capture(gn_program* p) {
  GN_REQUIRE(p, "gn_program_capture: null program");
  drop_graphs(p);  // a re-capture (after gn_program_set_gemm_plan and its like) forgets the graph of every set of flags
  CapturedGraph* c = nullptr;
  int32_t rc = capture_current(p, &c);
  if (rc != GN_OK) return rc;
  p->exec = c->exec;
  return GN_OK;
}

int32_t gn_program_launch(gn_program* p) {
  GN_REQUIRE(p && p->exec, "gn_program_launch: program not captured");
  // one graph per set of enabled flags, captured the first time that set is launched (in practice two: everything, and the steady state)
  auto it = p->graphs.find(p->enabled & seg_mask(p));
  CapturedGraph* c = it != p->graphs.end() ? &it->second : nullptr;
  if (!c) {
    int32_t rc = capture_current(p, &c);
    if (rc != GN_OK) return rc;
  }
  GN_HIP(hipGraphLaunch(c->exec, p->ctx->stream));
  p->last_run_ops = c->ops;
  return GN_OK;
}

// ---- guarded segments ------------------------------------------------------------------------------------------------
int32_t gn_program_begin_segment(gn_program* p, int32_t* seg_id) {
  GN_REQUIRE(p && seg_id, "gn_program_begin_segment: null argument");
  GN_REQUIRE(p->open_seg < 0, "gn_program_begin_segment: segments do not nest");
  GN_REQUIRE(!p->exec, "gn_program_begin_segment: the program is captured");
  GN_REQUIRE(p->segs.size() < 64, "gn_program_begin_segment: at most 64 segments per program");
  p->open_seg = (int64_t)p->ops.size();
  *seg_id = (int32_t)p->segs.size();
  return GN_OK;
}
int32_t gn_program_end_segment(gn_program* p) {
  GN_REQUIRE(p && p->open_seg >= 0, "gn_program_end_segment: no open segment");
  p->segs.push_back(Segment{p->open_seg, (int64_t)p->ops.size()});
  p->open_seg = -1;
  return GN_OK;
}
int32_t gn_program_set_segment_enabled(gn_program* p, int32_t seg_id, int32_t enabled) {
  GN_REQUIRE(p && seg_id >= 0 && seg_id < (int32_t)p->segs.size(), "gn_program_set_segment_enabled: no segment %d", seg_id);
  if (enabled) p->enabled |= 1ull << seg_id;
  else p->enabled &= ~(1ull << seg_id);
  return GN_OK;
}
int64_t gn_program_last_run_ops(const gn_program* p) { return p ? p->last_run_ops : 0; }

// ---- events ----------------------------------------------------------------------------------------------------------
int32_t gn_event_create(void** ev) {
  GN_REQUIRE(ev, "gn_event_create: null");
  hipEvent_t e;
  GN_HIP(hipEventCreate(&e));
  *ev = (void*)e;
  return GN_OK;
}
int32_t gn_event_destroy(void* ev) {
  if (ev) GN_HIP(hipEventDestroy((hipEvent_t)ev));
  return GN_OK;
}
int32_t gn_event_record(gn_ctx* ctx, void* ev) {
  GN_REQUIRE(ctx && ev, "gn_event_record: null");
  GN_HIP(hipEventRecord((hipEvent_t)ev, ctx->stream));
  return GN_OK;
}
int32_t gn_event_elapsed_ms(void* start, void* stop, float* ms) {
  GN_REQUIRE(start && stop && ms, "gn_event_elapsed_ms: null");
  GN_HIP(hipEventSynchronize((hipEvent_t)stop));
  GN_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return GN_OK;
}
int32_t gn_stream_synchronize(gn_ctx* ctx) {
  GN_REQUIRE(ctx, "gn_stream_synchronize: null ctx");
  GN_HIP(hipStreamSynchronize(ctx->stream));
  return GN_OK;
}

}  // extern "C"
