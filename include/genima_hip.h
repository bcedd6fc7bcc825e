/*
 * genima_hip.h -- C ABI of libgenima_hip.so: the MI355X (gfx950 / CDNA4) kernels under the Genima hot path.
 *
 * The reference (MohitShridhar/genima) has no FFI of its own: its device arithmetic is reached through
 * Python seams.  This header is the boundary the build puts *underneath* those seams; each entry
 * point cites the reference call site whose third-party device op it replaces.  Conventions (binding):
 *   - extern "C", plain C types only; no C++ exceptions cross the boundary.
 *   - every function returns int32_t status: 0 = ok, negative = error (gn_last_error() has the thread-local message).
 *   - the caller owns ALL device memory (weights, activations, workspaces) and passes raw device pointers + shapes;
 *     the library never allocates device memory.  *_workspace_bytes() queries precede ops that need scratch.
 *   - functions enqueue on the gn_ctx's stream and never synchronise (asynchronous w.r.t. the host).
 *   - activations are NHWC ("[B, H*W, C]" row-major == the token layout of the transformer blocks); f16 storage with
 *     f32 accumulation (the reference runs torch_dtype=float16: controller/agent/sd_controlnet_agent.py:34,40).
 *   - weights are packed [Cout][KH*KW*Cin] (tap-major, channel-minor; K contiguous) by the host (genima_amd/packing.py).
 */
#ifndef GENIMA_HIP_H
#define GENIMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_OK 0
#define GN_ERR_INVALID (-1)      /* bad argument / unsupported shape */
#define GN_ERR_HIP (-2)          /* a HIP runtime call failed */
#define GN_ERR_UNSUPPORTED (-3)

/* epilogue activations */
enum { GN_ACT_NONE = 0, GN_ACT_SILU = 1, GN_ACT_GELU = 2, GN_ACT_QUICK_GELU = 3, GN_ACT_RELU = 4, GN_ACT_GEGLU = 5,
       GN_ACT_TANH3 = 6 /* 3*tanh(x/3): AutoencoderTiny's latent clamp (controller/agent/sd_controlnet_agent.py:45-49); gn_act only */ };
/* output modes of the GEMM epilogue */
enum { GN_OUT_ROWMAJOR = 0, GN_OUT_BATCH_TRANSPOSED = 1, GN_OUT_F32 = 2 /* row-major float output, ldo in floats */ };

typedef struct gn_ctx gn_ctx;
typedef struct gn_program gn_program;

/* ---- context ------------------------------------------------------------------------------------------------ */
int32_t gn_version(void);
const char* gn_last_error(void);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the default stream. */
int32_t gn_ctx_create(int32_t device, void* stream, gn_ctx** out);
int32_t gn_ctx_destroy(gn_ctx* ctx);
int32_t gn_ctx_set_stream(gn_ctx* ctx, void* stream);

/* ---- K1/K3/K6/K7/K8: MFMA implicit-GEMM convolution and Linear (one kernel family) --------------------------------
 * out[m, n] = epilogue( sum_k A[m, k] * W[n, k] )            M = B*Ho*Wo (conv) or rows (linear), K = KH*KW*(C1+C2)
 * Replaces the cuDNN conv / cuBLAS GEMM calls reached from `self.pipe(...)` (controller/agent/sd_controlnet_agent.py:67-76)
 * and `controlnet(...)` / `unet(...)` / `vae.encode` / `text_encoder` (diffusion/train_controlnet_genima.py:1324-1388).
 * Epilogue order:  v = acc + bias[n] + shift[m / rows_per_batch, n];  v = act(v);  v *= out_scale;  v += residual[m, n].
 * GN_ACT_GEGLU: W rows are packed in alternating 32-row blocks [hidden | gate]; out[m, j] = hidden * gelu(gate), out has N/2 cols.
 */
/* ---- the GroupNorm bridge (round 5): statistics out of the PRODUCER, GroupNorm-apply (+ SiLU) inside the CONSUMER ---------------------------
 * diffusers ResnetBlock2D runs  conv -> GroupNorm -> SiLU -> conv  and Transformer2DModel  conv -> GroupNorm -> proj_in  (inside `self.pipe(...)`,
 * controller/agent/sd_controlnet_agent.py:67-76): as separate launches every GroupNorm is a dependent pass over the tensor between two GEMMs.
 * Here the op that WRITES the tensor also adds its per-(sample, group) sum and sum of squares -- of the f16 values it stored -- into a
 * caller-zeroed statistics block (gn_stats_sink), and the op that READS it normalises its A operand on the way into the MFMA (gn_norm_in), or a
 * single coalesced apply pass does (gn_groupnorm_desc.stats_in).  Sums are fixed point (sum * 2^GN_STATS_SHIFT, sum of squares * 2^GN_STATS_SHIFT_SQ,
 * int64, device-scope integer atomics): integer addition is order-independent, so the statistics -- and everything downstream -- are
 * bit-reproducible run to run.  The second word's coarser scale is range: a slab's sum of squares may reach 2.2e15 before the word wraps. */
#define GN_STATS_SHIFT 24
#define GN_STATS_SHIFT_SQ 12
/* The statistics block: int64 [replicas][samples][groups][GN_STATS_LINE] -- one 128-byte line per (replica, sample, group) holding
 * (sum * 2^GN_STATS_SHIFT, sum of squares * 2^GN_STATS_SHIFT_SQ) in its first two words, ZEROED by the caller before the producers run.  Device-scope atomics
 * serialise per memory line (measured on MI355X: ~100 ns each; 2 240 adds onto the 8 lines of a packed 1 x 32 x 2 block cost a 28 us conv
 * another 30 us), hence a line per group, and `replicas` > 1 where few samples leave few lines: a producer workgroup adds into replica
 * (its row-tile index % replicas), the consumer sums the replicas (integer adds: any order, same bits). */
#define GN_STATS_LINE 16
typedef struct gn_stats_sink {
  void* stats;             /* the statistics block; NULL = off */
  int32_t cpg;             /* channels per group of the consuming GroupNorm */
  int32_t coff;            /* channel, in the consumer's (possibly concatenated) input, of this tensor's channel 0 */
  int32_t groups;          /* groups of the consuming GroupNorm */
  int32_t rows_per_sample; /* output rows (pixels) per sample */
  int32_t samples;         /* samples (the block's second extent) */
  int32_t replicas;        /* >= 1 */
} gn_stats_sink;
typedef struct gn_norm_in {
  const void* stats;       /* the statistics block the producers of the input filled (complete when this op starts); NULL = off */
  const void* gamma;       /* f16 [C] over the (concatenated) input channels */
  const void* beta;
  float eps;
  int32_t groups, cpg;
  int32_t act;             /* GN_ACT_NONE or GN_ACT_SILU applied after the affine */
  int32_t rows_per_sample; /* INPUT pixels (conv) / rows (dense) per sample */
  int32_t samples, replicas; /* extents of the statistics block */
} gn_norm_in;

/* GroupNorm fused into a split-K launch's REDUCE (round 5): the small-M convs of the 8x8 .. 32x32 latent levels split K and finish in a reduce
 * kernel anyway; with norm_out set that kernel owns one (sample, group) slab per workgroup -- it sums the partial slabs, applies the epilogue,
 * stores the raw f16 tensor to `out` as usual AND GroupNorm(+ SiLU) of it to `y`: diffusers ResnetBlock2D's conv1 -> norm2 -> SiLU and
 * conv2 -> next block's norm1 / Transformer2DModel.norm without the GroupNorm launch.  Row-major f16 output, rows_per_batch rows per sample,
 * N % groups == 0, an even group width, a slab (rows_per_batch x N / groups f16) of at most 96 KB; ignored (error) when the plan does not split K
 * (gn_gemm_workspace_bytes() == 0). */
typedef struct gn_norm_out {
  void* y;                 /* [M, N] f16 normalised output (row stride N); NULL = off */
  const void* gamma;       /* f16 [N] */
  const void* beta;
  float eps;
  int32_t groups;
  int32_t act;             /* GN_ACT_NONE or GN_ACT_SILU */
  int32_t rows_per_sample;
} gn_norm_out;

typedef struct gn_gemm_desc {
  const void* a;          /* A source 1: dense [M, lda] or NHWC [B, H, W, C1] */
  const void* a2;         /* conv only: second NHWC source [B, H, W, C2], virtually concatenated on channels; or NULL */
  const void* w;          /* [N, ldw] f16, K contiguous */
  const void* bias;       /* [N] f16 or NULL */
  const void* shift;      /* [M / rows_per_batch, ldshift] f16 or NULL (time-embedding shift, K3) */
  const void* residual;   /* [M, ldr] f16 or NULL */
  void* out;              /* f16 */
  void* workspace;        /* f32 split-K scratch (gn_gemm_workspace_bytes) or NULL when splitk <= 1 */
  int64_t M, N, K;
  int64_t lda, ldw, ldr, ldo;
  int64_t ldshift;        /* row stride of shift (0 = N) */
  int32_t conv;           /* 0 = dense A, 1 = implicit-GEMM gather */
  int32_t B, H, W, C1, C2;         /* conv: source tensor dims (before the optional nearest-2x upsample) */
  int32_t KH, KW, stride, pad_t, pad_l, Ho, Wo;
  int32_t upsample2x;     /* conv: 1 = input is nearest-upsampled 2x on the fly (K8) */
  int32_t act;            /* GN_ACT_* */
  int32_t out_mode;       /* GN_OUT_*; BATCH_TRANSPOSED: out[b][n][m - b*rows_per_batch], row stride ldo, batch stride N*ldo */
  int32_t rows_per_batch; /* for shift / transposed output; 0 = M */
  int32_t splitk;         /* 0 = library heuristic, >=1 explicit */
  int32_t tile;           /* 0 = library heuristic; 1..6 = {256x128, 128x128, 128x64, 64x64, 256x64, 128x256} register-staged block tile,
                             7..14 = {256x256, 256x128, 128x128, 128x64, 64x64, 256x64, 128x320, 256x320} LDS-DMA block tile,
                             15 = 256x256 ping-pong (8-phase, counted vmcnt; K % 64 == 0, conv C1/C2 % 64 == 0, no GEGLU / batch),
                             16..22 = {128x128, 128x64, 64x64, 256x64, 128x160, 64x160, 64x320} with a 3-stage LDS-DMA ring (two K tiles
                             in flight, counted vmcnt); 20..22 are the exact-fit tiles of the N = 640 / 1280 / 320 launches,
                             23 = 128x160 two-stage LDS-DMA, 24 = 128x320 two-stage LDS-DMA on eight waves of 32x160,
                             25 = PERSISTENT ping-pong 256x256 (round 6, csrc/gemm_ppp.hip): one workgroup per CU walks the tile list, the next
                             tile's LDS ring is requested before the finished tile's epilogue, the last partial round is split along K; needs
                             >= one 256x256 tile per CU, a row-major f16 output with N, ldo % 8 == 0, no split-K / out2 / shift + residual
                             together, ln_c1 and GEGLU only together (else tile 15 runs), and, where gn_gemm_workspace_bytes() is not 0, a
                             workspace of that size for the f32 hand-off slabs of the tiles several workgroups share
                             (the host autotunes this per shape: genima_amd/engine.py) */
  int32_t residual_before_act; /* 1: v = act(acc + bias + shift + residual) (ResNet basic block); 0: residual added last */
  float out_scale;        /* 1.0f = none */
  /* batched GEMM (attention backward, per-sample products): `batch` independent problems of the same shape; problem z uses
   * operand + (z / batch_inner) * *_bs + (z % batch_inner) * *_bs2 (strides in elements of that operand; batch_inner >= 1).
   * batch <= 1 = a single problem.  Split-K is disabled when batch > 1. */
  int32_t batch, batch_inner;
  int64_t a_bs, a_bs2, w_bs, w_bs2, out_bs, out_bs2, res_bs, res_bs2;
  int32_t accumulate;     /* GN_OUT_F32 only: out += result (gradient accumulation) */
  /* fp8 Linear (SURVEY section 8 a15 / BASELINE configs[4] "fp8 MFMA"; the reference side is the fp16 autocast Linear of
   * diffusion/train_controlnet_sdxl_genima.py:1448-1471): 1 = a and w hold OCP e4m3 bytes (K contiguous; K, lda, ldw count bytes
   * and are multiples of 16), out = epilogue(scale_a[m] * scale_w[n] * sum_k a*w) on v_mfma_scale_f32_32x32x64_f8f6f4.
   * gn_quantize_fp8_rows produces the bytes and the per-row scales of both operands.  Dense row-major only. */
  int32_t fp8;
  const void* scale_a;    /* fp8: f32 [M] */
  const void* scale_w;    /* fp8: f32 [N], 16-byte aligned */
  /* two-destination output: the q | k | v projections of a self-attention block as ONE launch (diffusers Attention.to_q / to_k /
   * to_v, three cuBLAS calls in the reference: SURVEY.md K7).  Columns [0, split_n) go to `out` (row-major, ldo) as usual; columns
   * [split_n, N) go to `out2` batch-transposed: out2[b][n - split_n][m - b * rows_per_batch], row stride ldo2 -- the V^T layout
   * gn_attention_fwd reads.  split_n % 32 == 0; GN_OUT_ROWMAJOR, no GEGLU / batch / fp8; K is never split.  NULL = off. */
  void* out2;
  int64_t ldo2;
  int32_t split_n;
  /* LayerNorm folded into the Linear that consumes it (diffusers BasicTransformerBlock.norm1 -> attn1.to_q/k/v, norm2 -> attn2.to_q,
   * norm3 -> ff.net[0].proj; CLIPEncoderLayer.layer_norm1/2 -> q/k/v, fc1: a LayerNorm kernel + a cuBLAS call each in the reference).
   * `a` holds the RAW rows; `w` the gamma-scaled weight W'[n, k] = W[n, k] * gamma[k] (f16); `ln_c1` f32 [N] = sum_k W'[n, k] over the
   * f16-rounded W'; `bias` holds c2[n] = sum_k W[n, k] * beta[k] + b[n].  The kernel takes each row's mean / rstd (biased variance,
   * ln_eps) from the A fragments of its K loop and emits rstd * (a . W'^T - mean * c1) + c2 through the usual epilogue (activation,
   * GEGLU, residual, out2 ...).  Dense f16 Linears on the LDS-DMA tiles (7..14, 16..23); K is never split.  NULL = off. */
  float ln_eps;
  const float* ln_c1;
  /* two-level output row pitch (row-major f16 outputs): row m is written at (m / out_row_width) * ldo_hi + (m % out_row_width) * ldo
   * elements from `out`.  One PHASE of a nearest-2x upsampling conv (diffusers Upsample2D: F.interpolate(scale 2, "nearest") + a 3x3
   * conv -- the UNet's up_blocks.*.upsamplers.0 and the VAE decoder's) is a 2x2 conv over the SOURCE pixels whose
   * results land on every other pixel of every other row of the output: out_row_width = W, ldo = 2 * C, ldo_hi = 4 * W * C,
   * out = base + (dy * 2 * W + dx) * C.  0 = off (row m at m * ldo). */
  int32_t out_row_width;
  int64_t ldo_hi;
  /* 1: the FOUR phase convs of an Upsample2D as one launch (batch = 4, conv, KH = KW = 2): w = [4][N][ldw] (phase 2 dy + dx at w + z * w_bs),
   * pad_t / pad_l / out / ldo / ldo_hi / out_row_width describe phase (0, 0); phase (dy, dx) uses padding 1 - dy / 1 - dx and writes
   * ldo_hi / 2 * dy + ldo / 2 * dx elements further. */
  int32_t up_phases;
  /* 1: a 1x1 conv of a SECOND tensor appended along K -- out = conv_KHxKW(a; w[:, :KH*KW*C1]) + conv_1x1(a2; w[:, KH*KW*C1:]) + bias:
   * diffusers ResnetBlock2D's  conv2(h) + conv_shortcut(x)  (the blocks whose channel count changes: every up block of the UNet reads a
   * concatenation) as ONE launch instead of a 1x1 launch, its output's round trip and a residual read.  a2 = [B, H, W, C2] (C2 channels, same
   * pixels as the output), K = KH*KW*C1 + C2, w = [N][K] with the 1x1 weight behind the packed KHxKW weight, bias = the two biases' sum.
   * A block whose input is a concatenation (the up blocks: cat(hidden, skip)) appends BOTH tensors: a2 (C2 channels, C2 % 64 == 0) then a3
   * (C3 channels), K = KH*KW*C1 + C2 + C3.  Stride 1, same-size output, C1 % 64 == 0, no fused upsample; LDS-DMA tiles (7..23; the others are
   * mapped onto them).
   * Dense problems (conv == 0): out = [A | A2] . W^T -- the last C2 of the K columns come from a2 (row stride lda2), K - C2 a multiple of 64.
   * That is how TWO Linears without a nonlinearity between them run as one: Transformer2DModel's  proj_out(ff.net.2(g) + h) + x  is
   * [W_po W_ff2 | W_po] . [g ; h] + (W_po b_ff2 + b_po) + x  (packing `ffo_pout`: the product in fp32, one rounding). */
  int32_t k_append;
  const void* a3;         /* k_append (conv): optional second appended source [B, H, W, C3] or NULL */
  int32_t C3;
  int64_t lda2;           /* k_append (dense): row stride of a2 */
  /* GroupNorm bridge, producer side: add the statistics of the f16 values this op stores (row-major f16 outputs; not GEGLU / out2 / batch) */
  gn_stats_sink sink;
  /* GroupNorm bridge, consumer side: a (and a2 of a virtual concat) hold the RAW tensor; each A tile is normalised (x * scale + shift, SiLU)
   * in LDS after it lands, taps in the zero padding stay zero, an appended k_append segment stays raw.  Ring tiles 16 .. 22, conv or dense,
   * C1 (and C2) % 64 == 0; a row tile may span at most 4 samples (gn_gemm_norm_in_supported). */
  gn_norm_in norm_in;
  gn_norm_out norm_out;   /* GroupNorm of the output inside the split-K reduce (above) */
} gn_gemm_desc;
int32_t gn_gemm_norm_in_supported(const gn_gemm_desc* d);
int32_t gn_gemm_norm_out_supported(const gn_gemm_desc* d); /* the problem AND its plan (tile / splitk as set in d) take norm_out */
int64_t gn_gemm_workspace_bytes(const gn_gemm_desc* d);
/* 1 when the plan named in d (tile / splitk) carries the fusions attached to d -- norm_out needs a plan that splits K, norm_in a ring tile whose
 * rows span at most 4 samples -- i.e. when gn_gemm would not refuse the launch for its plan; 0 otherwise (gn_last_error says why).
 * gn_program_set_gemm_plan asks here before it patches a recorded op. */
int32_t gn_gemm_plan_valid(const gn_gemm_desc* d);
#define GN_NUM_GEMM_TILES 25
/* kernel families of the GEMM tiles: register-staged, two-stage LDS-DMA, ping-pong 256x256, three-stage LDS-DMA ring, persistent ping-pong */
enum { GN_GEMM_REG = 0, GN_GEMM_DMA = 1, GN_GEMM_PP = 2, GN_GEMM_RING = 3, GN_GEMM_PPP = 4 };
typedef struct gn_gemm_tile {
  int32_t bm, bn;   /* block tile */
  int32_t family;   /* GN_GEMM_* */
  int32_t geglu;    /* carries GN_ACT_GEGLU */
  int32_t fp8;      /* the fp8 kernel exists for this tile */
} gn_gemm_tile;
/* fills *out for tile 1 .. GN_NUM_GEMM_TILES (the gn_gemm_desc::tile values); GN_ERR_INVALID outside that range */
int32_t gn_gemm_tile_info(int32_t tile, gn_gemm_tile* out);
/* 1 when ring tile `tile` can carry norm_in for rows_per_sample output rows per sample and ct normalised channels: its rows span at most
 * 4 samples, and the ring plus their scale / shift table fit the CU's LDS */
int32_t gn_gemm_norm_in_tile_fits(int32_t tile, int64_t rows_per_sample, int64_t ct);
/* tile 25's in-launch hand-offs wait with a bound; -> how many waits have given up on the current device since the library was loaded (0 in a
 * healthy process; tests assert it). */
int64_t gn_ppp_timeouts(void);
/* probe aid (a library built with -DGN_PPP_PROFILE): per-workgroup cycle sums of the last tile-25 launch, 8 words per workgroup; zeros otherwise */
int32_t gn_ppp_profile_read(uint32_t* out, int32_t words);
/* tuning hook: force tile configuration 0..3 = {256x128, 128x128, 128x64, 64x64} for every following gn_gemm; -1 = heuristic */
int32_t gn_set_gemm_tile_override(int32_t cfg);
int32_t gn_gemm(gn_ctx* ctx, const gn_gemm_desc* d);
/* fp8 operand preparation for gn_gemm_desc.fp8: q[r, k] = e4m3_rne(x[r, k] * 448 / amax_r), scales[r] = amax_r / 448 (1 for an
 * all-zero row); x f16 [rows, ldx], q bytes [rows, ldq] with ldq % 16 == 0 and >= round_up(K, 16) (the pad bytes are written as
 * zeros), scales f32 [rows].  Activations: rows = tokens; weights [N, K]: rows = output channels (done once per weight). */
int32_t gn_quantize_fp8_rows(gn_ctx* ctx, const void* x, int64_t ldx, int64_t rows, int32_t K, void* q, int64_t ldq, void* scales);

/* ---- fused chains of a BasicTransformerBlock's Linears (csrc/tblock.hip) --------------------------------------------------------
 * One workgroup keeps 128 rows of the [M, C] residual stream in LDS for a whole chain of GEMMs and streams the chain's weights through an
 * LDS ring from a "weight tape" (one contiguous buffer holding the LDS image of every 20 KB weight slot in consumption order,
 * genima_amd/packing.py pack_tblock_tape; gn_tblock_tape_bytes() long).  Replaces, inside the diffusers transformer blocks that
 * `self.pipe(...)` runs (controller/agent/sd_controlnet_agent.py:67-76; graphs.emit_transformer), the gn_gemm launches
 *   GN_TBLOCK_FRONT: out = (a * scale[b] + shift[b]) Wi^T + bi   (Transformer2DModel.norm applied from its statistics-only pass + proj_in)
 *                   out2 = LayerNorm1(out) [Wq | Wk]^T  row-major [M, 2C];  out3 = (LayerNorm1(out) Wv^T)^T per sample: V^T [B][C][ldo3]
 *                                                         (norm1 folded into attn1.to_q / to_k / to_v; the attention kernels' operands)
 *   GN_TBLOCK_MID : out  = a Wo^T + bo + res1            (attn1.to_out.0 + residual)
 *                   out2 = LayerNorm2(out) Wq^T           (norm2 folded into attn2.to_q, as gn_gemm_desc.ln_c1)
 *   GN_TBLOCK_TAIL: h2   = a Wo^T + bo + res1            (attn2.to_out.0 + residual)
 *                   h3   = GEGLU(LayerNorm3(h2) W1^T + b1) W2^T + b2 + h2   (norm3 folded into ff.net.0.proj; ff.net.2 + residual)
 *                   out  = h3 Wp^T + bp + res2            (proj_out + the transformer's input)
 * h2 / h3 and the [M, 4C] GEGLU intermediate never leave the chip; every intermediate is rounded to f16 where the separate launches round
 * it.  Built for C = 320 (the 64x64-latent level), M % 128 == 0; gn_tblock_supported() says whether a problem qualifies.
 * All tensors f16 row-major, rows 16-byte aligned. */
enum { GN_TBLOCK_MID = 1, GN_TBLOCK_TAIL = 2, GN_TBLOCK_FRONT = 3 };
typedef struct gn_tblock_desc {
  int32_t kind;           /* GN_TBLOCK_* */
  int32_t C;              /* channels (320) */
  int64_t M;              /* rows (tokens) */
  const void* a;          /* [M, lda]: the attention output the first Linear consumes */
  const void* res1;       /* [M, ldr1]: residual of the first Linear (MID / TAIL) */
  const void* res2;       /* TAIL: [M, ldr2] residual of proj_out (the transformer's input); MID: NULL */
  void* out;              /* [M, ldo]: MID: the residual stream after attn1; TAIL: the transformer's output */
  void* out2;             /* MID: [M, ldo2] cross-attention queries; TAIL: NULL */
  const void* tape;       /* the chain's weight tape */
  int64_t tape_bytes;
  int64_t lda, ldr1, ldr2, ldo, ldo2;
  float ln_eps;
  const void* scsh;       /* FRONT: f32 [B][C][2] GroupNorm (scale, shift) pairs (gn_groupnorm_fwd with y == NULL) */
  void* out3;             /* FRONT: V^T [B][C][ldo3] */
  int64_t ldo3;
  int32_t rows_per_batch; /* FRONT: tokens per sample (a multiple of 128) */
} gn_tblock_desc;
int64_t gn_tblock_tape_bytes(int32_t kind, int32_t C);          /* 0 = not built for this kind / width */
int32_t gn_tblock_supported(int32_t kind, int64_t M, int32_t C); /* 1 / 0 */
int32_t gn_tblock(gn_ctx* ctx, const gn_tblock_desc* d);
/* The chain's weight tape from the packed f16 tensors (what genima_amd/packing.py pack_tblock_*_tape does with torch ops, bit for bit): every
 * 20 KB slot is the LDS image the kernel copies verbatim -- [rows x 32] sub-tiles with 64-byte rows whose 16-byte chunks are XOR-swizzled by
 * (row >> 2) & 3 -- in consumption order, the bias / c1 / c2 vectors behind the last slot.  Run once per checkpoint load.
 *   w_a, b_a : the chain's first Linear [C, C], [C]     (FRONT proj_in; MID attn1.to_out.0; TAIL attn2.to_out.0)
 *   w_ln, c1, c2 : its LayerNorm-folded Linear (gn_pack_fold_layernorm): FRONT attn1 q | k | v [3C, C]; MID attn2.to_q [C, C];
 *                  TAIL ff.net.0.proj [8C, C] in the packed GEGLU row order (gn_pack_geglu_rows); c1 f32, c2 f16
 *   w2, b2 : TAIL ff.net.2 [C, 4C], [C];   w_p, b_p : TAIL proj_out [C, C], [C] */
typedef struct gn_tblock_tape_src {
  int32_t kind, C;
  const void* w_a; const void* b_a;
  const void* w_ln; const float* c1; const void* c2;
  const void* w2; const void* b2;
  const void* w_p; const void* b_p;
} gn_tblock_tape_src;
int32_t gn_pack_tblock_tape(gn_ctx* ctx, const gn_tblock_tape_src* src, void* tape, int64_t tape_bytes);

/* ---- K4/K5/K11: flash-style attention forward --------------------------------------------------------------------
 * o[b, i, h*D + :] = softmax_j(scale * q[b,i,h] . k[b,j,h]) v[b,j,h]; V is consumed TRANSPOSED (vt[b][h*D + d][j], produced
 * for free by the V projection's GN_OUT_BATCH_TRANSPOSED epilogue).  Replaces xformers memory_efficient_attention / torch SDPA
 * (controller/agent/diffusion_agent.py:35-36, diffusion/train_controlnet_genima.py:1125-1126).  D in {32, 64}.
 * vt row stride must be a multiple of 8 and cover round_up(Nk, 64) columns (pad columns must hold finite values). */
typedef struct gn_attn_desc {
  const void* q; const void* k; const void* vt; void* o;
  int64_t q_bs, k_bs, vt_bs, o_bs;   /* batch strides (elements) */
  int32_t q_rs, k_rs, vt_rs, o_rs;   /* row strides (elements) */
  int32_t B, heads, Nq, Nk, D;
  int32_t causal;
  float scale;
  float* lse;                        /* optional f32 [B][heads][Nq]: log2-domain log-sum-exp of the scaled scores, kept for
                                        gn_attention_bwd (training); NULL in inference */
  int32_t v_rowmajor;                /* 1 (D = 64): `vt` is V itself, row-major [B][Nk][vt_rs] with head h at column h*D (what a plain
                                        q | k | v projection writes); the kernel transposes out of its LDS tile (ds_read_b64_tr_b16) */
} gn_attn_desc;
int32_t gn_attention_fwd(gn_ctx* ctx, const gn_attn_desc* d);
/* Tuning / test aid: pick the D = 64 forward kernel for every later gn_attention_fwd (and recorded attention op) of this process.
 * -1 = the library's own choice (default; the GN_ATTN_VARIANT environment variable, read once, sets the initial value),
 * 0 = attention.hip (4 waves x 32 rows), 4 = attention_stream.hip wherever eligible, 5 = attention_pwg.hip wherever eligible
 * (non-causal, V^T given, Nk % 64 == 0, Nk >= 128).  Returns the previous value. */
int32_t gn_attention_set_variant(int32_t variant);

/* fp8 (OCP e4m3) attention forward, D = 64 -- the opt-in attention of the fp8 training forward (BASELINE configs[4] "fp8 MFMA";
 * xformers attention under diffusion/train_controlnet_sdxl_genima.py:1448-1471).  Both products run on the K = 64 fp8 MFMA; the
 * probabilities are e4m3 too, so the result sits ~1e-2 (relative, per element) from the f16 kernel: never used by the inference path.
 * gn_attention_fp8_quantize makes the operands from the f16 q | k | v rows ([B][N][*_rs] views, head h at column 64 h):
 *   q8 [B][N][heads*64] = e4m3(q * scale * log2 e), k8 [B][N][heads*64] = e4m3(k)  (bytes, saturating at +-448),
 *   v8t [B][heads*64][Npad] = e4m3(v) transposed, the keys of every 64-key tile in the MFMA operand order (csrc/attention_fp8.hip);
 *   Npad = a multiple of 64 >= N; keys >= N are written as zeros.
 * gn_attention_fp8_fwd takes a gn_attn_desc whose q / k / vt are those byte tensors (strides in BYTES; `scale` is ignored: it is
 * already in q8; v_rowmajor must be 0), o f16 and the optional lse as for gn_attention_fwd (same log2-domain value, so
 * gn_attention_bwd can run on the f16 q / k / v the operands were made from). */
int32_t gn_attention_fp8_quantize(gn_ctx* ctx, const void* q, const void* k, const void* v, int64_t q_rs, int64_t k_rs, int64_t v_rs,
                                  int64_t q_bs, int64_t k_bs, int64_t v_bs, int32_t B, int32_t N, int32_t heads, float scale,
                                  void* q8, void* k8, void* v8t, int32_t Npad);
int32_t gn_attention_fp8_fwd(gn_ctx* ctx, const gn_attn_desc* d);

/* Flash-attention backward (D = 64; xformers memory-efficient attention backward under accelerator.backward,
 * diffusion/train_controlnet_genima.py:1125-1126, :1402).  P is recomputed per tile from q, k and the forward's lse; two
 * deterministic kernels (dQ over key tiles; dK, dV over query tiles), no atomics.  q / k / v / o / d_o and the gradients are
 * row-major [B][rows][ld] with head h at column h*D of the given base pointer; qt / kt / dot (transposed copies of Q, K, dO that
 * round 1's kernels streamed) are IGNORED and may be NULL: the kernels read the transposed operand out of the row-major LDS tile
 * with ds_read_b64_tr_b16.  Rows Nk .. Nk_rows-1 of k / v must be zero padding (their dk / dv rows are
 * written as zeros up to round_up(Nk, 128), rows past that are left untouched); Nq and Nk_rows are multiples of 8.  delta: f32 [B][heads][Nq] scratch (sum_d dO*O, written here). */
typedef struct gn_attn_bwd_desc {
  const void* q; const void* k; const void* v; const void* o; const void* d_o;
  const void* qt; const void* kt; const void* dot;
  const float* lse; float* delta;
  void* dq; void* dk; void* dv;
  int64_t q_bs, k_bs, v_bs, o_bs, do_bs, qt_bs, kt_bs, dot_bs, dq_bs, dk_bs, dv_bs;   /* batch strides (elements) */
  int32_t q_rs, k_rs, v_rs, o_rs, do_rs, qt_rs, kt_rs, dot_rs, dq_rs, dk_rs, dv_rs;   /* row strides (elements) */
  int32_t B, heads, Nq, Nk, Nk_rows, D;
  float scale;
} gn_attn_bwd_desc;
int32_t gn_attention_bwd(gn_ctx* ctx, const gn_attn_bwd_desc* d);

/* Attention-probability dropout inside the flash kernels (nn.MultiheadAttention's dropout under the reference ACT's DETR layers,
 * controller/method/genima_act.py; p = 0.1 there).  The keep mask is a pure function of (seed, bh = b * heads + h, query row i, key j),
 * evaluated wherever a kernel holds a probability, so nothing is materialised.  All arithmetic is uint32 and wraps:
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   a = mix(seed_lo ^ 0x6A09E667 ^ (bh * 0x9E3779B9))
 *   r = mix(mix((a ^ seed_hi) + i * 0x85EBCA6B) ^ (j * 0xC2B2AE35))
 *   keep(i, j) = r >= threshold,   threshold = min(2^32 - 1, floor(p * 2^32)) (made on the host in f64),   inv_keep = 1 / (1 - p)
 * threshold = 0 keeps every element.  O = ((softmax(S) o keep) * inv_keep) V; the row statistics are those of the undropped P, so lse is the
 * value gn_attention_fwd writes.  Backward: delta = sum_d dO O (O the dropped output), dV = (P o keep * inv_keep)^T dO,
 * dP = (dO V^T) o keep * inv_keep, dS = scale P (dP - delta), dQ = dS K, dK = dS^T Q. */
typedef struct gn_attn_dropout {
  uint32_t threshold, seed_lo, seed_hi;
  float inv_keep;
} gn_attn_dropout;
/* gn_attention_fwd with dropout: non-causal, V^T given (v_rowmajor = 0), D in {32, 64}; always csrc/attention.hip's 4-wave x 32-row kernel. */
int32_t gn_attention_dropout_fwd(gn_ctx* ctx, const gn_attn_desc* d, const gn_attn_dropout* dr);
/* gn_attention_bwd with dropout (D = 64), on the o and lse of gn_attention_dropout_fwd with the same gn_attn_dropout; the padded-row and
 * zero-fill contract of gn_attention_bwd holds unchanged. */
int32_t gn_attention_dropout_bwd(gn_ctx* ctx, const gn_attn_bwd_desc* d, const gn_attn_dropout* dr);
/* The same mask on a materialised f16 tensor x [bh][nq][ld] (the batched-GEMM attention backward: P, dP), in place:
 * x[b][i][j] = x[b][i][j] * keep(b, i, j) * inv_keep for i < nq, j < nk; columns nk .. ld - 1 are not touched.  With keep_out (uint8, same
 * indexing) the keep bytes (0 / 1) are written there instead and x is not read or written (x may be NULL): the mask itself, for tests. */
int32_t gn_attention_dropout_apply(gn_ctx* ctx, void* x, int32_t bh, int32_t nq, int32_t nk, int64_t ld, const gn_attn_dropout* dr, void* keep_out);

/* ---- K2: GroupNorm(+SiLU), NHWC --------------------------------------------------------------------------------
 * y = act(GroupNorm_G(cat(x, x2)) * gamma + beta).  Three launches: coalesced partial statistics over pixel slabs, a finalize
 * that folds (mean, rstd, gamma, beta) into per-(b, c) scale/shift, and a coalesced apply.  Replaces torch
 * native_group_norm + silu (every ResnetBlock2D / Transformer2DModel entry / conv_norm_out). */
typedef struct gn_groupnorm_desc {
  const void* x; const void* x2;     /* NHWC f16; x2 optional concat source */
  const void* gamma; const void* beta; /* [C1+C2] f16 */
  void* y;                           /* [B, HW, C1+C2] f16 */
  void* workspace;                   /* gn_groupnorm_workspace_bytes() */
  int32_t B, HW, C1, C2, groups;
  int32_t act;                       /* GN_ACT_NONE or GN_ACT_SILU */
  float eps;
  void* save_stats;                  /* training: optional f32 [B][groups][2] (mean, rstd) kept for gn_groupnorm_bwd */
  void* save_scsh;                   /* training: optional f32 [B][C][2] per-(b, c) scale/shift kept for gn_groupnorm_bwd */
  const void* stats_in;              /* GroupNorm bridge: the statistics block the producers of x / x2 filled (gn_stats_sink; samples = B) --
                                        ONE coalesced apply launch, no statistics passes; NULL = compute them here */
  int32_t stats_replicas;            /* replicas of stats_in (>= 1) */
} gn_groupnorm_desc;
int64_t gn_groupnorm_workspace_bytes(const gn_groupnorm_desc* d);
int32_t gn_groupnorm_fwd(gn_ctx* ctx, const gn_groupnorm_desc* d);

/* gn_groupnorm_fwd with y == NULL and save_scsh set: STATISTICS ONLY -- the per-(sample, channel) scale / shift pairs are written and
 * nothing is normalised; gn_conv3x3_gn applies them (and the SiLU) to its input patch in LDS.
 *
 * ---- 3x3 convolution (stride 1, padding 1) with GroupNorm-apply + SiLU fused into its prologue (csrc/conv_gn.hip) ------------------------
 * out = conv3x3(act(x * scale[b, c] + shift[b, c])) + bias (+ residual): diffusers ResnetBlock2D's norm1 -> SiLU -> conv1 and
 * norm2 -> SiLU -> conv2 (+ shortcut) without the normalised tensor's round trip through HBM (the VAE decoder inside `self.pipe(...)`,
 * controller/agent/sd_controlnet_agent.py:67-76).  A workgroup keeps the 10 x 18 input patch of an 8 x 16 output tile in LDS, normalises it
 * there (the arithmetic of gn_groupnorm_fwd's apply pass: the MFMA sees the same f16 values) and reads all nine taps from it.
 * Needs H % 8 == 0, W % 16 == 0, Cin % 128 == 0, and Cout % 128 == 0 or -- the narrow variant, no residual: the VAE's conv_norm_out -> SiLU ->
 * conv_out with its 3 (padded 8) output channels -- Cout in {8, 16, 24, 32} (gn_conv3x3_gn_supported). */
typedef struct gn_conv3x3_gn_desc {
  const void* x;          /* NHWC f16 [B, H, W, Cin]: the RAW tensor the GroupNorm reads */
  const void* scsh;       /* f32 [B][Cin][2] (scale, shift) from the statistics-only GroupNorm call, or NULL: plain convolution */
  const void* w;          /* packed conv weight [Cout][9 * Cin] f16 (gn_pack_conv_weight) */
  const void* bias;       /* [Cout] f16 or NULL */
  const void* residual;   /* [B * H * W, ldr] f16 or NULL: added after the bias */
  void* out;              /* [B * H * W, ldo] f16 */
  int64_t ldr, ldo;
  int32_t B, H, W, Cin, Cout;
  int32_t act;            /* GN_ACT_NONE / GN_ACT_SILU on the normalised input (with scsh) */
} gn_conv3x3_gn_desc;
int32_t gn_conv3x3_gn_supported(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int32_t gn_conv3x3_gn(gn_ctx* ctx, const gn_conv3x3_gn_desc* d);

/* ---- 3x3 convolution (stride 1, padding 1) from an LDS-resident patch in 64-channel groups, 128 x 160 output tiles (csrc/conv_patch.hip) -----
 * out = conv3x3(act(X * scale[b, c] + shift_gn[b, c])) + bias + shift[b, :] (+ residual), X = x or the virtual concat [x | x2] along channels:
 * gn_conv3x3_gn's scheme for the UNet / ControlNet ResNet convs at 320 / 640 output channels (diffusers ResnetBlock2D conv1 with its
 * time_emb_proj shift and, in the up blocks, its concatenated input; conv2 with its residual).  Same packed weight [Cout][9 * (C1 + C2)] as gn_gemm.
 * Needs H % 8 == 0, W % 16 == 0, (C1 + C2) % 64 == 0, C1 % 64 == 0 when x2 is given, Cout % 160 == 0 (gn_conv3x3_patch_supported); an
 * unsupported problem is an error and launches nothing.  Epilogue order: bias, time shift, residual (gn_gemm's), in f32, one rounding. */
typedef struct gn_conv3x3_patch_desc {
  const void* x;          /* NHWC f16 [B, H, W, C1]: the RAW tensor the GroupNorm reads */
  const void* x2;         /* NHWC f16 [B, H, W, C2] or NULL: channels C1 .. C1 + C2 - 1 of the virtual concat */
  const void* scsh;       /* f32 [B][C1 + C2][2] (scale, shift) by concatenated channel from the statistics-only GroupNorm call, or NULL: plain conv */
  const void* w;          /* packed conv weight [Cout][9 * (C1 + C2)] f16 (gn_pack_conv_weight) */
  const void* bias;       /* [Cout] f16 or NULL */
  const void* shift;      /* [B, ldshift] f16 or NULL: per-sample channel shift (a column slice of the time-shift table) */
  const void* residual;   /* [B * H * W, ldr] f16 or NULL: added last */
  void* out;              /* [B * H * W, ldo] f16 */
  int64_t ldr, ldo, ldshift;
  int32_t B, H, W, C1, C2, Cout;
  int32_t act;            /* GN_ACT_NONE / GN_ACT_SILU on the normalised input (with scsh) */
} gn_conv3x3_patch_desc;
int32_t gn_conv3x3_patch_supported(int32_t B, int32_t H, int32_t W, int32_t C1, int32_t C2, int32_t Cout);
int32_t gn_conv3x3_patch(gn_ctx* ctx, const gn_conv3x3_patch_desc* d);

/* ---- diffusers AutoencoderTinyBlock at 64 channels as one launch (csrc/taesd.hip) ----------------------------------------------------
 * out = relu(conv3(relu(conv2(relu(conv1(x))))) + x): 3x3 convs, stride 1, padding 1, NHWC f16 [B, H, W, 64] -- every block of the
 * TAESD / TAESDXL encoder.  w[k]: packed conv weight [64][9 * 64] f16 (gn_pack_conv_weight), bias[k]: [64] f16.  The two intermediate
 * maps stay in LDS, rounded to f16 and ReLU'd as the three-launch route stores them; out must not overlap x.
 * gn_tiny_block_supported: C == 64, any H, W > 0. */
int32_t gn_tiny_block_supported(int32_t C, int32_t H, int32_t W);
int32_t gn_tiny_block(gn_ctx* ctx, const void* x, const void* const w[3], const void* const bias[3], void* out, int32_t B, int32_t H,
                      int32_t W, int32_t C);

/* ---- K7: LayerNorm over the last dim of [M, C] (C % 8 == 0, C <= 4096) --------------------------------------------- */
int32_t gn_layernorm_fwd(gn_ctx* ctx, const void* x, const void* gamma, const void* beta, void* y,
                         int64_t M, int32_t C, float eps);

/* ---- K9: sinusoidal timestep embedding -> f16 [B, dim]  (t: device f32 [B]) ------------------------------------- */
int32_t gn_timestep_embedding(gn_ctx* ctx, const float* t, void* out, int32_t B, int32_t dim, int32_t flip_sin_to_cos,
                              float freq_shift);

/* ---- K10: scheduler elementwise ops on f16 latents [n] ------------------------------------------------------------
 * gn_scale_pad:  out[p, 0:C] = x[p, 0:C] * scale, out[p, C:Cpad] = 0       (scale_model_input / latents/scaling_factor,
 *                and the channel padding the implicit-GEMM conv wants for Cin = 4)
 * gn_euler_step: x <- x + eps * (sigma_next - sigma), f32 math, f16 storage; eps has row stride ld_eps
 * gn_add_noise:  out = a[b] * x0 + c[b] * noise  (DDPM add_noise, diffusion/train_controlnet_genima.py:1359) */
int32_t gn_scale_pad(gn_ctx* ctx, const void* x, void* out, int64_t pixels, int32_t C, int32_t Cpad, float scale);
int32_t gn_euler_step(gn_ctx* ctx, void* x, const void* eps, int64_t pixels, int32_t C, int32_t ld_eps, float sigma,
                      float sigma_next);
/* InstructPix2Pix channel concatenation (diffusers StableDiffusionInstructPix2PixPipeline: cat([scale_model_input(latents), image_latents],
 * dim=1); diffusion/train_instruct_pix2pix_genima.py:1236-1239): out[p, 0:C] = x[p*ld1 + 0:C] * scale, out[p, C:C+C2] = x2[p*ld2 + 0:C2] * scale2,
 * out[p, C+C2:Cpad] = 0 */
int32_t gn_scale_cat_pad(gn_ctx* ctx, const void* x, const void* x2, void* out, int64_t pixels, int32_t C, int32_t ld1, int32_t C2,
                         int32_t ld2, int32_t Cpad, float scale, float scale2);
int32_t gn_add_noise(gn_ctx* ctx, const void* x0, const void* noise, const float* sqrt_ac, const float* sqrt_1mac,
                     void* out, int32_t B, int64_t per_sample);

/* ---- K14: image pre/post-processing ------------------------------------------------------------------------------
 * gn_image_u8_to_f16: uint8 NHWC [pixels, 3] -> f16 [pixels, Cpad]: v/255*mul + add  (VaeImageProcessor.preprocess)
 * gn_image_f16_to_u8: f16 [pixels, ld] -> uint8 [pixels, 3]: round(clamp(v/2+0.5, 0, 1)*255)  (postprocess, Appendix D.6) */
int32_t gn_image_u8_to_f16(gn_ctx* ctx, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad, float mul, float add);
int32_t gn_image_f16_to_u8(gn_ctx* ctx, const void* in, uint8_t* out, int64_t pixels, int32_t ld);
/* The same conversion over B frames that lie anywhere on the device (the DataLoader's frame cache, genima_amd/data.py):
 * out[b, p, :] = frame src[b] pixel p: v / 255 * mul + add in channels 0..2, zeros up to Cpad (as gn_image_u8_to_f16, bit for bit).
 * src: DEVICE array of B device pointers to uint8 [pixels, 3] frames (4-byte aligned; pointers may repeat). */
int32_t gn_gather_u8_to_f16(gn_ctx* ctx, const uint8_t* const* src, void* out, int32_t B, int64_t pixels, int32_t Cpad, float mul, float add);
/* One training batch of the ACT controller out of a device-resident demo set (genima_amd/replay.py DeviceReplay; the reference's
 * controller/utils/dataloader.py _sample), one launch.  Tables, all on the device:
 *   frame_ptr  int64 [N_obs][V]  addresses of uint8 [pixels, 3] frames (4-byte aligned frames take dword loads, others byte loads)
 *   qpos       f32 [N_obs][S], action f32 [N][A]: already normalised
 *   obs_index, first_obs, last_tr  int32 [N]: a transition's own observation, the first observation and the last transition of its episode
 *   lang_tokens int32 [N_ep][L_tok], episode int32 [N] (a transition's episode): optional, read only when tokens_out is given
 *   idx        int32 [B]: the batch's transitions, ON THE DEVICE (repeats allowed); a value outside [0, N) is clamped into it
 * Per sample b, n = idx[b], frame-stack slot k < fs reads observation o(k) = max(obs_index[n] - (fs - 1) + k, first_obs[n]):
 *   images[b][v * fs + k][p][0..7]   f16 = frame (o(k), v) pixel p: byte / 255 in channels 0..2 (gn_image_u8_to_f16 with mul 1, add 0, bit
 *                                    for bit), zeros in 3..7; 16-byte aligned
 *   images_u8[b][v * fs + k][p][0..2]  the same bytes unconverted; optional (NULL: not written)
 *   low_dim_state[b][k][0..S)        = qpos[o(k)]
 *   action_out[b][j][0..A)           = action[min(n + j, last_tr[n])], j < T: the chunk repeats the episode's last action
 *   tokens_out[b][0..L_tok)          = lang_tokens[episode[n]]; optional (NULL: not written)
 * B <= 65535, V * fs <= 65535.  Every table index is clamped into its table.  Eager only: no gn_program_add_ counterpart. */
typedef struct gn_replay_gather_desc {
  const int64_t* frame_ptr;
  const float* qpos;
  const float* action;
  const int32_t* obs_index;
  const int32_t* first_obs;
  const int32_t* last_tr;
  const int32_t* idx;
  void* images;
  uint8_t* images_u8;
  float* low_dim_state;
  float* action_out;
  const int32_t* lang_tokens;
  const int32_t* episode;
  int32_t* tokens_out;
  int64_t pixels, N_obs;
  int32_t B, V, fs, T, S, A, N, N_ep, L_tok;
} gn_replay_gather_desc;
int32_t gn_replay_gather(gn_ctx* ctx, const gn_replay_gather_desc* d);
/* ACT image path (controller/method/genima_act.py:146-148, :188): uint8 [pixels, 3] -> f16 [pixels, Cpad]: v * m_c + a_c
 * (m_c = 1/(255 std_c), a_c = -mean_c/std_c; channels >= 3 zero) */
int32_t gn_image_normalize_u8(gn_ctx* ctx, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad, float m0, float m1,
                              float m2, float a0, float a1, float a2);
/* ---- weight repacking (explicit gn_pack_* calls into caller-owned buffers; genima_amd/packing.py is the Python
 * host's torch restatement of the same layouts, bit-identical on the two copies: tests/test_kernels_gpu.py) -------------------------
 * diffusers Conv2d.weight OIHW (f32, or f16 when src_f16) -> dst f16 [round_up(O, 8)][KH * KW * round_up(I, 8)] with
 * dst[o][(kh * KW + kw) * Ip + c] = src[o][c][kh][kw], zero padding: the W operand of gn_gemm(conv) */
int32_t gn_pack_conv_weight(gn_ctx* ctx, const void* src_oihw, int32_t src_f16, void* dst, int32_t O, int32_t I, int32_t KH, int32_t KW);
/* diffusers GEGLU.proj weight [2H, K] (or its bias: K = 1), hidden rows first then gate rows -> alternating 32-row blocks
 * [hidden 0..31 | gate 0..31 | hidden 32..63 | ...], the order GN_ACT_GEGLU's epilogue pairs up.  H % 32 == 0 */
int32_t gn_pack_geglu_rows(gn_ctx* ctx, const void* src, int32_t src_f16, void* dst, int32_t H, int64_t K);
/* operands of gn_gemm_desc::ln_c1 from a packed f16 Linear weight w [N, K] (row stride ldw) and its LayerNorm's gamma / beta [K]
 * (+ the Linear's bias [N] or NULL): ln_weight = f16(w * gamma) [N, K] (row stride ldw), ln_c1[n] = sum_k ln_weight[n, k] (f32),
 * ln_c2[n] = f16(sum_k w[n, k] * beta[k] + bias[n]) */
int32_t gn_pack_fold_layernorm(gn_ctx* ctx, const void* w, const void* gamma, const void* beta, const void* bias, void* ln_weight,
                               float* ln_c1, void* ln_c2, int32_t N, int32_t K, int64_t ldw);
/* out[b, :] = x[b, idx[b], :]  (CLIP EOT-token pooling, controller/method/genima_act.py:337-343) */
int32_t gn_gather_rows(gn_ctx* ctx, const void* x, const int32_t* idx, void* out, int32_t B, int32_t L, int32_t D);
/* out[i] = index of the first maximum of row i of an int32 [rows, cols] matrix (EOT = highest token id) */
int32_t gn_argmax_rows_i32(gn_ctx* ctx, const int32_t* x, int32_t* out, int32_t rows, int32_t cols);
/* strided 4-D copy of contiguous f16 runs of L elements (L % 8 == 0; strides in elements, multiples of 8): the layout shuffles
 * between kernels (ACT: per-view feature maps -> views-along-width token rows of the encoder sequence) */
int32_t gn_copy4d(gn_ctx* ctx, const void* in, void* out, const int64_t* sizes, const int64_t* in_strides,
                  const int64_t* out_strides, int32_t L);

/* ---- misc elementwise / gather ------------------------------------------------------------------------------------ */
int32_t gn_add(gn_ctx* ctx, const void* a, const void* b, void* out, int64_t n);              /* f16, n % 8 == 0 */
/* count <= GN_ADD_MULTI_MAX independent out[i] = a[i] + b[i] (n[i] % 8 == 0) as ONE launch: UNet2DConditionModel.forward's
 * `down_block_res_samples + down_block_additional_residuals` / `sample + mid_block_additional_residual` additions (thirteen torch adds
 * inside `self.pipe(...)`, controller/agent/sd_controlnet_agent.py:67-76) */
#define GN_ADD_MULTI_MAX 16
int32_t gn_add_multi(gn_ctx* ctx, const void* const* a, const void* const* b, void* const* out, const int64_t* n, int32_t count);
/* the same adds with the GroupNorm bridge's producer side: tensor i is [n[i] / C[i]] rows of C[i] channels and adds the statistics of what it
 * stores to sinks[i] (sinks[i].stats == NULL: none) -- the UNet's skip + ControlNet-residual sums feed the decoder's concatenated GroupNorms */
int32_t gn_add_multi_stats(gn_ctx* ctx, const void* const* a, const void* const* b, void* const* out, const int64_t* n, const int32_t* C,
                           const gn_stats_sink* sinks, int32_t count);
int32_t gn_act(gn_ctx* ctx, const void* x, void* out, int64_t n, int32_t act);                /* f16, n % 8 == 0 */
/* FiLM (controller/method/genima_act.py:190: ``encoder_model(image, task_emb)`` with use_lang_cond, genima_act.yaml:39):
 * out[r, :] = act((1 + gamma[r / rows_per_film, :]) * x[r, :] + beta[r / rows_per_film, :]); x / out f16 [rows, C], gamma / beta f16 rows of
 * stride ld_film (slices of the per-layer FiLM feature buffer); out may alias x */
int32_t gn_film(gn_ctx* ctx, const void* x, void* out, const void* gamma, const void* beta, int64_t ld_film, int64_t rows_per_film,
                int64_t rows, int32_t C, int32_t act);
int32_t gn_embedding(gn_ctx* ctx, const int32_t* ids, const void* tok, const void* pos, void* out, int32_t B,
                     int32_t L, int32_t D);                                                   /* CLIP token + position */
int32_t gn_softmax_rows(gn_ctx* ctx, void* x, int64_t rows, int32_t cols, int32_t ld, float scale); /* in place, f16 */
/* same with key padding: columns >= valid get probability 0 (cols stays a multiple of 8) */
int32_t gn_softmax_rows_masked(gn_ctx* ctx, void* x, int64_t rows, int32_t cols, int32_t ld, float scale, int32_t valid);
int32_t gn_maxpool3x3s2(gn_ctx* ctx, const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C);

/* ---- temporal ensembling of action chunks (the `execution_horizon` / `temporal_agg` knobs of controller/cfgs/eval_genima.yaml:29,33, which the
 * reference never reads: controller/eval_genima.py:261-263; the rule is the ACT paper's, generalised from one executed action per call to h) ----
 * chunk  f32 [B, T, ld] (gn_action_ensemble) or f16 [B, T, ld] (gn_action_ensemble_f16: the controller's a_hat as its head writes it; every f16
 *        is an f32, so the two agree bit for bit on equal values); ld >= A is the row pitch, only the first A columns are read
 * state  gn_action_ensemble_state_bytes(B, T, A, K) bytes (-1: bad shape), 16-byte aligned, zeroed ONCE by the caller (a zeroed row is an empty
 *        one).  Per row: the last K chunks as f32 [K, T, A], the environment step each slot's chunk starts at (int32, -1 = empty), the ring head
 * steps  int32 [B] on the device: the current environment step t >= 0 of each row
 * reset  uint8 [B] on the device: non-zero empties that row's ring before the new chunk goes in
 * out    f32 [B, h, A]: the actions of the environment steps t .. t + h - 1
 * The new chunk replaces the oldest slot, with start t.  For a target step s every slot with 0 <= s - start < T takes part; those slots in
 * order of insertion (i = 0: the oldest; the order of their starts as long as steps do not go backwards between resets) get the weights
 * w_i = exp(-m i), and out[s] = sum_i w_i chunk_i[s - start_i] / sum_i w_i, summed in f32 from the oldest to the newest -- the same bits on every
 * run.  Every one of the A dimensions is averaged alike, the gripper's included (the reference gives no other rule).  K >= ceil(T / h) holds every
 * chunk that can still cover a step when t advances by h per call; a smaller K is refused -- except K = 1, the ring of the new chunk alone
 * (temporal_agg off): out = chunk[:, :h, :A] bit for bit.
 * One launch, one workgroup per row, plain loads and stores; between replays of a recorded program only the contents of steps / reset change. */
int64_t gn_action_ensemble_state_bytes(int32_t B, int32_t T, int32_t A, int32_t K);
int32_t gn_action_ensemble(gn_ctx* ctx, const float* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B, int32_t T,
                           int32_t A, int32_t ld, int32_t K, int32_t h, float m);
int32_t gn_action_ensemble_f16(gn_ctx* ctx, const void* chunk, void* state, const int32_t* steps, const uint8_t* reset, float* out, int32_t B, int32_t T,
                               int32_t A, int32_t ld, int32_t K, int32_t h, float m);

/* ---- R sampled chunks combined into the one that is executed.  The diffusion stage draws noise, so R draws for one observation give R chunks;
 * the combined chunk enters the ring above as the new chunk, and from there on the rule, the state blob and gn_action_ensemble_state_bytes are
 * gn_action_ensemble's.  The combination, element e = t * A + a of a chunk (t < T, a < A), x_r the f16 sample r widened to f32:
 *   mean    mean[e] = (x_0[e] + x_1[e] + .. + x_{R-1}[e]) * inv_R: f32 additions in sample order starting from x_0[e], then one multiplication by
 *           inv_R, which must be (float)(1.0 / R) rounded once by the caller (any other value is refused) -- gn_openloop_seed_actions' mean_j, so
 *           its seed_mean columns describe the chunk executed here
 *   medoid  d(r, q) = sum_e |x_r[e] - x_q[e]|, D_r = sum_q d(r, q), pick = the lowest r with the smallest D_r; the combined chunk is sample
 *           `pick` widened.  All A dimensions count alike, the gripper's included.  D_r is summed in f32 in ONE fixed order by the row's workgroup
 *           of 256 threads: thread i adds its terms for q = 0 .. R - 1 (outer) and e = i, i + 256, .. < T * A (inner) to one f32 starting from 0;
 *           within each wave of 64 lanes the 64 sums are added by the xor butterfly over lane distances 32, 16, 8, 4, 2, 1; then
 *           D_r = ((w0 + w1) + w2) + w3 over the four waves.  Picks compare with <, from r = 0 up.  No atomics: equal inputs give equal picks in
 *           both entry points below and on every run
 *   spread  = (sum_r sum_e |x_r[e] - chosen[e]|) * inv_R / (float)(T * A): the samples' mean absolute disagreement with what is executed, in
 *           normalised action units.  Three operations in this order: the sum (thread i adds e = i, i + 256, .. (outer), r = 0 .. R - 1 (inner);
 *           butterfly and waves as for D_r), one multiplication by inv_R, one division by (float)(T * A)
 * R = 1 under either rule is the sample itself: outputs and state bytes are gn_action_ensemble_f16's bit for bit (pick 0 under medoid, spread 0).
 *
 * gn_action_ensemble_samples_f16: one launch, one workgroup per row b, which stages the row's R * T * A values as f32 in LDS.
 *   chunk    f16: sample r of row b is [T][ld] from chunk + b * bs + r * ss (elements).  [B][R]: bs = R * T * ld, ss = T * ld; [R][B]: bs = T * ld,
 *            ss = B * T * ld
 *   combine  0 = mean, 1 = medoid;  state, steps, reset, out, K, h, m as gn_action_ensemble takes them
 *   pick_out int32 [B] or NULL: the pick, -1 under mean;  spread_out f32 [B] or NULL
 *   The output pass takes the new slot's values from LDS, not from the ring: no thread reads a word of device memory another thread of the
 *   launch writes.  Refused, launching nothing and leaving outputs and state as they were: whatever gn_action_ensemble_f16 refuses, R outside
 *   [1, GN_ENSEMBLE_MAX_SAMPLES], R * T * A > GN_ENSEMBLE_MAX_STAGED, a wrong inv_R, combine outside {0, 1}, a misaligned pointer, negative
 *   strides and strides under which two samples of (T - 1) * ld + A elements overlap. */
#define GN_ENSEMBLE_MAX_SAMPLES 64
#define GN_ENSEMBLE_MAX_STAGED 12288
int32_t gn_action_ensemble_samples_f16(gn_ctx* ctx, const void* chunk, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine, void* state,
                                       const int32_t* steps, const uint8_t* reset, float* out, int32_t* pick_out, float* spread_out, int32_t B, int32_t T,
                                       int32_t A, int32_t ld, int32_t K, int32_t h, float m);

/* ---- training-side kernels (ControlNet fine-tune step, diffusion/train_controlnet_genima.py:1317-1408) ----------
 * The backward matrix products reuse gn_gemm: dX = dY.W through a transposed weight copy, dW = dY^T.X through transposed
 * activations with GN_OUT_F32 + split-K, conv dgrad = conv with rotated weights, conv wgrad = GEMM over gn_im2col_t's image.
 * Parameter gradients are f32 and accumulate; all reductions are deterministic. */
int32_t gn_transpose2d(gn_ctx* ctx, const void* in, void* out, int32_t rows, int32_t cols, int64_t ld_in, int64_t ld_out,
                       int32_t batch, int64_t in_bs, int64_t out_bs);                 /* out[b][c][r] = in[b][r][c] (f16) */
/* the same, and columns [rows, ld_out) of every output row are written as zeros (ld_out <= round_up(rows, 64)): the padded reduction length
 * of a GEMM operand -- the cross-attention V^T of 77 tokens -- without a fill launch in front of the transpose */
int32_t gn_transpose2d_zpad(gn_ctx* ctx, const void* in, void* out, int32_t rows, int32_t cols, int64_t ld_in, int64_t ld_out,
                            int32_t batch, int64_t in_bs, int64_t out_bs);
/* out[(tap*C + c)][m] = x[b, oy*stride - pad + dy, ox*stride - pad + dx, c] (0 in the padding); M = B*Ho*Wo contiguous */
int32_t gn_im2col_t(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ksize,
                    int32_t stride, int32_t pad);
/* ---- weight gradient on operands in their forward layout (no transposed copies, no im2col^T) ---------------------------------------
 * dw[n, k] += sum_r dy[r, n] * X[r, k];  dense: X = x [R, ld_x];  conv: X[r, tap * C + c] = x[b, oy*stride - pad + dy, ox*stride - pad + dx, c]
 * for r = (b, oy, ox), zero outside the image (x NHWC [B, H, W, C], C % 8 == 0).  What autograd computes for nn.Linear / nn.Conv2d weights
 * inside accelerator.backward(loss) (diffusion/train_controlnet_genima.py:1391).  f32 result accumulated into dw; the reduction over the
 * R rows is split across workgroups deterministically (workspace: gn_wgrad_workspace_bytes). */
typedef struct gn_wgrad_desc {
  const void* dy;        /* f16 [R, ld_dy] */
  const void* x;         /* f16 [R, ld_x] or NHWC [B, H, W, C] */
  float* dw;             /* f32 [N, ld_dw], accumulated */
  void* workspace;
  int64_t R, N, K;       /* K = columns of dw (conv: KH*KW*C) */
  int64_t ld_dy, ld_x, ld_dw;
  int32_t conv, B, H, W, C, KH, KW, stride, pad, Ho, Wo;
  int32_t tile;          /* 0 = heuristic, 1 = 128x128, 2 = 64x64, 3 = 128x256, 4 = 256x128 on eight waves (N / K at least a tile; else 128x128) */
  int32_t splitk;        /* 0 = heuristic */
  float* dbias;          /* optional f32 [N] += column sums of dy (the bias gradient), from the fragments the kernel loads anyway */
  float* dshift;         /* optional f32 [shift_groups, N] += column sums per block of R / shift_groups rows (per-sample time-shift gradient) */
  int32_t shift_groups;  /* R / shift_groups must be a multiple of 64 */
} gn_wgrad_desc;
int64_t gn_wgrad_workspace_bytes(const gn_wgrad_desc* d);
int32_t gn_wgrad(gn_ctx* ctx, const gn_wgrad_desc* d);

/* Many gn_transpose2d problems in ONE launch (the trainable network's derived weight copies -- W^T for the Linears' data gradients,
 * the tap-rotated conv weights -- are rebuilt after every optimizer step; accelerate / autograd get them for free from cuBLAS's
 * transposed operand forms, diffusion/train_controlnet_genima.py:1391).  `items`: DEVICE memory, each as the 16-byte-vector form of
 * gn_transpose2d requires; block_begin = running sum of batch * ceil(rows/64) * ceil(cols/64), total_blocks = its end. */
typedef struct gn_transpose_item {
  const void* in; void* out;
  int64_t ld_in, ld_out, in_bs, out_bs;
  int32_t rows, cols, batch, block_begin;
} gn_transpose_item;
int32_t gn_transpose2d_multi(gn_ctx* ctx, const gn_transpose_item* items, int32_t n_items, int32_t total_blocks);

/* gn_transpose2d of one matrix that also yields sums[g][cols] += the column sums of row block g (groups = 1: bias gradient;
 * groups = batch: per-sample time-shift gradient; sums2 / groups2: an optional second grouping from the same pass) -- the
 * weight-gradient path transposes dY anyway.  (rows / groups) % 64 == 0; workspace: ceil(rows / 64) * cols floats.  Replaces the
 * `.sum(0)` of autograd's Linear / conv bias backward. */
int32_t gn_transpose2d_colsum(gn_ctx* ctx, const void* in, void* out, int32_t rows, int32_t cols, int64_t ld_in, int64_t ld_out,
                              float* sums, int32_t groups, float* sums2, int32_t groups2, void* workspace);
int64_t gn_colsum_workspace_bytes(int32_t nb, int32_t rows_per_batch, int32_t cols);
/* out[b][c] (+)= sum_r x[b*rows_per_batch + r][c]  (bias gradients nb = 1; time-shift gradients nb = batch) */
int32_t gn_colsum_f32(gn_ctx* ctx, const void* x, float* out, int32_t nb, int32_t rows_per_batch, int32_t cols, int64_t ld,
                      void* workspace, int32_t accumulate);
int32_t gn_reduce_rows_f32(gn_ctx* ctx, const float* part, float* out, int32_t groups, int32_t R, int32_t cols, int32_t accumulate);
int32_t gn_act_bwd(gn_ctx* ctx, const void* dy, const void* z, void* dz, int64_t n, int32_t act);   /* dz = dy * act'(z) */
/* unfused GEGLU out = hidden * gelu(gate); hg [M, 2*Hd]: block == 0 -> [hidden | gate] halves, block > 0 -> alternating
 * block-column groups [hidden | gate] (the packed ff.net.0.proj layout of GN_ACT_GEGLU, block = 32) */
int32_t gn_geglu_fwd(gn_ctx* ctx, const void* hg, void* out, int64_t M, int32_t Hd, int32_t block);
int32_t gn_geglu_bwd(gn_ctx* ctx, const void* dy, const void* hg, void* dhg, int64_t M, int32_t Hd, int32_t block);
/* attention backward softmax step, in place over dp: ds = scale * p * (dp - rowsum(p * dp)) */
int32_t gn_softmax_bwd(gn_ctx* ctx, const void* p, void* dp, int64_t rows, int32_t cols, int64_t ld, float scale);
int64_t gn_layernorm_bwd_workspace_bytes(int64_t M, int32_t C);
/* dx from (x, gamma, dy); dgamma/dbeta (f32, dbeta == dgamma + C, accumulated) optional */
/* dx_add (optional, may alias dx): the gradient x already holds from another branch; dx = f16(f16(dx) + dx_add) */
int32_t gn_layernorm_bwd(gn_ctx* ctx, const void* x, const void* gamma, const void* dy, void* dx, float* dgamma, float* dbeta,
                         void* workspace, int64_t M, int32_t C, float eps, const void* dx_add);
int64_t gn_groupnorm_bwd_workspace_bytes(int32_t B, int32_t HW, int32_t C);
/* backward of gn_groupnorm_fwd(d) run with save_stats/save_scsh; dx / dx2 follow d->x / d->x2 (either may be NULL).
 * C1 + C2 <= 4096 divisible into d->groups groups of at most 256 channels; dgamma / dbeta (f32 [C], accumulated) come together or not
 * at all.  Every argument check precedes the first launch: a refused call writes nothing. */
int32_t gn_groupnorm_bwd(gn_ctx* ctx, const gn_groupnorm_desc* d, const void* dy, void* dx, void* dx2, const float* scsh,
                         const float* stats, float* dgamma, float* dbeta, void* workspace, const void* dx_add, const void* dx2_add);
int32_t gn_zero_upsample2x(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C); /* stride-2 dgrad */
int32_t gn_sumpool2x2(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C);       /* upsample dgrad */
int32_t gn_mse_loss(gn_ctx* ctx, const void* pred, const void* target, void* dpred, float* loss_out, void* workspace,
                    int64_t pixels, int32_t C, int32_t ld_pred, int32_t ld_target, float grad_scale);
/* ---- sphere-weighted loss (csrc/loss_weight.hip): an EXTENSION of the reference, used only with ControlNetTrainer's sphere_loss_weight > 0.
 * Eager only; none of the three synchronises; every argument check precedes the first launch: a refused call writes nothing, returns
 * non-zero and sets the last error.  Each product and sum below is one rounded operation (no fused multiply-add).
 *
 * gn_change_mask: where the target image differs from the conditioning image, on the bytes the f16 batch was made from -- the `a_gt > 0`
 * rule of the sphere metrics.  target / cond f16 [B][H][W][ld_t / ld_c], ld >= 3; mask f16 [B][H][W][8], 16-byte aligned.  Per pixel and
 * channel c < 3: tb_c = clamp(rintf(target_c * t_mul + t_add), 0, 255) in f32 (a NaN gives 0), cb_c alike from cond with c_mul, c_add;
 * d = sum_c |tb_c - cb_c| (exact integers); mask[..][0] = d > threshold ? 1 : 0, channels 1..7 = 0.  An image in [-1, 1] takes
 * (127.5, 127.5), one in [0, 1] takes (255, 0).  Refused: a NULL pointer, B, H or W <= 0, ld < 3, threshold < 0, a non-finite scale or
 * offset, a misaligned pointer. */
int32_t gn_change_mask(gn_ctx* ctx, const void* target, const void* cond, void* mask, int32_t B, int32_t H, int32_t W, int32_t ld_t, int32_t ld_c,
                       float t_mul, float t_add, float c_mul, float c_add, int32_t threshold);
/* gn_loss_weight_pool: the per-latent-pixel loss weight.  mask f16 [B][H][W][ld_m] (channel 0 is read); F = H / h = W / w in 1 .. 16.
 * n = the number of mask pixels of a latent pixel's F x F block whose channel 0 is != 0;
 *   weight       f32 [B][h][w] = 1 + lambda * (n / (F * F)), in f32
 *   count_total  int64 [1], 8-byte aligned = the sum of all n: integer additions only (64-bit vector atomics on this word, which the entry
 *                point zeroes on the ctx stream), so every run gives the same bits
 *   wsum         f64 [1], 8-byte aligned = (double)(B * h * w) + (double)lambda * (double)count_total / (double)(F * F) = the sum of weight
 * Refused: a NULL pointer, a size <= 0, H % h or W % w != 0, H / h != W / w, F > 16, lambda < 0 or not finite, a misaligned pointer. */
int32_t gn_loss_weight_pool(gn_ctx* ctx, const void* mask, int32_t ld_m, float* weight, int64_t* count_total, double* wsum, int32_t B, int32_t H,
                            int32_t W, int32_t h, int32_t w, float lambda);
/* gn_mse_loss_weighted: gn_mse_loss with a per-pixel weight and a weighted MEAN.  weight f32 [pixels]; wsum f64 [1] (device memory, read inside
 * the kernels: the host never reads it).  gs = (grad_scale * 2) / (float)((double)C * wsum[0]); d = (float)pred - (float)target;
 * dpred = the f16 nearest to (gs * weight[px]) * d -- the f32 factor gs * weight[px] times d, exact, rounded once -- for c < C, 0 in the padded channels; loss_out[0] = sum(weight * d * d) / (C * wsum[0]), by gn_mse_loss's
 * fixed-order two-stage reduction (the same workspace).  dpred may be NULL.  With weight == 1 and wsum == pixels, dpred has gn_mse_loss's bits. */
int32_t gn_mse_loss_weighted(gn_ctx* ctx, const void* pred, const void* target, const float* weight, const double* wsum, void* dpred, float* loss_out,
                             void* workspace, int64_t pixels, int32_t C, int32_t ld_pred, int32_t ld_target, float grad_scale);
/* gn_mse_loss_parts: what a loss is made of -- a READ-OUT (ControlNetTrainer's loss_parts / eval_loss), never a loss: it produces no gradient.
 * pred f16 [B][h][w][ld_pred], target f16 [B][h][w][ld_target] (the first C channels valid); mask f16 [B][H][W][ld_m] (channel 0 is read,
 * F = H / h = W / w in 1 .. 16) or NULL = nothing marked (H, W, ld_m are then ignored); bucket int32 [B] in device memory; table f64
 * [n_buckets + 1][5], 8-byte aligned, ACCUMULATED into (the caller zeroes it); workspace: gn_mse_loss_parts_workspace_bytes(B, h, w),
 * 8-byte aligned.  Per latent pixel p of sample b: n_p = the mask pixels of its F x F block whose channel 0 is != 0, s_p = n_p / (F F) in
 * f64, d = (float)pred - (float)target (one f32 subtraction), e_p = sum_{c < C} (double)d (double)d in f64.  Per sample:
 *   S_b = sum_p s_p e_p,  G_b = sum_p (1 - s_p) e_p,  A_b = (sum_p n_p) / (F F) (the count is kept as an integer),  P_b = h w
 * and row bucket[b] of the table gains (S_b, G_b, A_b, P_b, 1), b = 0 .. B - 1 in that order by one thread; a bucket[b] outside
 * 0 .. n_buckets - 1 goes to the extra last row.  Two stages in a fixed order (contiguous ranges of 256 pixels through a fixed lane tree,
 * then the ranges in index order), no floating-point atomics: every run gives the same bits.  Never synchronises.  Refused before the
 * first launch (nothing is written): a NULL pointer other than mask, a size <= 0, C > ld_pred or C > ld_target, n_buckets < 1, a
 * misaligned pointer, and with a mask H % h, W % w, H / h != W / w or F > 16. */
int64_t gn_mse_loss_parts_workspace_bytes(int32_t B, int32_t h, int32_t w);
int32_t gn_mse_loss_parts(gn_ctx* ctx, const void* pred, const void* target, const void* mask, const int32_t* bucket, double* table, void* workspace,
                          int32_t B, int32_t h, int32_t w, int32_t C, int32_t ld_pred, int32_t ld_target, int32_t H, int32_t W, int32_t ld_m,
                          int32_t n_buckets);
int32_t gn_sumsq_f32(gn_ctx* ctx, const float* x, int64_t n, float* out, void* workspace);
/* global-norm clipping after loss-scale removal (accelerator.clip_grad_norm_, diffusion/train_controlnet_genima.py:1403-1405):
 * norm = sqrt(sumsq[0]) * inv_scale; clip[0] = min(1, max_norm / (norm + 1e-6)); clip[1] = norm; clip[2] = 1 when non-finite
 * (gn_adamw_flat given this clip buffer then leaves the parameters untouched, as GradScaler.step does) */
int32_t gn_clip_coef(gn_ctx* ctx, const float* sumsq, float* clip, float max_norm, float inv_scale);
/* half_out (optional): f16 [n] working copy of the parameters, refreshed in the same pass; zero_grad: grad is cleared in the same pass
 * (optimizer.zero_grad(), also when the step is skipped) */
int32_t gn_adamw_flat(gn_ctx* ctx, float* param, float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int32_t step, const float* clip_dev, float grad_scale,
                      void* half_out, int32_t zero_grad);
/* 8-bit blockwise AdamW (the reference's --use_8bit_adam = bitsandbytes.optim.AdamW8bit; csrc/optim8.hip): gn_adamw_flat's update with both
 * moments stored as one code byte per element + one f32 absmax per quantisation block, value = map[code] * absmax (m: map_signed, v:
 * map_unsigned; 256 ascending f32 entries each, built by the host).  block_table: n_blocks rows of two int64 on the device, (element
 * offset into param / grad / half_out, a multiple of 4; code offset * 512 + length, 1 <= length <= 256); block b owns m_absmax[b] /
 * v_absmax[b].  A row that reaches outside [0, n) or [0, n_codes) is ignored.  Re-quantisation picks the NEAREST code, the lower index
 * on a tie.  A skipped step (clip_dev[2] != 0) leaves codes and absmax untouched and still clears the gradient.  No workspace. */
int32_t gn_adamw8_flat(gn_ctx* ctx, float* param, float* grad, int64_t n, void* m_codes, void* v_codes, int64_t n_codes, float* m_absmax,
                       float* v_absmax, const int64_t* block_table, int32_t n_blocks, const float* map_signed, const float* map_unsigned,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, const float* clip_dev,
                       float grad_scale, void* half_out, int32_t zero_grad);
/* VAE posterior sample of the train step (diffusion/train_controlnet_genima.py:1329-1332): moments [p, ld_moments] = (mean | logvar),
 * out[p, 0:C] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale, out[p, C:ld_out] = 0 */
int32_t gn_latent_sample(gn_ctx* ctx, const void* moments, const void* eps, void* out, int64_t pixels, int32_t C,
                         int32_t ld_moments, int32_t ld_eps, int32_t ld_out, float scale);
/* EMAModel.step of the InstructPix2Pix fine-tune (diffusion/train_instruct_pix2pix_genima.py:821-824, :1271-1272) on the flat fp32
 * buffers: shadow <- shadow - one_minus_decay * (shadow - param), f32 op order of diffusers' `s_param.sub_(one_minus_decay * (s_param - param))` */
int32_t gn_ema_flat(gn_ctx* ctx, float* shadow, const float* param, int64_t n, float one_minus_decay);
int32_t gn_cast_f32_f16(gn_ctx* ctx, const float* x, void* out, int64_t n);
int32_t gn_fill_f32(gn_ctx* ctx, float* x, int64_t n, float v);

/* ---- train-time augmentation on the device (diffusion/train_controlnet_genima.py:775-830, `--augmentations` colorjitter, blur, affine,
 * crop; README recipe crop,colorjitter) --
 * gn_color_jitter: torchvision ColorJitter's four adjust_* ops on [B, HW, ld] f16 RGB pixels in [0, 1], applied in `order`
 * (op ids 0 brightness, 1 contrast, 2 saturation, 3 hue = ColorJitter.get_params' fn_idx) with `factors[id]`; f32 colour math,
 * adjust_contrast's per-image grey mean by a deterministic two-stage sum.  out may alias x.
 * gn_gaussian_blur: torchvision gaussian_blur on NHWC f16 [B, H, W, C], C % 8 == 0: reflect padding by ksize / 2 (odd ksize 3..9,
 * H, W > ksize / 2) and a depthwise conv with the 2-D taps taps[i] * taps[j] of the host's ksize f32 1-D taps; f32 sums, no alias.
 * gn_affine_nearest: torchvision F.affine(NEAREST, fill=None) on NHWC f16 [B, H, W, C], C % 8 == 0, with one f32 inverse matrix
 * theta[6] for the batch: the affine grid and grid_sample(nearest, zeros, align_corners=False) source index (round half to even),
 * 0 outside the image; no alias.
 * gn_reflect_pad_crop: F.pad(mode="reflect", pad on all sides) + crop of the original H x W at (crop_i, crop_j). */
int64_t gn_color_jitter_workspace_bytes(int32_t B);
int32_t gn_color_jitter(gn_ctx* ctx, const void* x, void* out, int32_t B, int64_t HW, int32_t ld, const int32_t* order,
                        const float* factors, void* workspace);
int32_t gn_reflect_pad_crop(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t pad,
                            int32_t crop_i, int32_t crop_j);
int32_t gn_gaussian_blur(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ksize,
                         const float* taps);
int32_t gn_affine_nearest(gn_ctx* ctx, const void* x, void* out, int32_t B, int32_t H, int32_t W, int32_t C, const float* theta);

/* ---- dataset generation: the joint-action spheres (render/joint_marker.py:86-181 -- pyrender's flat-shaded textured uv_spheres on an
 * OpenGL context -- and the composite of render/render_data.py:282-307), ray-cast and composited in one launch per batch of views.
 * All pointers are device memory.  Per view b < B:
 *   cams[b]        18 f32: fx fy cx cy | camera-to-world pose 3x4 row-major, already in the OpenGL convention (-z forward, y up:
 *                  joint_marker.py:101-118 applied by the caller) | znear zfar
 *   spheres[b][s]  16 f32, s < S <= 8: world pose 3x4 row-major | radius | base colour factor r g b;  count[b] <= S of them are drawn
 *   tex_index[b][s] layer of atlas uint8 [T, th, tw, 4] (RGBA, row 0 = the image's top row)
 * Sample (u, v) in pixel (x, y): samples = 1: the centre; samples = 4: (x, y) + (.375, .125), (.875, .375), (.125, .625), (.625, .875).
 * Ray from the camera origin along pose * (dx, dy, -1), dx = (u - cx) / fx, dy = (cy - v) / fy (signed fx, fy).  Hit: the nearest front
 * intersection whose eye depth lies in [znear, zfar]; p = Rs^T (hit - centre); uv = (p.xy / radius + 1) / 2 with v = 0 at the texture's
 * BOTTOM row; bilinear fetch on texel centres, repeat wrap; sample colour = factor * texel / 255 in f32, white on a miss; pixel =
 * round-to-nearest(255 * mean of the samples).  white = all three channels 255 (the reference keys on the colour):
 *   full     uint8 [B, H, W, 3] = white ? bg : pixel
 *   rnd      uint8 [B, H, W, 3] = white ? bg2 : trunc(pixel * blend[b] + bg2 * (1 - blend[b]))  (f64, unfused, as numpy computes it)
 *   occupied uint8 [B, H, W]    = !white
 *   full_f16 / rnd_f16: the same two images as f16 NHWC-8 [n_tiled, 2H, 2W, 8] in the 2x2 camera tiling (genima_amd/tiling.py): view b is
 *            tile t = tile_index ? tile_index[b] : b -- image t / 4, tile row (t % 4) / 2, tile column t % 2; a view whose t is outside
 *            [0, 4 n_tiled) writes nothing -- each byte converted as gn_image_u8_to_f16 does (v / 255 * mul + add, channels 3..7 zero).
 * Every output may be NULL.  bg (needed by full*) and bg2 + blend (needed by rnd*) are uint8 [B, H, W, 3], or, with bg_tiled != 0, the
 * tiled uint8 [n_tiled, 2H, 2W, 3] frames addressed like the f16 outputs; bg_frames (with bg_tiled, instead of bg): a DEVICE array of n_tiled
 * device pointers to such tiled frames lying anywhere (the DataLoader's frame cache, as gn_gather_u8_to_f16's src). */
typedef struct gn_render_desc {
  const float* cams;
  const float* spheres;
  const int32_t* tex_index;
  const int32_t* count;
  const uint8_t* atlas;
  const uint8_t* bg;
  const uint8_t* bg2;
  const double* blend;
  const int32_t* tile_index;
  const uint8_t* const* bg_frames;
  uint8_t* full;
  uint8_t* rnd;
  uint8_t* occupied;
  void* full_f16;
  void* rnd_f16;
  int32_t B, S, H, W, T, th, tw, samples, bg_tiled, n_tiled;
  float full_mul, full_add, rnd_mul, rnd_add;
} gn_render_desc;
int32_t gn_render_spheres(gn_ctx* ctx, const gn_render_desc* d);

/* One random-background training batch of the ACT controller, DRAWN from trajectories instead of gathered from frames (genima_amd/replay.py
 * DeviceReplay(render=...); the reference's rlbench_data_rnd_bg tree, render/render_data.py:296-311: the joint-target spheres alpha-blended
 * over a random texture, no scene), one launch.  Tables, all on the device:
 *   cams f32 [N_obs * V][18], spheres f32 [N_obs * V][n_spheres][16], tex_index int32 [N_obs * V][n_spheres], count int32 [N_obs * V]:
 *              gn_render_spheres' per-view inputs for every observation and camera, row obs * V + v;  atlas uint8 [n_tex, th, tw, 4]
 *   bank       uint8 [NB][H][W][3]: the background textures
 *   qpos, action, obs_index, first_obs, last_tr, lang_tokens, episode, idx: as gn_replay_gather takes them (idx on the device, clamped)
 * Per sample b, n = idx[b], view v < V and frame-stack slot k < fs, with slot = (b * V + v) * fs + k and o(k) gn_replay_gather's:
 *   view o(k) * V + v is ray-cast exactly as gn_render_spheres does (samples in {1, 4}) and composited as its rnd output:
 *   pixel' = white ? bank[layer] : trunc(pixel * blend + bank[layer] * (1 - blend))   (f64, unfused)
 * layer and blend are a pure function of (seed, draw, slot); mix is gn_attn_dropout's, all integer arithmetic is uint32 and wraps:
 *   base  = mix(seed_lo ^ 0x6A09E667 ^ (draw * 0x9E3779B9)) ^ seed_hi
 *   s     = mix(base + slot * 0x85EBCA6B)
 *   layer = (uint64(mix(s ^ 0xC2B2AE35)) * NB) >> 32
 *   u     = mix(s ^ 0x27D4EB2F) >> 8                                   24 bits
 *   blend = alpha_blend + (1.0 - alpha_blend) * (u * 2^-24)           f64, unfused: in [alpha_blend, 1) up to the last rounding
 * Outputs:
 *   images[b][v * fs + k][H][W][0..7]  f16 = pixel' / 255 in channels 0..2 (gn_image_u8_to_f16 with mul 1, add 0, bit for bit), zeros in
 *                                      3..7; 16-byte aligned
 *   images_u8[b][v * fs + k][H][W][0..2]  pixel'; bg_layer int32 [B][V * fs] = layer; blend_out f64 [B][V * fs] = blend: optional (NULL: not
 *                                      written)
 *   low_dim_state, action_out, tokens_out: gn_replay_gather's, bit for bit
 * B <= 65535, V * fs <= 65535, n_spheres <= 8, NB >= 1, 0 <= alpha_blend <= 1.  Every table index is clamped into its table.  Eager only. */
typedef struct gn_replay_render_desc {
  const float* cams;
  const float* spheres;
  const int32_t* tex_index;
  const int32_t* count;
  const uint8_t* atlas;
  const uint8_t* bank;
  const float* qpos;
  const float* action;
  const int32_t* obs_index;
  const int32_t* first_obs;
  const int32_t* last_tr;
  const int32_t* idx;
  void* images;
  uint8_t* images_u8;
  int32_t* bg_layer;
  double* blend_out;
  float* low_dim_state;
  float* action_out;
  const int32_t* lang_tokens;
  const int32_t* episode;
  int32_t* tokens_out;
  int64_t N_obs;
  double alpha_blend;
  uint32_t seed_lo, seed_hi, draw;
  int32_t B, V, fs, T, S, A, N, N_ep, L_tok;              /* gn_replay_gather_desc's */
  int32_t n_spheres, H, W, n_tex, th, tw, samples, NB;   /* gn_render_desc's S, H, W, T, th, tw, samples; the bank's layers */
} gn_replay_render_desc;
int32_t gn_replay_render(gn_ctx* ctx, const gn_replay_render_desc* d);

/* Open-loop evaluation scores (genima_amd/openloop.py OpenLoopEval): a generated image against the rendered ground truth, and a predicted action
 * chunk against the demo's.  All three entry points write rows row0 .. row0 + n_valid - 1 of a result table of `rows` rows: sample b < n_valid writes row
 * row0 + b, samples b >= n_valid (the padding of a last batch) write nothing.  Eager only.  A refused call (NULL required pointer, B, V, H, W,
 * T <= 0, A < 2, n_valid outside [0, B], row0 < 0 or row0 + n_valid > rows, tiled with V != 4) launches nothing and leaves the outputs as they
 * were; n_valid == 0 is accepted and does nothing.
 *
 * gn_openloop_image_metrics, per (sample b, view v), in integer arithmetic:
 *   gen       uint8: tiled = 1 (V = 4): the pipeline's [B][2H][2W][3] output, view v = the tile at row v / 2, column v % 2 (the order
 *             GenimaACT.act_tiled untiles in);  tiled = 0: [B * V][H][W][3]
 *   gt        uint8 [B * V][H][W][3], occupied uint8 [B * V][H][W]: gn_render_spheres' `full` and `occupied`
 *   img_out   uint64 [rows][V][5], 8-byte aligned = (se_in, n_in, se_out, n_out, wrap_sq):
 *     se_in   = sum over the pixels with occupied != 0 and the 3 channels of (gen - gt)^2, as plain integers;  n_in = the number of those pixels
 *     se_out, n_out: the same over the pixels with occupied == 0
 *     wrap_sq = sum over ALL pixels and channels of ((d * d) & 255) with d = (gen - gt) & 255: numpy's uint8 arithmetic, so wrap_sq / (H W 3) is
 *               the `mse` of the reference's validation score (diffusion/train_controlnet_genima.py:642-650) for one view
 *   The entry point zeroes the rows it owns (on the ctx stream), then per-block partial sums are added with 64-bit vector atomics: integer
 *   addition is order-independent, so every run gives the same bits.  H * W * 3 < 2^31; B, V <= 65535.
 *
 * gn_openloop_action_metrics, per (sample b, chunk position t), one thread each:
 *   a_hat     f16, element (b, t, j) at a_hat[b * bs_hat + t * ld_hat + j] (gn_act_loss's addressing; ld_hat >= A);  actions f32 [B][T][A]
 *   joint_scale  f32 [A - 1] or NULL (= 1): the action std gives radians
 *   act_out   f32 [rows][T][2]:
 *     [0] = sum over j < A - 1 of joint_scale[j] * |a_hat[j] - actions[j]|: each term one f32 subtraction of the exactly converted half, one
 *           f32 multiplication, added in f32 in index order j = 0 .. A - 2 (no fused multiply-add), so the bits repeat
 *     [1] = 1.0 where (a_hat[A - 1] > 0) == (actions[A - 1] > 0.5), else 0.0: the gripper output is a logit (calculate_loss uses
 *           BCE-with-logits); a logit of exactly 0 counts as closed */
int32_t gn_openloop_image_metrics(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* occupied, uint64_t* img_out, int32_t B, int32_t V,
                                  int32_t H, int32_t W, int32_t tiled, int32_t row0, int32_t n_valid, int32_t rows);
int32_t gn_openloop_action_metrics(gn_ctx* ctx, const void* a_hat, int64_t ld_hat, int64_t bs_hat, const float* actions, const float* joint_scale,
                                   float* act_out, int32_t B, int32_t T, int32_t A, int32_t row0, int32_t n_valid, int32_t rows);

/* gn_openloop_sphere_metrics: where the generated spheres landed (row0, n_valid, rows as above: sample b writes the S * 17 values of each of its
 * views into row row0 + b).  Per (sample b < n_valid, view v, sphere s < S), integer sums over the pixels
 * (x, y), x0 <= x < x1, y0 <= y < y1, of the sphere's window, with local coordinates lx = x - x0, ly = y - y0:
 *   gen, gt, occupied   as gn_openloop_image_metrics takes them (tiled selects gen's layout);  cond uint8 [B * V][H][W][3]: the observation
 *             frames the render was drawn over (gn_render_spheres' bg)
 *   win       int32 [B * V][S][4] = (x0, y0, x1, y1), half-open, DEVICE memory, 4-byte aligned (genima_amd/render.py sphere_windows makes them;
 *             windows of different spheres may overlap, and then share pixels: every window is summed on its own)
 *   win_host  NULL, or a HOST copy of win.  With it the entry point checks every one of the B * V * S windows and refuses the call unless
 *             0 <= x0 <= x1 <= W, 0 <= y0 <= y1 <= H, x1 - x0 <= 256 and y1 - y0 <= 256.  Without it nothing can be refused by value; the
 *             kernel ALWAYS clamps what it reads: x0 into [0, W], x1 into [x0, min(W, x0 + 256)], y likewise with H -- for a window that
 *             passes the check this changes nothing, and no table value can make the kernel read or write outside its buffers.
 *   threshold int32 >= 0.  Per pixel: a_gen = max(0, sum_c |gen_c - cond_c| - threshold), a_gt = max(0, sum_c |gt_c - cond_c| - threshold)
 *   sph_out   uint64 [rows][V][S][17], 8-byte aligned:
 *     [0]       the window's area in pixels
 *     [1..4]    sum a_gen, sum a_gen lx, sum a_gen ly, sum a_gen (lx^2 + ly^2)
 *     [5..8]    the same four sums with a_gt
 *     [9]       n_occ = the number of window pixels with occupied != 0
 *     [10]      sum over those pixels and the 3 channels of (gen - gt)^2
 *     [11..13]  sum of gen's r, g, b over those pixels;  [14..16] the same of gt
 *   One workgroup owns one window and stores its 17 values itself (no atomics, no zeroing pass: an empty window stores 17 zeros), so every
 *   run gives the same bits.  A window holds at most 65 536 pixels and a column stays below 6.6e12.  Refused, launching nothing and leaving
 *   sph_out as it was: a NULL pointer other than win_host, B, V, H, W as gn_openloop_image_metrics bounds them, S outside [1, 8], threshold
 *   < 0, tiled with V != 4, n_valid outside [0, B], row0 < 0 or row0 + n_valid > rows, a misaligned win / win_host / sph_out, and a window
 *   that fails win_host's check.  n_valid == 0 is accepted and does nothing.  Eager only. */
int32_t gn_openloop_sphere_metrics(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* cond, const uint8_t* occupied, const int32_t* win,
                                   const int32_t* win_host, uint64_t* sph_out, int32_t B, int32_t V, int32_t H, int32_t W, int32_t S, int32_t tiled,
                                   int32_t threshold, int32_t row0, int32_t n_valid, int32_t rows);

/* gn_openloop_orientation: which orientation the generated spheres show.  The stripe texture is the only place the image carries a joint's
 * rotation (the hit point goes through the sphere's own frame, m = Rs^T Rc, into the texture), so per (sample b < n_valid, view v, sphere
 * slot s < S, candidate k < K) the TRUE sphere is re-drawn with its rotation turned by R_k and compared with the generated window (row0,
 * n_valid, rows as above: sample b writes the S * K * 4 values of each of its views into row row0 + b).
 *   gen, gt, occupied, win, win_host, tiled   as gn_openloop_sphere_metrics takes them: the same window clamp, the same optional host check
 *   cams      f32 [B * V][18], spheres f32 [B * V][S][16], tex_index int32 [B * V][S], count int32 [B * V], atlas uint8 [T][th][tw][4]
 *             (4-byte aligned), samples in {1, 4}: gn_render_spheres' per-view inputs; count and tex_index are clamped as the renderer
 *             clamps them (count into [0, S], tex_index into [0, T - 1])
 *   rot       f32 [K][9], DEVICE memory, 4-byte aligned, 1 <= K <= 64: K rotations R_k in the sphere's OWN frame, row-major.  Candidate k of
 *             sphere s is the view's sphere table with only sphere s's rotation Rs (pose elements [i * 4 + l], i, l < 3) replaced by
 *               Rs_k[i][l] = (float)((double)Rs[i][0] * R_k[0][l] + (double)Rs[i][1] * R_k[1][l] + (double)Rs[i][2] * R_k[2][l]),
 *             the sum added left to right without fused multiply-add.  Every other sphere, the centre, the radius, the factor and the
 *             texture stay, so occlusion is the real one, and an identity R_k reproduces the ground-truth pose.  A slot s >= count is not
 *             drawn: all its candidates are the unchanged view
 *   shift     int32 [B * V][S][2] = (dx, dy), DEVICE memory, 4-byte aligned, or NULL (= 0): gen is read at (x + dx, y + dy), so a generated
 *             sphere that sits a few pixels off is compared texture against texture.  The kernel clamps each component into [-127, 127]; a
 *             shifted position outside the view's own H x W (its own tile, when tiled) drops that pixel from the gen sums only
 *   ori_out   uint64 [rows][V][S][K][4], 8-byte aligned.  Over the window's pixels with occupied != 0 (a silhouette does not depend on the
 *             rotation, so every candidate sums over the same set), with c the candidate's rendered colour at the pixel -- gn_render_spheres'
 *             raw render before any composite, bit for bit (the two kernels share the drawing code and the compile flags):
 *     [0]     sum over the 3 channels of (c - gen)^2 over the pixels whose shifted position is inside;  [1] the number of those pixels
 *     [2]     sum over the 3 channels of (c - gt)^2;  [3] the number of pixels in [2]
 *   One workgroup owns one (window, candidate) and stores its four values itself (no atomics, no zeroing pass: an empty window stores four
 *   zeros), so every run gives the same bits.  A column stays below 65 536 * 195 075 = 1.3e10.  Refused, launching nothing and leaving
 *   ori_out as it was: a NULL pointer other than win_host / shift, the bounds gn_openloop_sphere_metrics puts on B, V, H, W, S, tiled, row0,
 *   n_valid and rows, B * V > 65535, K outside [1, 64], samples not 1 or 4, T, th or tw <= 0, a misaligned pointer, and a window that fails
 *   win_host's check.  n_valid == 0 is accepted and does nothing.  Eager only. */
int32_t gn_openloop_orientation(gn_ctx* ctx, const uint8_t* gen, const uint8_t* gt, const uint8_t* occupied, const int32_t* win, const int32_t* win_host,
                                const float* cams, const float* spheres, const int32_t* tex_index, const int32_t* count, const uint8_t* atlas,
                                const float* rot, const int32_t* shift, uint64_t* ori_out, int32_t B, int32_t V, int32_t H, int32_t W, int32_t S, int32_t K,
                                int32_t T, int32_t th, int32_t tw, int32_t samples, int32_t tiled, int32_t row0, int32_t n_valid, int32_t rows);

/* Open-loop scores of an execution mode (execution_horizon h, temporal_agg, m): what gn_action_ensemble would have executed at every step of
 * every held-out episode, replayed from the chunks an evaluation computes anyway.  Observations are teacher-forced, so a rollout with horizon h
 * uses exactly the chunks of the transitions at steps 0, h, 2h, ... of each episode.
 *
 * gn_openloop_exec_actions, per (transition n, action dimension a), one thread each:
 *   chunks    f16 [N][T][ld], ld >= A the row pitch, only the first A columns are read: row n is the chunk predicted at transition n
 *   first_tr  int32 [N], DEVICE memory: the index of the first transition of n's episode.  The kernel clamps it into [0, n]
 *   exec      f32 [N][A];  n_calls  int32 [N] or NULL: the number of taking-part calls
 *   With f = first_tr[n], the step s = n - f and the call that executes it starting at t = s - s % h, the taking-part calls are {t} without
 *   temporal_agg, and with it u = t - j h for j = floor((T - 1 - (s - t)) / h) .. 0, keeping u >= 0: oldest first.  Then
 *     exec[n][a] = sum_i w_i chunks[f + u_i][s - u_i][a] / sum_i w_i,   w_0 = 1, w_i = expf(-m i),
 *   in f32 throughout, accumulated from the oldest call to the newest: bit for bit the row gn_action_ensemble_f16 returns for step s when it is
 *   called at t = 0, h, 2h, ... with K = ceil(T / h) (K = 1 without temporal_agg) after a reset -- the two kernels share the weighted sum and
 *   the compile flags.  Every read of chunks stays inside rows first_tr[n] .. n.
 *
 * gn_openloop_exec_metrics, per transition n, one thread each:
 *   exec      f32 [N][A] (the above);  demo f32 [N][A]: the normalised demo action of each transition (row 0 of its chunk);  first_tr as above
 *   joint_scale  f32 [A - 1] or NULL (= 1)
 *   out       f32 [N][4]:
 *     [0] = sum over j < A - 1 of joint_scale[j] * |exec[n][j] - demo[n][j]|, as gn_openloop_action_metrics sums it (one f32 subtraction, one
 *           multiplication, one addition per term, in index order, no fused multiply-add)
 *     [1] = 1.0 where (exec[n][A - 1] > 0) == (demo[n][A - 1] > 0.5), else 0.0: gn_openloop_action_metrics' gripper rule
 *     [2] = the executed jump sum_j joint_scale[j] * |exec[n][j] - exec[n - 1][j]|, summed alike; 0 at an episode's first step (first_tr[n] >= n)
 *     [3] = the same jump of demo
 * Both are eager only, deterministic (plain loads and stores, no atomics) and order-independent.  Refused, launching nothing and leaving the
 * outputs as they were: a NULL pointer other than n_calls / joint_scale, N or T <= 0, A < 2, ld < A, h outside 1 .. T, m < 0 or NaN. */
int32_t gn_openloop_exec_actions(gn_ctx* ctx, const void* chunks, const int32_t* first_tr, float* exec, int32_t* n_calls, int32_t N, int32_t T,
                                 int32_t A, int32_t ld, int32_t h, int32_t temporal_agg, float m);
int32_t gn_openloop_exec_metrics(gn_ctx* ctx, const float* exec, const float* demo, const int32_t* first_tr, const float* joint_scale, float* out, int32_t N,
                                 int32_t A);
/* gn_openloop_exec_actions_samples: gn_openloop_exec_actions over the combined chunk of every transition (gn_action_ensemble_samples_f16 states
 * the combination): bit for bit the rows that entry returns when it is called at t = 0, h, 2h, ... of each episode after a reset.
 *   chunks   f16: sample r of transition n is [T][ld] from chunks + n * ns + r * ss (elements); an evaluation's [R][N] table has ns = T * ld,
 *            ss = N * T * ld
 *   pick_out int32 [N]: under medoid REQUIRED -- a first launch (one workgroup per transition, the shared pick) stores every transition's pick
 *            there and the replay launch reads it; under mean optional, filled with -1
 *   first_tr, exec, n_calls, h, temporal_agg, m as gn_openloop_exec_actions takes them.  Eager only.  Refused, launching nothing: what that entry
 *   refuses, plus R, R * T * A, inv_R, combine, alignment and overlapping strides as gn_action_ensemble_samples_f16 refuses them. */
int32_t gn_openloop_exec_actions_samples(gn_ctx* ctx, const void* chunks, int64_t ns, int64_t ss, int32_t R, float inv_R, int32_t combine,
                                         const int32_t* first_tr, float* exec, int32_t* n_calls, int32_t* pick_out, int32_t N, int32_t T, int32_t A,
                                         int32_t ld, int32_t h, int32_t temporal_agg, float m);

/* gn_openloop_triangulate: where the drawn spheres are in the WORLD.  Each sphere is triangulated from the centroids of the views that found
 * it and compared with its true centre; one launch over the finished tables of a run.  All pointers but the two host copies are device memory.
 *   sph       uint64 [N][V][S][17], 8-byte aligned: gn_openloop_sphere_metrics' table (columns 1..3 the generated mass and its x / y sums,
 *             5..7 the ground truth's)
 *   win       int32 [N][V][S][4], 4-byte aligned: the windows the table was summed over (only x0, y0 are read, as numbers)
 *   cams      f32 [N][V][18]: gn_render_spheres' camera tables
 *   slot      int32 [N][G][V]: the sphere slot s of view v that shows group g of transition n, or -1 (a group is one world point; slot s of two
 *             views need not be the same sphere).  The kernel reads a slot outside [0, S) as -1, so no table value can make it read outside
 *             its buffers
 *   centre    f64 [N][G][3], 8-byte aligned: the true world centre of each group
 *   slot_host, win_host   NULL, or HOST copies of slot and win.  With them the entry point refuses the call unless every slot lies in [-1, S)
 *             and every window has 0 <= x0 <= x1, 0 <= y0 <= y1 and at most 256 per side
 *   min_ratio f64 >= 0, min_det f64 > 0;  N >= 0, V in [2, 8], S in [1, 8], G in [1, 8], N * V * S * 17 < 2^31
 *   out       f64 [N][G][2][8], 8-byte aligned; kind 0 is the generated image, kind 1 the ground-truth render
 * Per (n, g, kind), one thread each, everything in f64 without fused multiply-add:
 *   used      view v is used when s = slot[n][g][v] >= 0 and, with gen_m / gt_m columns 1 / 5 of sph[n][v][s]:  kind 1: gt_m > 0;
 *             kind 0: gen_m > 0, gt_m > 0 and gen_m >= min_ratio * gt_m
 *   observation  u = x0 + sum_x / m + 0.5, v = y0 + sum_y / m + 0.5 with the kind's own three columns: the centroid in image coordinates, a
 *             pixel's centre at + 0.5 (gn_render_spheres' one-sample offset)
 *   ray       origin o = the camera position (the pose's translation column), direction d = pose * (dx, dy, -1) normalised, dx = (u - cx) / fx,
 *             dy = (cy - v) / fy (signed fx, fy): gn_render_spheres' ray through (u, v)
 *   point     x solves A x = b, A = sum (I - d d^T), b = sum (I - d d^T) o over the used views in index order: the least-squares closest
 *             point to the rays; x = adj(A) b / det(A) in one fixed order of operations
 *   [0]       the number of used views
 *   [1..3]    x
 *   [4]       |x - centre[n][g]|
 *   [5]       sqrt(mean over the used views of |(I - d d^T)(x - o)|^2): the RMS distance from x to the rays
 *   [6]       sqrt(mean over the used views of (u' - u)^2 + (v' - v)^2), (u', v') the projection of x: p = R^T (x - o), z = -p.z,
 *             u' = cx + fx p.x / z, v' = cy - fy p.y / z;  NaN when z <= 0 in a used view
 *   [7]       det(A) / (trace(A) / 3)^3: 0 for parallel rays, at most 1; 0 with fewer than two used views
 *   With fewer than two used views, or unless [7] >= min_det, the case is unsolved: [1..6] are NaN, [0] and [7] are still written.
 * Plain loads and stores, no atomics, no zeroing pass: every run gives the same bits.  Refused, launching nothing and leaving out as it was: a
 * NULL pointer other than the host copies, N < 0, V, S or G outside its range, min_ratio < 0 or NaN, min_det <= 0 or NaN, a misaligned
 * pointer, a host table that fails its check.  N == 0 is accepted and does nothing.  Eager only. */
int32_t gn_openloop_triangulate(gn_ctx* ctx, const uint64_t* sph, const int32_t* win, const float* cams, const int32_t* slot, const double* centre,
                                const int32_t* slot_host, const int32_t* win_host, double* out, double min_ratio, double min_det, int32_t N, int32_t V,
                                int32_t S, int32_t G);

/* The seed axis of an open-loop evaluation: a run repeated with R generator seeds keeps its sphere table and its chunks per seed, and these two
 * reduce over that axis -- how much of a score is the checkpoint and how much the noise draw.  One launch each over the finished tables of a
 * run; all pointers are device memory.
 *
 * gn_openloop_seed_spheres, per (transition n, view v, sphere s), one thread each, everything in f64:
 *   sph       uint64 [R][N][V][S][17], 8-byte aligned: gn_openloop_sphere_metrics' table per seed.  gen_m, sx, sy are columns 1..3 of seed r;
 *             gt_m, tx, ty columns 5..7, the same for every seed: seed 0's are read
 *   found     seed r is found when gen_m > 0, gt_m > 0 and gen_m >= min_ratio * gt_m (gn_openloop_triangulate's rule for the generated image)
 *   ct = (tx / gt_m, ty / gt_m), the true centroid;  c_r = (sx / gen_m, sy / gen_m), seed r's;  q_r = gen_m / gt_m
 *   out       f64 [N][V][S][8], 8-byte aligned, sums over the found seeds in seed order r = 0 .. R - 1:
 *     [0]     k, the number of found seeds
 *     [1], [2]  the bias m - ct, m = (sum c_r) / k
 *     [3]     the spread (sum |c_r - m|^2) / k, from a second pass over the seeds (not from sum x^2 - (sum x)^2 / k)
 *     [4]     (sum |c_r - ct|^2) / k, the mean squared shift;  |d|^2 = d.x d.x + d.y d.y
 *     [5]     the mean of q_r, (sum q_r) / k
 *     [6]     the population variance of q_r, (sum (q_r - [5])^2) / k, from the second pass too
 *     [7]     max over r of |c_r - ct|^2
 *   With k = 0 (a hidden sphere, or no seed found it) [1..7] are NaN and [0] is still written.
 *   Refused, launching nothing and leaving out as it was: a NULL or misaligned pointer, R outside [1, 64], N < 0, V outside [2, 8], S outside
 *   [1, 8], N * V * S * 17 >= 2^31, min_ratio < 0 or NaN.  N == 0 is accepted and does nothing.
 *
 * gn_openloop_seed_actions, per (transition n, chunk position t), one thread each, everything in f32:
 *   chunks    f16 [R][N][T][ld], ld >= A the row pitch, only the first A columns are read: the chunk each seed's image made the controller predict
 *   demo      f32 [N][T][A]: the normalised demo chunk;  joint_scale f32 [A - 1] or NULL (= 1)
 *   inv_R     (float)(1.0 / R), rounded once on the host (any other value is refused)
 *   With a_r[j] seed r's value widened to f32 and mean_j = (sum_r a_r[j]) * inv_R, the sum added in seed order:
 *   out       f32 [N][T][4]:
 *     [0] = sum over j < A - 1 of joint_scale[j] * |mean_j - demo[j]|: the error of the SEED-MEAN chunk, summed as gn_openloop_action_metrics
 *           sums its terms (one subtraction, one multiplication, one addition per term, in index order)
 *     [1] = 1.0 where (mean_{A-1} > 0) == (demo[A - 1] > 0.5), else 0.0: that kernel's gripper rule on the mean logit
 *     [2] = sum over j < A - 1 of joint_scale[j] * ((sum_r |a_r[j] - mean_j|) * inv_R): the mean absolute deviation across the seeds
 *     [3] = (sum_r e_r) * inv_R in seed order, e_r = seed r's own [0] of gn_openloop_action_metrics, computed with that kernel's operations in
 *           its order: bit for bit the f32 seed-order mean of that kernel's output over the same chunks
 *   Refused, launching nothing and leaving out as it was: a NULL pointer other than joint_scale, R outside [1, 64], N or T <= 0, A < 2, ld < A,
 *   N * T > 2^24, R * N * T * ld >= 2^31, inv_R other than (float)(1.0 / R), a misaligned pointer.
 * Both: plain loads and stores, no atomics, no zeroing pass, no fused multiply-add, no sqrt and no exp: every run gives the same bits.  Eager only. */
int32_t gn_openloop_seed_spheres(gn_ctx* ctx, const uint64_t* sph, double* out, double min_ratio, int32_t R, int32_t N, int32_t V, int32_t S);
int32_t gn_openloop_seed_actions(gn_ctx* ctx, const void* chunks, int32_t ld, const float* demo, const float* joint_scale, float* out, float inv_R,
                                 int32_t R, int32_t N, int32_t T, int32_t A);

/* Camera-pose and light perturbation of a batch of views (genima_amd/perturb.py, OpenLoopEval(perturb=...)): one launch warps every view by
 * its own homography, resamples it bilinearly and applies a per-channel gain and offset.  All pointers are device memory.
 *   src       uint8 [B][H][W][3], the views (B = samples x views);  dst uint8 [B][H][W][3], the result.  dst must not overlap src
 *   valid     uint8 [B][H][W] or NULL: 1 where the output pixel's sample point lies inside the source image, else 0
 *   n_revealed int32 [B] (4-byte aligned) or NULL: per view the number of pixels with valid == 0 -- border the source never showed.  Zeroed by
 *             the call on the ctx stream, then summed per workgroup and added with one integer atomicAdd each: order-independent, same bits
 *   M         f64 [B][9], 8-byte aligned: per view the row-major 3x3 matrix that takes an OUTPUT pixel to the SOURCE pixel (homogeneous)
 *   colour    f64 [B][6], 8-byte aligned: per view gain r g b | offset r g b, the offsets in levels of 0 .. 255
 * Per output pixel (x, y) of view b, in f64, every operation rounded once in the written order (no fused multiply-add):
 *    1. X = x + 0.5, Y = y + 0.5
 *    2. a = (M0 X + M1 Y) + M2
 *    3. c = (M3 X + M4 Y) + M5
 *    4. w = (M6 X + M7 Y) + M8
 *    5. if !(w > 0), or a, c or w is not finite: the pixel is (0, 0, 0), valid = 0 (it counts as revealed), and nothing below applies
 *    6. u = a / w, v = c / w
 *    7. valid = (0 <= u <= W and 0 <= v <= H)
 *    8. su = clamp(u - 0.5, -(W - 1), 2 (W - 1)), x0 = floor(su), tx = su - x0;  sv, y0, ty likewise from v and H;
 *       clamp(t, lo, hi) = t < lo ? lo : (t > hi ? hi : t)
 *    9. the column indices x0 and x0 + 1 are folded into the image by ONE reflection about the edge pixel's centre (torch's `reflect`):
 *       i < 0 -> -i, else i > W - 1 -> 2 (W - 1) - i; then clamped to [0, W - 1].  Rows likewise with H.
 *   10. per channel, p00 p01 (row y0) and p10 p11 (row y0 + 1) the four source bytes as f64, at the folded columns x0 and x0 + 1:
 *       top = p00 (1 - tx) + p01 tx,  bot = p10 (1 - tx) + p11 tx,  cc = top (1 - ty) + bot ty    ((1 - tx) and (1 - ty) rounded once each)
 *       t = cc gain[ch] + offset[ch];  out = rint(t > 0 ? (t > 255 ? 255 : t) : 0), half to even (a NaN t gives 0)
 * With M the identity, gain 1 and offset 0 the result is a copy, bit for bit: tx = ty = 0 and every product is exact.
 * Revealed border is MIRRORED scene, not what a moved camera would have seen there; `valid` and n_revealed say how much of it there is.
 * Refused, launching nothing and leaving the outputs as they were: a NULL ctx, src, dst, M or colour; B, H or W <= 0; B > 65535;
 * B * H * W * 3 >= 2^31; dst overlapping src (dst == src included); a misaligned M, colour or n_revealed.  Eager only. */
int32_t gn_view_perturb(gn_ctx* ctx, const uint8_t* src, uint8_t* dst, uint8_t* valid, int32_t* n_revealed, const double* M, const double* colour,
                        int32_t B, int32_t H, int32_t W);

/* gn_view_perturb's rule over the trainer's frames (genima_amd/data.py DataLoader(view_augment=...)): n frames of 2 x 2 tiled views
 * (tiling.py order: tile t at tile row t / 2, tile column t % 2), every tile an independent H x W view with its own matrix and colour row.
 * All pointers are device memory.  Exactly one source is given:
 *   src       uint8 [n][2H][2W][3], stacked frames, or
 *   frames    a DEVICE array (8-byte aligned) of n device pointers to such tiled frames: they may be 4-byte aligned, may repeat and may lie
 *             anywhere (the table gn_gather_u8_to_f16 and gn_render_desc::bg_frames read).  THE CALLER GUARANTEES that no output overlaps a
 *             frame; nothing here can check it.
 *   M         f64 [n][4][9], 8-byte aligned;  colour f64 [n][4][6], 8-byte aligned: indexed by frame i, then tile t
 * Output tile t of frame i is gn_view_perturb's rule, steps 1 to 10 above with the TILE's H and W, applied to source tile t of frame i with
 * M[i][t] and colour[i][t]: pixel (x, y) of the tile is pixel ((t % 2) W + x, (t / 2) H + y) of the frame, source and output alike.  The fold
 * of step 9 and the clamp of step 8 act INSIDE the tile: no sample ever reads a neighbouring tile.
 * Outputs, each may be NULL, at least one of dst and dst_f16 is not:
 *   dst       uint8 [n][2H][2W][3]: the warped and re-coloured tiled frames (gn_render_spheres takes them as bg with bg_tiled)
 *   dst_f16   f16 [n][2H][2W][8], 16-byte aligned: each byte dst would hold, converted as gn_image_u8_to_f16 converts it,
 *             (f16)((float)v / 255 * mul + add); channels 3 .. 7 are zero
 *   valid     uint8 [n][2H][2W]: step 7's valid of every pixel
 *   n_revealed int32 [n][4], 4-byte aligned: per (frame, tile) the number of pixels with valid == 0.  Zeroed by the call on the ctx stream,
 *             then summed per workgroup and added with one integer atomicAdd each: order-independent, same bits
 * With the identity matrix, gain 1 and offset 0 dst is a copy of the source and dst_f16 is gn_image_u8_to_f16 of it, bit for bit.  In
 * general dst, valid and n_revealed equal gn_view_perturb on the untiled views, put back into the tiling, bit for bit.
 * Refused, launching nothing and leaving the outputs as they were: a NULL ctx, M or colour; both of src and frames, or neither; dst and
 * dst_f16 both NULL; n, H or W <= 0; 4 n > 65535; n * 2H * 2W * 3 >= 2^31; a misaligned M, colour, frames, n_revealed or dst_f16; with
 * src, a dst that overlaps it (dst == src included); a mul or add that is not finite.  Eager only. */
int32_t gn_view_augment_tiled(gn_ctx* ctx, const uint8_t* src, const uint8_t* const* frames, uint8_t* dst, void* dst_f16, uint8_t* valid,
                              int32_t* n_revealed, const double* M, const double* colour, int32_t n, int32_t H, int32_t W, float mul, float add);

/* ---- op programs: record once, replay on the stream (eagerly or as a captured hipGraph) ---------------------------
 * The host classes (UNet2DConditionModel / ControlNetModel / AutoencoderKL / pipeline) lower a forward pass to a flat list of
 * the ops above with all buffers pre-allocated, so the 5-step denoise loop runs without returning to Python. */
int32_t gn_program_create(gn_ctx* ctx, gn_program** out);
int32_t gn_program_destroy(gn_program* p);
int32_t gn_program_add_gemm(gn_program* p, const gn_gemm_desc* d);
int32_t gn_program_add_attention(gn_program* p, const gn_attn_desc* d);
int32_t gn_program_add_tblock(gn_program* p, const gn_tblock_desc* d);
int32_t gn_program_add_conv3x3_gn(gn_program* p, const gn_conv3x3_gn_desc* d);
int32_t gn_program_add_conv3x3_patch(gn_program* p, const gn_conv3x3_patch_desc* d);
int32_t gn_program_add_groupnorm(gn_program* p, const gn_groupnorm_desc* d);
int32_t gn_program_add_tiny_block(gn_program* p, const void* x, const void* const w[3], const void* const bias[3], void* out, int32_t B,
                                 int32_t H, int32_t W, int32_t C);
int32_t gn_program_add_layernorm(gn_program* p, const void* x, const void* gamma, const void* beta, void* y, int64_t M,
                                 int32_t C, float eps);
int32_t gn_program_add_timestep_embedding(gn_program* p, const float* t, void* out, int32_t B, int32_t dim,
                                          int32_t flip_sin_to_cos, float freq_shift);
int32_t gn_program_add_scale_pad(gn_program* p, const void* x, void* out, int64_t pixels, int32_t C, int32_t Cpad,
                                 float scale);
int32_t gn_program_add_euler_step(gn_program* p, void* x, const void* eps, int64_t pixels, int32_t C, int32_t ld_eps,
                                  float sigma, float sigma_next);
int32_t gn_program_add_scale_cat_pad(gn_program* p, const void* x, const void* x2, void* out, int64_t pixels, int32_t C, int32_t ld1,
                                     int32_t C2, int32_t ld2, int32_t Cpad, float scale, float scale2);
int32_t gn_program_add_image_f16_to_u8(gn_program* p, const void* in, uint8_t* out, int64_t pixels, int32_t ld);
int32_t gn_program_add_image_u8_to_f16(gn_program* p, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad,
                                       float mul, float add);
/* stream control inside a program: ops recorded after gn_program_add_fork run on the program's second HIP stream (which first
 * waits for everything recorded before the fork) until gn_program_add_main switches back; gn_program_add_join makes the main
 * stream wait for the side stream.  Used to run the ControlNet next to the UNet encoder inside a denoise step (both only read the
 * scaled latents); also valid under hipGraph capture (fork / join become graph edges).  Partial replays (gn_program_run of a
 * sub-range) ignore them and run serially. */
int32_t gn_program_add_fork(gn_program* p);
int32_t gn_program_add_main(gn_program* p);
int32_t gn_program_add_join(gn_program* p);
int32_t gn_program_add_add(gn_program* p, const void* a, const void* b, void* out, int64_t n);
int32_t gn_program_add_add_multi(gn_program* p, const void* const* a, const void* const* b, void* const* out, const int64_t* n, int32_t count);
int32_t gn_program_add_add_noise(gn_program* p, const void* x0, const void* noise, const float* sqrt_ac, const float* sqrt_1mac,
                                 void* out, int32_t B, int64_t per_sample);
int32_t gn_program_add_act(gn_program* p, const void* x, void* out, int64_t n, int32_t act);
int32_t gn_program_add_film(gn_program* p, const void* x, void* out, const void* gamma, const void* beta, int64_t ld_film,
                            int64_t rows_per_film, int64_t rows, int32_t C, int32_t act);
int32_t gn_program_add_embedding(gn_program* p, const int32_t* ids, const void* tok, const void* pos, void* out,
                                 int32_t B, int32_t L, int32_t D);
int32_t gn_program_add_softmax_rows(gn_program* p, void* x, int64_t rows, int32_t cols, int32_t ld, float scale);
int32_t gn_program_add_maxpool3x3s2(gn_program* p, const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C);
int32_t gn_program_add_action_ensemble(gn_program* p, const void* chunk, int32_t chunk_f16, void* state, const int32_t* steps, const uint8_t* reset,
                                       float* out, int32_t B, int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m);
/* gn_action_ensemble_samples_f16 as a recorded op: exactly one op appended, none when refused.  Refused at record time, by this name: a NULL
 * program, whatever the launch refuses, and a guarded segment that is open (the op's state advances on every call, so no replay may skip it)
 * -- which no gn_program_add_* entry checks itself, hence the other name: those entries record inside a segment as they are told. */
int32_t gn_program_record_action_ensemble_samples(gn_program* p, const void* chunk, int64_t bs, int64_t ss, int32_t R, float inv_R, int32_t combine, void* state,
                                               const int32_t* steps, const uint8_t* reset, float* out, int32_t* pick_out, float* spread_out, int32_t B,
                                               int32_t T, int32_t A, int32_t ld, int32_t K, int32_t h, float m);
int32_t gn_program_add_image_normalize_u8(gn_program* p, const uint8_t* in, void* out, int64_t pixels, int32_t Cpad, float m0,
                                          float m1, float m2, float a0, float a1, float a2);
int32_t gn_program_add_gather_rows(gn_program* p, const void* x, const int32_t* idx, void* out, int32_t B, int32_t L, int32_t D);
int32_t gn_program_add_copy4d(gn_program* p, const void* in, void* out, const int64_t* sizes, const int64_t* in_strides,
                              const int64_t* out_strides, int32_t L);
int32_t gn_program_add_argmax_rows_i32(gn_program* p, const int32_t* x, int32_t* out, int32_t rows, int32_t cols);
int64_t gn_program_num_ops(const gn_program* p);
/* In-call tile tuning.  The reference has no counterpart (diffusers leaves kernel selection to cuDNN's own autotuner inside
 * `self.pipe(...)`, controller/agent/sd_controlnet_agent.py:67-76); here the tile / K split of a recorded gn_gemm op can be read back and
 * replaced, so that candidates are timed INSIDE the recorded call (cold operands, the neighbours' cache state) instead of in an isolated
 * hot loop.  get: GN_ERR_INVALID when op is not a gn_gemm.  set: `workspace` replaces the op's split-K scratch pointer (NULL keeps the
 * recorded one; a plan that splits K with neither is refused); refused on a captured program. */
int32_t gn_program_get_gemm(const gn_program* p, int64_t op, gn_gemm_desc* out);
int32_t gn_program_set_gemm_plan(gn_program* p, int64_t op, int32_t tile, int32_t splitk, void* workspace);
/* GroupNorm bridge plumbing of a recorded program: the consumer of a tensor is recorded AFTER its producer, so the producer's sink is attached
 * afterwards -- op = a recorded gn_gemm (index 0) or gn_add_multi (index = which of its tensors); and the statistics arena is cleared by a
 * memset op at the top of every replay */
int32_t gn_program_set_sink(gn_program* p, int64_t op, int32_t index, const gn_stats_sink* sink, int32_t channels);
/* attach norm_out to a recorded gn_gemm (the GroupNorm that reads its output is recorded after it) */
int32_t gn_program_set_norm_out(gn_program* p, int64_t op, const gn_norm_out* n);
int32_t gn_program_add_memset(gn_program* p, void* ptr, int64_t bytes);
int32_t gn_program_set_memset_bytes(gn_program* p, int64_t op, int64_t bytes); /* shrink a recorded memset to the bytes the program came to use */
int32_t gn_memset(gn_ctx* ctx, void* ptr, int64_t bytes);
/* sizeof() of the descriptor structs as the library was compiled (0 gn_gemm_desc, 1 gn_attn_desc, 2 gn_groupnorm_desc, 3 gn_tblock_desc,
 * 4 gn_conv3x3_gn_desc, 5 gn_stats_sink, 6 gn_norm_in, 7 gn_norm_out, 8 gn_conv3x3_patch_desc, 9 gn_replay_gather_desc, 10 gn_replay_render_desc): a host binding checks its own layout against these before the first call */
int64_t gn_desc_sizeof(int32_t which);
/* first..last (exclusive) op range; last < 0 = to the end */
int32_t gn_program_run(gn_program* p, int64_t first, int64_t last);
int32_t gn_program_capture(gn_program* p);   /* capture the whole program into a hipGraph on the ctx stream */
int32_t gn_program_launch(gn_program* p);    /* replay the captured graph */
/* Guarded segments: work whose inputs stay the same from call to call (the prompt's text tower and K / V projections, the time shifts of a
 * baked timestep table) is marked at record time and skipped while its inputs are unchanged -- its output buffers persist between replays.
 *   begin / end    mark the ops recorded in between as one segment (contiguous, not nested, at most 64); every segment starts enabled
 *   set_enabled    the caller's decision: only the caller knows whether the segment's inputs (and the weights behind it) changed
 * A FULL replay -- gn_program_run(p, 0, -1) and gn_program_launch -- skips the kernel ops of a disabled segment.  Stream markers (fork /
 * main / join) inside it still act -- except a fork whose side section has nothing left to run, which is not opened.  A replay of an explicit range (first > 0 or last >= 0) runs exactly the ops it names, whatever the
 * flags say.  gn_program_launch keeps one captured graph per set of flags it was launched with (captured on first use on the ctx stream);
 * gn_program_capture drops them all.  gn_program_last_run_ops: kernel ops issued by the last full replay.
 * gn_bytes_changed: one launch that compares `live` with the snapshot `seen` (16-byte aligned, bytes a multiple of 4), brings `seen` up to
 * date and writes 1 / 0 to the int32 `flag` in device memory. */
int32_t gn_program_begin_segment(gn_program* p, int32_t* seg_id);
int32_t gn_program_end_segment(gn_program* p);
int32_t gn_program_set_segment_enabled(gn_program* p, int32_t seg_id, int32_t enabled);
int64_t gn_program_last_run_ops(const gn_program* p);
int32_t gn_bytes_changed(gn_ctx* ctx, const void* live, void* seen, int64_t bytes, int32_t* flag);

/* ---- timing helper: HIP events on the ctx stream (bench.py's roofline leg) ------------------------------------- */
int32_t gn_event_create(void** ev);
int32_t gn_event_destroy(void* ev);
int32_t gn_event_record(gn_ctx* ctx, void* ev);
int32_t gn_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on stop */
int32_t gn_stream_synchronize(gn_ctx* ctx);

/* ---- ACT controller update (controller/method/genima_act.py:27-139, :348-422) ----------------------------
 * gn_film_bwd: backward of gn_film (act NONE / RELU): dx = dz (1 + gamma), with dz = dy * act'(z); optional copies dz and dz * x whose
 *   per-(batch, channel) column sums (gn_colsum_f32) are dbeta / dgamma.
 * gn_dropout: out = x * keep_mask * scale (inverted dropout, mask drawn by the caller; the backward is the same call on dy).
 * gn_cvae_sample / gn_cvae_bwd: z = mu + exp(logvar / 2) eps over info = [mu | logvar] rows (reparametrize, :64-68) and its backward
 *   plus the KL term's gradient (kl_scale = loss_scale * kl_weight / B).
 * gn_act_loss: calculate_loss (:115-139): out4 = (loss, l1, gripper BCE x 0.05, kl); d_a_hat = grad_scale * d(l1 + gripper)/d(a_hat);
 *   a_hat f16 [B][T_rows][ld_hat] (rows >= T and columns >= A are padding), actions f32 [B][T][A], is_pad u8 [B][T] or NULL.
 * gn_add_f32_to_f16: dst[b, c] += src[b, c] (f32 column sums into an f16 feature gradient). */
int32_t gn_film_bwd(gn_ctx* ctx, const void* dy, const void* x, const void* gamma, const void* beta, int64_t ld_film, int64_t rows_per_film,
                    int64_t rows, int32_t C, int32_t act, void* dx, void* dz, void* dzx);
int32_t gn_dropout(gn_ctx* ctx, const void* x, const uint8_t* keep_mask, void* out, int64_t n, float scale);
int32_t gn_cvae_sample(gn_ctx* ctx, const void* info, int64_t ld_info, const float* eps, void* z, int64_t ld_z, int32_t B, int32_t L);
int32_t gn_cvae_bwd(gn_ctx* ctx, const void* info, int64_t ld_info, const float* eps, const void* dz, int64_t ld_z, void* dinfo, int32_t B, int32_t L,
                    float kl_scale);
int32_t gn_act_loss(gn_ctx* ctx, const void* a_hat, int64_t ld_hat, int64_t bs_hat, const float* actions, const uint8_t* is_pad, const void* info,
                    int64_t ld_info, int32_t B, int32_t T, int32_t T_rows, int32_t A, int32_t L, float kl_weight, float grad_scale, float* out4,
                    void* d_a_hat);
int32_t gn_add_f32_to_f16(gn_ctx* ctx, const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int32_t B, int32_t C);
/* train-time ElasticTransform of the ACT policy (controller/method/genima_act.py:150-163): bilinear warp of NHWC f16 [B, H, W, C] by one
 * displacement field disp f32 [H][W][2] = (dx, dy) in pixels shared by the batch; samples outside the image read 0 */
int32_t gn_warp_bilinear(gn_ctx* ctx, const void* in, void* out, const float* disp, int32_t B, int32_t H, int32_t W, int32_t C);
/* the displacement field of that ElasticTransform (torchvision v2.ElasticTransform._get_params): noise f32 [2][H][W] on the device, plane 0
 * the dx draw and plane 1 the dy draw in [-1, 1) -> disp f32 [H][W][2] = (dx, dy) in pixels, the layout gn_warp_bilinear takes.  Each plane
 * is reflect-padded by ksize / 2 (one reflection: H, W > ksize / 2), convolved along W and then along H with the ksize host f32 taps
 * (odd ksize 3..129; f32 FMAs in tap order 0 .. ksize - 1, so two calls on one input give the same bits), and multiplied by scale_x
 * (plane 0) / scale_y (plane 1).  workspace: gn_elastic_field_workspace_bytes(H, W) of device memory, the plane between the two passes.
 * noise, disp (8-byte aligned) and workspace must not alias each other.  A refused call launches nothing and leaves disp as it was. */
int64_t gn_elastic_field_workspace_bytes(int32_t H, int32_t W);
int32_t gn_elastic_field(gn_ctx* ctx, const float* noise, float* disp, void* workspace, int32_t H, int32_t W, int32_t ksize, const float* taps,
                         float scale_x, float scale_y);

/* ---- data-parallel gradient exchange (SURVEY.md section 8b "comm"; replaces accelerate's DDP all-reduce under accelerator.backward,
 * diffusion/train_controlnet_genima.py:1216-1218, :1402-1405).  One communicator per (process, GPU); the RCCL unique id (128 bytes) is
 * created on rank 0 and carried to the other ranks by the caller.  gn_comm_allreduce_grads SUMS one flat f32 buffer over the ranks in
 * place -- RCCL reduce-scatter + all-gather (+ a small all-reduce for a tail shorter than nranks) on the communicator's own HIP stream,
 * ordered behind everything launched so far on ctx's stream -- and returns at once; gn_comm_wait makes ctx's stream wait for it.
 * wire_bf16 = 1 sends bf16 on the links (the sum then rounds to bf16: opt-in).  scratch: device memory of gn_comm_scratch_bytes(). */
typedef struct gn_comm gn_comm;
int32_t gn_comm_unique_id(void* id128);
int32_t gn_comm_init(gn_ctx* ctx, int32_t rank, int32_t nranks, const void* id128, gn_comm** out);
int32_t gn_comm_destroy(gn_comm* comm);
int64_t gn_comm_scratch_bytes(const gn_comm* comm, int64_t count, int32_t wire_bf16);
int32_t gn_comm_allreduce_grads(gn_comm* comm, float* buf, int64_t count, int32_t wire_bf16, void* scratch);
int32_t gn_comm_wait(gn_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* GENIMA_HIP_H */
