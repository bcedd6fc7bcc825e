"""CPU references for the per-kernel parity tests of the fine-tune step's loss, clip, AdamW, EMA, cast, column-sum and conv-backward layout
kernels of csrc/backward.hip (tests/test_train_step_ops_gpu.py, tests/test_train_step_ref_cpu.py).

TEST INFRASTRUCTURE ONLY, torch / numpy only: nothing here goes through genima_amd.  Conventions of tests/act_ops_ref.py: a ``*_terms``
function takes the working dtype first -- float64 gives the reference, float32 restates the kernel's f32 arithmetic for ``m32_of`` -- and
returns (value, sum of |terms|) or a list of such pairs; scalars enter as the f32 values the library receives.  The summation ORDER of an
f32 sum is not restated: its terms are added in f64 and the order is covered by the ``*_chain`` count, the longest chain of f32 additions
any term goes through, read off the kernel text (the line is named next to each count; lines of csrc/backward.hip unless stated).
The inputs of the tests are built here too, so that the CPU module can check the conditions they are chosen to meet."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from act_ops_ref import cdiv
from norm_bwd_ref import geglu_join, geglu_split

Tensor = torch.Tensor
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
F16_MAX = 65504.0


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def f32v(x) -> float:
    """The f32 value a c_float argument arrives as."""
    return float(np.float32(x))


def _c(x, dt) -> Tensor:
    """An f32-rounded scalar in the working dtype."""
    return torch.tensor(f32v(x), dtype=F32).to(dt)


def pick(fn, i: int):
    """fn returning a list of (value, terms) pairs -> the function returning pair i (for m32_of on one output)."""
    return lambda dt, *a, **kw: fn(dt, *a, **kw)[i]


# ---- gn_mse_loss ------------------------------------------------------------------------------------------------------------------------------
MSE_THREADS = 256 * 256  # gn_mse_loss: `const int blocks = 256`, 256 threads each (:1037, :1039)
MSE_SIZES = [1024, 65536 + 296, 3 * 65536 + 8]               # pixels * ld_pred: idle threads / 296 threads on a second trip / 3 trips + 8
MSE_LAYOUTS = [(4, 8, 4), (4, 8, 8), (4, 4, 4), (3, 8, 4)]   # (C, ld_pred, ld_target)
MSE_GRAD_SCALES = [1.0, 65536.0 / 4]                         # 1, and the trainer's loss_scale / grad_accum


def mse_inputs(n_elems: int, layout):
    """pred [pixels, ld_pred], target [pixels, ld_target] f16; the pad channels of both hold NaN (the kernel must not read them)."""
    Cc, ldp, ldt = layout
    assert n_elems % ldp == 0
    pixels = n_elems // ldp
    g = _gen(1, n_elems, Cc, ldp, ldt)
    pred, target = torch.full((pixels, ldp), NAN, dtype=F16), torch.full((pixels, ldt), NAN, dtype=F16)
    pred[:, :Cc], target[:, :Cc] = torch.randn(pixels, Cc, generator=g).to(F16), torch.randn(pixels, Cc, generator=g).to(F16)
    return pred, target


def mse_terms(dt, pred: Tensor, target: Tensor, Cc: int, grad_scale: float):
    """-> [(loss [1], sum |t|), (dpred [pixels, ld_pred], |dpred|)]: loss = mean over pixels * C of (pred - target)^2, dpred = grad_scale * 2 /
    (pixels C) * (pred - target), +0 in the pad channels.  f32: d, d * d and gs * d as the kernel's (:680, :681), the two host scalars as
    gn_mse_loss forms them (:1038, :1042: f32 quotients of the exactly converted count)."""
    pixels, ldp = pred.shape
    d = torch.zeros(pixels, ldp, dtype=dt)
    d[:, :Cc] = pred[:, :Cc].to(dt) - target[:, :Cc].to(dt)
    if dt == F64:
        inv, gs = 1.0 / (pixels * Cc), f32v(grad_scale) * 2.0 / (pixels * Cc)
    else:
        cnt = np.float32(float(pixels) * Cc)
        inv, gs = float(np.float32(1.0) / cnt), float(np.float32(grad_scale) * np.float32(2.0) / cnt)
    sq = (d * d).to(F64).sum() * inv
    dp = torch.tensor(gs, dtype=dt) * d
    return [(sq.reshape(1), sq.reshape(1)), (dp, dp.abs())]


def mse_chain(n_elems: int) -> int:
    trips = cdiv(n_elems, MSE_THREADS)  # :676  one `s += d * d` per grid-stride trip of a thread
    wave = 6                            # :683  wave_sum (common.h:87-94): four DPP folds, then (a + b) + (c + d) of the row totals
    lds = 3                             # :686  red[0] + red[1] + red[2] + red[3]
    second = 1                          # :693-696  sum_small_kernel adds the 256 partials in double; one rounding of (float)(s * scale)
    return trips + wave + lds + second


# ---- gn_sumsq_f32 -----------------------------------------------------------------------------------------------------------------------------
SUMSQ_S = 2048 * 256  # gn_sumsq_f32: `const int blocks = 2048` of 256 threads (:1050): the grid stride, in float4 on the aligned path
SUMSQ_ALIGNED = [1, 3, 4, 5, 5003, 4 * SUMSQ_S, 4 * (SUMSQ_S + 1) + 1, 4 * (2 * SUMSQ_S + 77) + 3, 4 * (3 * SUMSQ_S + 5) + 2]
SUMSQ_MISALIGNED = [5, 5003, SUMSQ_S + 100]
LOSS_SCALE = 65536.0


def sumsq_inputs(n: int) -> Tensor:
    """A unit Gaussian gradient times the loss scale, f32 [n]."""
    return torch.randn(n, generator=_gen(2, n)) * LOSS_SCALE


def sumsq_terms(dt, x: Tensor):
    xx = x.to(dt)
    s = (xx * xx).to(F64).sum().reshape(1)
    return s, s


def sumsq_chain(n: int, aligned: bool) -> int:
    if aligned:
        n4 = n >> 2
        unrolled = cdiv(n4 - SUMSQ_S, 2 * SUMSQ_S) if n4 > SUMSQ_S else 0  # :708  trips of `for (; i + stride < n4; i += 2 * stride)`
        thread = 2 * unrolled  # :710  `s0 += a.x * a.x + b.x * b.x`: the pair's sum, then onto s0
        thread += 1            # :712-715  the remainder load
        thread += 1            # :716  the scalar tail (onto s0)
    else:
        thread = cdiv(n, SUMSQ_S)  # :718  one `s0 += x[i] * x[i]` per trip
    combine = 2                    # :720  (s0 + s1) + (s2 + s3)
    wave = 6                       # :720  wave_sum (common.h:87-94)
    lds = 3                        # :723  red[0] + red[1] + red[2] + red[3]
    second = 1                     # :693-696  sum_small_kernel: double, one rounding of the float result
    return thread + combine + wave + lds + second


def sumsq_path(n: int, idx: int, aligned: bool) -> str:
    """Which load of sumsq_partial_kernel reads element ``idx`` of an n-element buffer: 'first' / 'second' (the two loads of the unrolled
    body, :709), 'remainder' (:713), 'tail' (:716) or 'misaligned' (:718)."""
    assert 0 <= idx < n
    if not aligned:
        return "misaligned"
    n4 = n >> 2
    if idx >= 4 * n4:
        return "tail"
    q = idx >> 2                      # float4 index; thread i0 = q % S reads i0, i0 + S (unrolled), i0 + 2S, ...
    if (q // SUMSQ_S) % 2 == 1:
        return "second"               # reached as i + stride of the unrolled trip at i = q - S (q < n4 is that trip's condition)
    return "first" if q + SUMSQ_S < n4 else "remainder"


def sumsq_plants(n: int, aligned: bool):
    """-> [(path name, index)]: one index on every load path the (n, alignment) has."""
    S = SUMSQ_S
    if not aligned:
        return [("misaligned", 1234), ("misaligned", n - 7)]  # a first-trip and (n > S) a second-trip element of the scalar loop
    assert n == 4 * (3 * S + 5) + 2
    return [("first", 4 * 12345 + 1), ("second", 4 * (S + 777) + 2), ("first", 4 * (2 * S + 3)), ("second", 4 * (3 * S + 4) + 3),
            ("remainder", 4 * (2 * S + 1000) + 3), ("tail", n - 1)]


# ---- gn_clip_coef -----------------------------------------------------------------------------------------------------------------------------
# (name, sumsq, max_norm, inv_scale)
CLIP_CASES = [("zero", 0.0, 1.0, 1.0 / 65536), ("tiny", 1e-12, 1.0, 1.0 / 65536), ("below", (0.9999 * 65536) ** 2, 1.0, 1.0 / 65536),
              ("above", (1.0001 * 65536) ** 2, 1.0, 1.0 / 65536), ("1e30", 1e30, 1.0, 1.0 / 65536), ("past 3e38", 1e37, 1.0, 1e20),
              ("inf", INF, 1.0, 1.0 / 65536), ("nan", NAN, 1.0, 1.0 / 65536)]
CLIP_NORM_ROUNDINGS = 3  # :753  sqrtf (<= 1 ulp = 2 half-ulps) and the product with inv_scale (1): in units of 2^-24 relative
CLIP_COEF_ROUNDINGS = 6  # :757  the norm's 3, norm + 1e-6f (1), the quotient (<= 1 ulp = 2)


def clip_terms(dt, sumsq: float, max_norm: float, inv_scale: float):
    """-> (coefficient, norm, found-inf flag) as Python floats, evaluated in ``dt`` from the f32 values of the three inputs (:753-757)."""
    f = np.float32 if dt == F32 else np.float64
    with np.errstate(all="ignore"):
        norm = f(np.sqrt(f(np.float32(sumsq)))) * f(np.float32(inv_scale))
        bad = bool(not (norm == norm) or norm > f(np.float32(3.0e38)))
        coef = f(0.0) if bad else min(f(1.0), f(np.float32(max_norm)) / (norm + f(np.float32(1e-6))))
    return float(coef), float(norm), 1.0 if bad else 0.0


# ---- gn_adamw_flat ----------------------------------------------------------------------------------------------------------------------------
ADAMW_HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
ADAMW_NS = [1, 255, 257, 5000]
ADAMW_STEPS = [1, 2, 3, 10, 1000]
ADAMW_WDS = [0.0, 1e-2]
ADAMW_GRAD_SCALES = [1.0, 1.0 / 65536]
ADAMW_CLIPS = [None, 0.37]
ADAMW_OFFSET = 3  # the odd element offset of the slices into the flat buffers (training.py: master[a:b], grad[a:b], half[a:b])


def adamw_inputs(n: int, grad_scale: float, seed: int = 0):
    """-> (p, g, m, v) f32 [n].  |g * grad_scale| log-uniform over 1e-6 .. 10 (sqrt(v) from far below eps's reach to far above it: eps inside
    the root would show), m / v a random state of that gradient's scale (v >= 0); half of the parameters ~1e-5 (far smaller than the step
    lr * m^ / sqrt(v^) ~ 1e-2: the step is then resolved far below p's own rounding), half ~1.  n >= 2: element 0 has g = m = v = 0 (update
    exactly 0, no 0 / 0), element 1 has |g * grad_scale| = 1e18 (gi^2 = 1e36 stays finite)."""
    gen = _gen(3, n, seed)
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 7.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).to(F64)
    gt = mag * sign
    m = (torch.randn(n, generator=gen, dtype=F64) * mag).to(F32)
    v = (torch.rand(n, generator=gen, dtype=F64) * mag * mag).to(F32)
    p = torch.randn(n, generator=gen) * torch.where(torch.arange(n) % 2 == 0, 1e-5, 1.0)
    if n >= 2:
        gt[0], m[0], v[0] = 0.0, 0.0, 0.0
        gt[1], m[1], v[1] = -1e18, 3e17, 2e35
    g = (gt / f32v(grad_scale)).to(F32)
    return p, g, m, v


def adamw_bias_corrections(beta1: float, beta2: float, step: int):
    """1 - beta^step in f64 from the f32 values of the betas (what torch.optim.AdamW computes in Python floats)."""
    return 1.0 - math.pow(f32v(beta1), step), 1.0 - math.pow(f32v(beta2), step)


def adamw_terms(dt, p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr, beta1, beta2, eps, wd, step: int, clip0=None, grad_scale: float = 1.0):
    """One decoupled-weight-decay Adam step (adamw_kernel, :737-746) -> [(m', T), (v', T), (update, T), (p', T)] with update = p' - p =
    -lr wd p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps).  The hyper-parameters are their f32 values; the bias corrections are formed in
    f64 and (dt = f32) rounded once.  The update's terms are the decay and the Adam step with m' at the magnitude of its two terms (the f32
    restatement forms the update without going through p: what p's rounding adds is p's to bound, not the update's)."""
    one = torch.ones((), dtype=dt)
    bc1, bc2 = (torch.tensor(b, dtype=F64).to(dt) for b in adamw_bias_corrections(beta1, beta2, step))
    gs = _c(grad_scale, dt) * (_c(clip0, dt) if clip0 is not None else one)  # :737
    gi = g.to(dt) * gs                                                       # :738
    m1, m2 = _c(beta1, dt) * m.to(dt), (one - _c(beta1, dt)) * gi            # :740
    v1, v2 = _c(beta2, dt) * v.to(dt), (one - _c(beta2, dt)) * gi * gi       # :741
    mi, vi = m1 + m2, v1 + v2
    denom = vi.sqrt() / bc2.sqrt() + _c(eps, dt)                             # :744
    adam = (_c(lr, dt) / bc1) * (mi / denom)                                 # :745
    adam_t = (_c(lr, dt) / bc1) * ((m1.abs() + m2.abs()) / denom)            # its magnitude before the two terms of m' cancel
    dec = p.to(dt) * (_c(lr, dt) * _c(wd, dt))
    upd = -dec - adam
    pn = p.to(dt) * (one - _c(lr, dt) * _c(wd, dt)) - adam                   # :739, :745
    return [(mi, m1.abs() + m2.abs()), (vi, v1.abs() + v2.abs()), (upd, dec.abs() + adam_t), (pn, p.to(dt).abs() + dec.abs() + adam_t)]


def adamw_p_rounding(p_old: Tensor, p_new: Tensor) -> Tensor:
    """What the two roundings of p add to the device's p' - p, in f64: p (1 - lr wd) with the f32 factor (its rounding: <= 2^-25, p's
    product: <= 2^-24 |p|, :739) and the final subtraction (<= 2^-24 |p'|, :745)."""
    return 2.0 ** -24 * (1.5 * p_old.to(F64).abs() + p_new.to(F64).abs())


# ---- gn_ema_flat ------------------------------------------------------------------------------------------------------------------------------
EMA_NS = [4, 1020, 1028]
EMA_OMDS = [1e-4, 0.5, 1.0]


def ema_f32(shadow: Tensor, param: Tensor, one_minus_decay: float) -> Tensor:
    """s - omd * (s - q), one rounded f32 operation at a time (ema_flat_kernel's __fsub_rn / __fmul_rn, :793)."""
    assert shadow.dtype == F32 and param.dtype == F32
    d = shadow - param
    t = torch.tensor(f32v(one_minus_decay), dtype=F32) * d
    return shadow - t


# ---- gn_cast_f32_f16 --------------------------------------------------------------------------------------------------------------------------
def cast_values():
    """-> dict of named f32 tensors: every non-negative finite f16 value h ('exact'), the midpoint of h and its successor h+ ('mid': a tie),
    the f32 values next to that midpoint ('below', 'above'), the negatives of all of them, and the named special values."""
    bits = torch.arange(0, 0x7C00, dtype=torch.int16)
    h = bits.view(F16).to(F32)
    lo, hi = h[:-1], h[1:]          # h and h+ (h = 65504 has no finite successor: 65520 is among the specials)
    mid = (lo + hi) / 2             # exact: 12 significant bits
    below, above = torch.nextafter(mid, torch.full_like(mid, -INF)), torch.nextafter(mid, torch.full_like(mid, INF))
    tiny = torch.tensor(2.0 ** -25, dtype=F32)
    special = torch.stack([torch.tensor(x, dtype=F32) for x in (F16_MAX, -F16_MAX, 65520.0, -65520.0, 0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1e-40, -1e-40,
                                                                 2.0 ** -126, 2.0 ** -25, -2.0 ** -25, 1e30, -1e30, INF, -INF, NAN)]
                          + [torch.nextafter(torch.tensor(65520.0), torch.tensor(0.0)), torch.nextafter(tiny, torch.tensor(0.0)),
                             torch.nextafter(tiny, torch.tensor(1.0))])
    return dict(exact=h, mid=mid, below=below, above=above, special=special)


def cast_input() -> Tensor:
    """All of cast_values (positive and negative), flat; the length is not a multiple of 256."""
    v = cast_values()
    pos = torch.cat([v["exact"], v["mid"], v["below"], v["above"]])
    x = torch.cat([pos, -pos, v["special"]])
    return x if x.numel() % 256 else torch.cat([x, torch.ones(1)])


# ---- gn_colsum_f32 ----------------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [(1, 1, 8, 8), (1, 63, 8, 16), (3, 65, 136, 136), (4, 130, 320, 328), (1, 9000, 136, 136), (1100, 128, 8, 8)]  # (nb, rows_per_batch, cols, ld)
COLSUM_FAMILIES = ["gauss", "cancel"]


def colsum_chunks(nb: int, rows_per_batch: int) -> int:
    """colsum_chunks (:887-894)."""
    return min(max(rows_per_batch // 64, 1), cdiv(1024, nb), 128)


def colsum_inputs(case, family: str) -> Tensor:
    """x f16 [nb * rows_per_batch, ld]; the pad columns hold NaN.  'cancel': each batch's rows are r, -r pairs (an odd row count: one more row
    of 1e-3-sized values), so every column sum is ~0 against sum |x| ~ rows."""
    nb, rpb, cols, ld = case
    g = _gen(4, nb, rpb, cols, ld)
    v = torch.randn(nb, rpb, cols, generator=g)
    if family == "cancel" and rpb > 1:
        half = rpb // 2
        v[:, half:2 * half] = -v[:, :half]
        v[:, 2 * half:] *= 1e-3
        v = v[:, torch.randperm(rpb, generator=g)]
    x = torch.full((nb * rpb, ld), NAN, dtype=F16)
    x[:, :cols] = v.reshape(nb * rpb, cols).to(F16)
    return x


def colsum_terms(dt, x: Tensor, nb: int, rows_per_batch: int, cols: int, prior=None):
    """out[b][c] = (prior[b][c] +) sum over batch b's rows of x[:, c] -> (value, sum |terms|) [nb, cols].  The f16 -> f32 conversions are exact:
    there is no term arithmetic, only the order of the additions (colsum_chain)."""
    v = x[:, :cols].to(dt).to(F64).view(nb, rows_per_batch, cols)
    s, a = v.sum(1), v.abs().sum(1)
    if prior is not None:
        s, a = s + prior.to(F64), a + prior.to(F64).abs()
    return s, a


def colsum_chain(nb: int, rows_per_batch: int) -> int:
    chunks = colsum_chunks(nb, rows_per_batch)
    rows_per = cdiv(rows_per_batch, chunks)  # :180
    thread = cdiv(rows_per, 16)              # :184  `for (r = r0 + ty; r < r1; r += 16)`: one `s[e] +=` per trip
    lds = 16                                 # :197  `a += red[i][t]`, 16 row lanes in turn
    second = cdiv(chunks, 4) + 4             # :213-226  reduce_rows_f32_kernel over R = chunks rows: a wave's rows, (s0 + s1) + (s2 + s3), the four
    return thread + lds + second             #           waves' (a + b) + (c + d), out + t (tests/test_small_ops_gpu.py uses the same count)


# ---- conv-backward layout helpers ---------------------------------------------------------------------------------------------------------------
# (B, H, W, C, k, stride, pad); the issue's (1, 7, 9, 16, 3, 2, 1) has B * Ho * Wo = 20, not a multiple of 8: B = 2 (40) is the nearest that is
IM2COL_CASES = [(1, 4, 6, 8, 3, 1, 1), (2, 5, 8, 72, 3, 1, 1), (2, 7, 9, 16, 3, 2, 1), (1, 6, 4, 8, 3, 1, 0), (2, 4, 4, 136, 1, 1, 0)]
POOL_CASES = [(2, 3, 5, 8), (1, 1, 1, 24), (3, 7, 2, 136)]  # (B, H, W, C)


def conv_out_hw(H: int, W: int, k: int, stride: int, pad: int):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def map_inputs(B: int, H: int, W: int, Cc: int, seed: int = 0) -> Tensor:
    return torch.randn(B, H, W, Cc, generator=_gen(5, B, H, W, Cc, seed)).to(F16)


def upsample_input(case) -> Tensor:
    """map_inputs with a -0 and two NaN payloads planted (zero insertion moves bits)."""
    x = map_inputs(*case, seed=1)
    xi = x.view(torch.int16).view(-1)
    xi[1], xi[5], xi[xi.numel() - 2] = -0x8000, 0x7E01, -0x1AB  # -0, NaN 0x7E01, NaN 0xFE55
    return x


def im2col_t_ref(x: Tensor, k: int, stride: int, pad: int) -> Tensor:
    """x f16 [B, H, W, C] -> f16 [k k C, B Ho Wo]: row tap * C + c (tap = dy * k + dx), column m = (b Ho + oy) Wo + ox holds
    x[b, oy stride - pad + dy, ox stride - pad + dx, c], +0 in the padding.  F.unfold (rows c * k k + tap), rearranged."""
    B, H, W, Cc = x.shape
    u = F.unfold(x.permute(0, 3, 1, 2).to(F32), k, padding=pad, stride=stride)  # [B, C k k, L]; f16 -> f32 -> f16 is the identity
    L = u.shape[-1]
    return u.view(B, Cc, k * k, L).permute(2, 1, 0, 3).reshape(k * k * Cc, B * L).to(F16)


def zero_upsample_ref(x: Tensor) -> Tensor:
    """[B, H, W, C] -> [B, 2H, 2W, C]: out[b, 2y, 2x] = x[b, y, x] (the bits), +0 elsewhere."""
    B, H, W, Cc = x.shape
    out = torch.zeros(B, 2 * H, 2 * W, Cc, dtype=x.dtype)
    out[:, 0::2, 0::2] = x
    return out


def sumpool_terms(dt, x: Tensor):
    """[B, 2H, 2W, C] -> the sum of each 2 x 2 block [B, H, W, C], added in the kernel's order (:657-663) -> (value, sum |terms|)."""
    v = x.to(dt)
    a, b, c, d = v[:, 0::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 0::2], v[:, 1::2, 1::2]
    return ((a + b) + c) + d, a.abs() + b.abs() + c.abs() + d.abs()


def pool_inputs(case, cancel: bool) -> Tensor:
    """[B, 2H, 2W, C] f16; cancel: in every second block the four values are (a, b, -a, -b + 2^-10-sized rest)."""
    B, H, W, Cc = case
    x = torch.randn(B, 2 * H, 2 * W, Cc, generator=_gen(6, B, H, W, Cc)).to(F16)
    if cancel:
        x[:, 1::2, 0::2] = torch.where(torch.arange(Cc) % 2 == 0, -x[:, 0::2, 0::2], x[:, 1::2, 0::2])
        x[:, 1::2, 1::2] = torch.where(torch.arange(Cc) % 2 == 0, (-x[:, 0::2, 1::2].float() * (1 + 2.0 ** -9)).to(F16), x[:, 1::2, 1::2])
    return x


# ---- gn_geglu_fwd -------------------------------------------------------------------------------------------------------------------------------
GEGLU_CASES = [(3, 8, 0), (3, 8, 8), (5, 96, 32), (7, 1280, 32), (64, 1024, 0)]  # (M, Hd, blk)


def finite_f16() -> Tensor:
    """Every finite f16 value once (both zeros included): 2 * 0x7C00 values."""
    bits = torch.arange(0, 0x7C00, dtype=torch.int16)
    return torch.cat([bits.view(F16), (bits | -0x8000).view(F16)])


def geglu_inputs(case) -> Tensor:
    """hg f16 [M, 2 Hd] in the case's layout.  |hidden| <= 0.99 (hidden * gelu(gate) stays a finite f16 for every finite gate); the gates are
    2 x unit Gaussians, and in (64, 1024, 0) the first 63488 of them are every finite f16 value, shuffled."""
    M, Hd, blk = case
    g = _gen(7, M, Hd, blk)
    hid = (torch.randn(M, Hd, generator=g) * 0.5).clamp(-0.98, 0.98).to(F16)
    gate = (torch.randn(M, Hd, generator=g) * 2).to(F16)
    if case == (64, 1024, 0):
        fin = finite_f16()
        gate.view(-1)[:fin.numel()] = fin[torch.randperm(fin.numel(), generator=g)]
    return geglu_join(hid, gate, blk)


def geglu_fwd_terms(dt, hg: Tensor, blk: int):
    """out = hidden * gelu(gate), gelu(z) = z (1 + erf(z / sqrt 2)) / 2 (common.h:66) -> (value, T = |hidden| |z| (1 + |erf|) / 2: the
    magnitude before 1 + erf cancels for z < 0)."""
    h, z = (t.to(dt) for t in geglu_split(hg, blk))
    er = torch.erf(z * torch.tensor(0.70710678118654752, dtype=dt))
    return h * (0.5 * z * (1.0 + er)), h.abs() * 0.5 * z.abs() * (1.0 + er.abs())
