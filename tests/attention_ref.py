"""CPU references and derived error bounds for the flash-attention backward (csrc/attention_bwd.hip) and for the output O and the
log2-domain lse of the forward kernels (attention.hip, attention_stream.hip, attention_pwg.hip): tests/test_attention_ref_cpu.py,
tests/test_attention_bwd_gpu.py, tests/test_attention_fwd_ref_cpu.py, tests/test_attention_fwd_gpu.py.

TEST INFRASTRUCTURE ONLY, in the manner of tests/act_ops_ref.py: torch f64 on the CPU, evaluated from the kernel's own f16 inputs; nothing
here goes through genima_amd.  Layouts are the kernels': q / o / d_o [B, Nq, heads * D], k / v [B, Nk_rows, heads * D] (rows >= Nk zero),
lse2 / delta [B, heads, Nq]; lse2 is in log2 units, P = exp2(s * scale * log2 e - lse2).
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from act_ops_ref import ulp16

Tensor = torch.Tensor
F64, F32, F16 = torch.float64, torch.float32, torch.float16
LOG2E = 1.4426950408889634
D = 64


def _heads(t: Tensor, heads: int, dt=F64) -> Tensor:
    """[B, N, heads * d] -> [B, heads, N, d]"""
    B, N, C = t.shape
    return t.to(dt).reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)


def _rows(t: Tensor) -> Tensor:
    """[B, heads, N, d] -> [B, N, heads * d]"""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def c_log2(scale: float, dt=F64) -> Tensor:
    """scale * log2 e as the kernels hold it: the f32 product of the f32 scale and 1.4426950408889634f."""
    return (torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)).to(dt)


# ---- forward -----------------------------------------------------------------------------------------------------------------------
def attn_fwd_ref(q: Tensor, k: Tensor, v: Tensor, heads: int, Nk: int, scale: float, causal: bool = False):
    """f64 softmax attention over keys [0, Nk) -> (O [B, Nq, C], lse2 [B, heads, Nq] in log2 units)."""
    qh, kh, vh = _heads(q, heads), _heads(k[:, :Nk], heads), _heads(v[:, :Nk], heads)
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=F64).triu(1)
    lse = torch.logsumexp(s, -1)
    return _rows(torch.exp(s - lse[..., None]) @ vh), lse * LOG2E


# ---- backward ----------------------------------------------------------------------------------------------------------------------
def _bwd(dt, q, k, v, d_o, o16, lse2, heads: int, Nk: int, scale: float, *, f16_operands: bool = False, store_f16: bool = False, plant: str = ""):
    """The backward's formulas in dtype ``dt``.  f64: the reference.  f32: the kernels' arithmetic restated -- f32 scores,
    exp2(fmaf(s, c, -L)), P and dS rounded to f16 (f16_operands), f32 accumulation, the result rounded to f16 (store_f16).
    ``plant``: one deliberate error (tests/test_attention_ref_cpu.py)."""
    qh, kh, vh, gh, oh = (_heads(t, heads, dt) for t in (q, k[:, :Nk], v[:, :Nk], d_o, o16))
    L = lse2.to(dt)[..., None]
    r16 = (lambda t: t.to(F16).to(dt)) if f16_operands else (lambda t: t)
    s = qh @ kh.transpose(-1, -2)
    if dt == F64:
        c = scale * LOG2E if plant != "scale_for_scale_log2" else scale
        P = torch.exp2(s * c - L)
    else:  # the fused multiply-add rounds once: the f32 x f32 product is exact in f64
        P = torch.exp2((s.to(F64) * c_log2(scale) - L.to(F64)).to(F32))
    if plant == "shift_key":  # the probabilities of key Nk // 2 land on its neighbour's row of K / V
        j = Nk // 2
        P = P.clone()
        P[..., [j, j - 1]] = P[..., [j - 1, j]]
    delta = (gh * oh).sum(-1)
    dP = gh @ vh.transpose(-1, -2)
    sc = torch.tensor(scale, dtype=F32).to(dt) if dt != F64 else scale
    dS = P * (dP - (0 if plant == "no_delta" else delta[..., None])) * sc
    P_v = P
    if plant == "trunc_p":  # (f16)P rounded toward zero
        p16 = P.to(F16)
        P_v = (p16.view(torch.int16) - (p16.to(dt) > P).to(torch.int16)).view(F16).to(dt)  # (positive values: the bit pattern below)
    if plant == "last_query_row":  # the last live query row never reaches dK / dV
        P_v, dS_k = P_v.clone(), dS.clone()
        P_v[..., -1, :], dS_k[..., -1, :] = 0, 0
    else:
        dS_k = dS
    P16, dS16, dS16k = r16(P_v), r16(dS), r16(dS_k)
    out = SimpleNamespace(delta=delta, dq=_rows(dS16 @ kh), dk=_rows(dS16k.transpose(-1, -2) @ qh), dv=_rows(P16.transpose(-1, -2) @ gh))
    if store_f16:
        out.dq32, out.dk32, out.dv32 = out.dq, out.dk, out.dv
        out.dq, out.dk, out.dv = (t.to(F16).to(dt) for t in (out.dq, out.dk, out.dv))
    if dt == F64 and not plant:
        aq, ak, av, ag, ao = qh.abs(), kh.abs(), vh.abs(), gh.abs(), oh.abs()
        out.delta_ab = (ag * ao).sum(-1)
        # what the f32 arithmetic added up on the way to dS: the dot products behind dP and delta, before they cancel
        dS32 = P * ((ag @ av.transpose(-1, -2)) + out.delta_ab[..., None]) * scale
        out.dq_ab, out.dq_ab32, out.dq_b = _rows(dS.abs() @ ak), _rows(dS32 @ ak), _rows(ak.sum(-2, keepdim=True).expand_as(qh))
        out.dk_ab, out.dk_ab32, out.dk_b = (_rows(dS.abs().transpose(-1, -2) @ aq), _rows(dS32.transpose(-1, -2) @ aq),
                                            _rows(aq.sum(-2, keepdim=True).expand_as(kh)))
        out.dv_ab, out.dv_b = _rows(P.transpose(-1, -2) @ ag), _rows(ag.sum(-2, keepdim=True).expand_as(kh))
        out.dv_ab32 = out.dv_ab
    return out


def attn_bwd_ref(q, k, v, d_o, o16, lse2, heads: int, Nk: int, scale: float, plant: str = ""):
    """f64 backward from the f16 inputs and the o16 / lse2 THE KERNEL IS GIVEN (not recomputed ones):
        P = exp2(s scale log2e - lse2), delta = sum_d dO O, dP = dO V^T, dS = scale P (dP - delta), dV = P^T dO, dK = dS^T Q, dQ = dS K.
    -> namespace: dq [B, Nq, C], dk / dv [B, Nk, C], delta [B, heads, Nq], and per output element x = sum_i a_i b_i the magnitude sums
    x_ab = sum |a_i| |b_i| (sum |dS| |K|, sum |dS| |Q|, sum |P| |dO|), x_b = sum |b_i| (the column sums sum |K|, sum |Q|, sum |dO|),
    x_ab32 = x_ab with |dS| replaced by scale P (sum_d |dO| |V| + sum_d |dO| |O|), and delta_ab = sum_d |dO| |O|."""
    return _bwd(F64, q, k, v, d_o, o16, lse2, heads, Nk, scale, plant=plant)


def emulate_bwd_f32(q, k, v, d_o, o16, lse2, heads: int, Nk: int, scale: float, f16_operands: bool = True):
    """The kernels' arithmetic on the CPU (see _bwd); dq / dk / dv rounded to f16, the values before that store in dq32 / dk32 / dv32.
    It exists to fix M32 and to show that the bound's form is met by plain f32 evaluation; no GPU test compares against it."""
    return _bwd(F32, q, k, v, d_o, o16, lse2, heads, Nk, scale, f16_operands=f16_operands, store_f16=True)


# ---- bounds of the backward ----------------------------------------------------------------------------------------------------------
# An output element is x = sum_i a_i b_i with the left operand a (P for dV, dS for dK and dQ) rounded to f16 by the kernel, the products
# accumulated in f32 and the sum stored as f16:
#     |got - ref| <= 1/2 ulp16(ref)            the store: x32 rounds to the nearest f16
#                  + 2^-11 sum |a_i| |b_i|     a_i -> f16, unit roundoff 2^-11 for a normal a_i
#                  + 2^-25 sum |b_i|           ... and half the subnormal spacing 2^-24 for |a_i| < 2^-14 (whichever applies is below the sum
#                                              of the two); at 1024 keys a typical dS is 1e-4 and most of them are subnormal in f16
#                  + M32 sum32 |a_i| |b_i|     everything f32: the order of the score / dP / delta / output sums, the hardware exp2, the
#                                              fused multiply-add in front of it.  For dK / dQ sum32 takes |dS| before the cancellation in
#                                              dP - delta (x_ab32 above): an f32 error of dP is relative to sum_d |dO| |V|, not to |dP - delta|.
# M32 by the convention of act_ops_ref.m32_of: the largest |f32 evaluation - f64| / sum32 of emulate_bwd_f32(f16_operands=False) before
# its store, over every case of bwd_cases(), times 4 for what the CPU restatement does not have (the device's v_exp_f32 at 1 ulp, the
# MFMA's accumulation order).  Measured (tests/test_attention_ref_cpu.py::test_m32_is_four_times_the_measured_f32_error prints and pins
# them; the worst cases are the q x 4 family, where |s c - lse2| reaches 70 and one f32 ulp of it is 4e-6 of P):
#     dq 6.67e-7, dk 7.63e-7, dv 4.43e-6.          Never taken from a GPU run.
M32_MEASURED = {"dq": 6.67e-7, "dk": 7.63e-7, "dv": 4.43e-6}
M32 = {n: 4 * m for n, m in M32_MEASURED.items()}


def bwd_bounds(ref) -> dict:
    """{name: bound tensor} for dq, dk, dv and delta of an attn_bwd_ref result."""
    out = {}
    for n in ("dq", "dk", "dv"):
        x, ab, ab32, b = getattr(ref, n), getattr(ref, n + "_ab"), getattr(ref, n + "_ab32"), getattr(ref, n + "_b")
        out[n] = 0.5 * ulp16(x) + 2.0 ** -11 * ab + 2.0 ** -25 * b + M32[n] * ab32
    # delta: an f32 sum of 64 f16 x f16 products (each exact in f32), one chain of 64 additions
    out["delta"] = 64 * 2.0 ** -24 * ref.delta_ab
    return out


def assert_within(got: Tensor, ref: Tensor, bound: Tensor, what: str = "") -> float:
    """Every element: |got - ref| <= bound.  Prints and returns the largest err / bound."""
    got, ref = got.detach().cpu().to(F64), ref.detach().to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err/bound {ratio:.3f}, max |err| {float(err.max()):.3e}")
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), (f"{what}: |got - ref| {float(err.flatten()[worst]):.6e} > bound {float(bound.flatten()[worst]):.6e} at flat index "
                                        f"{worst} of {tuple(got.shape)} (got {float(got.flatten()[worst])!r}, ref {float(ref.flatten()[worst])!r}); "
                                        f"{int((err > bound).sum())} elements out")
    return ratio


def assert_bwd(got: dict, ref, what: str = "", names=("delta", "dq", "dk", "dv")) -> dict:
    """got: {name: tensor}; every element of every named output within bwd_bounds(ref).  All outputs are looked at before it raises."""
    bounds, ratios, failed = bwd_bounds(ref), {}, []
    for n in names:
        try:
            ratios[n] = assert_within(got[n], getattr(ref, n), bounds[n], f"{what} {n}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return ratios


# ---- the lse bound, from the forward kernels' code -------------------------------------------------------------------------------------
# All three kernels (attention.hip both V layouts, attention_stream.hip, attention_pwg.hip) compute, per query row,
#     q' = f16(f32(q) * c),  c = f32(scale) * 1.4426950408889634f            (qf[] in each kernel: "exponent units straight out of the MFMA")
#     s'_j = sum_d k_jd q'_d - m                                             (f32 MFMA, -m as the accumulator's initial value)
#     p_j = exp2(s'_j) (v_exp_f32), l = sum_j p_j, lse2 = m + log2(l) (v_log_f32)
# with m a maximum of some of the row's own scores (so l >= 1 up to rounding) that the fallbacks re-reference once per 32 or 64 keys.
#   (1) q -> q' is a rounding of the INPUT by up to 2^-11 per element, i.e. up to 2^-11 sum_d |c q_d k_jd| per score: 3.6e-3 log2 units in the
#       worst case on unit Gaussians, above the suite's old 2e-3 bar.  It is a deterministic function of q and c, so it is not bounded but
#       evaluated: shift = |lse2_f64(q', k) - lse2_f64(q, k)| exactly.  This is the bound the code implies; what it does to dQ / dK / dV
#       is tested in tests/test_attention_bwd_gpu.py::test_forward_feeds_backward.
#   (2) p_sum_f16 (attention.hip and attention_stream.hip: v_dot2c_f32_f16 on the packed pairs that enter P.V): l is the sum of the
#       probabilities ALREADY ROUNDED to f16 -> relative 2^-11 of l, plus 2^-25 per key for p_j below 2^-14 (against l >= 1):
#       log2e (2^-11 + n 2^-25).  attention_pwg.hip adds the f32 exponentials (add_f32 in its half-stages, acc += e0 + e1 in exps): no such term.
#   (3) f32, in units of 2^-24, with A = max_j sum_d |k_jd q'_d| >= |m|, |s'_j + m|:
#       65 products-and-init per score, relative to sum |k q'| + |m|                              -> 130 A
#       m_run += delta and negm -= delta kept apart in the fallbacks, once per 32 keys            -> 2 (n / 32) A
#       v_exp_f32 at 1 ulp (2 x 2^-24) per p_j; alpha = exp2(-delta) and l *= alpha per 32 keys   -> log2e (2 + 3 n / 32)
#       the row sum: at most n additions in a chain (a dot2 counts as two)                        -> log2e n
#       v_log_f32 at 1 ulp of |log2 l| <= |lse2| + A; the last addition and the f32 store         -> 2 (|lse2| + A) + 2 |lse2|
# The same bound holds after the optimistic softmax's fallback: it is the same arithmetic with m tracked.


def lse2_bound(q: Tensor, k: Tensor, heads: int, Nk: int, scale: float, *, p_sum_f16: bool, causal: bool = False):
    """-> (lse2 reference, per-row bound), both [B, heads, Nq] f64.  (One (batch, head) at a time: the existing forward tests call this
    at 4096 x 4096.)"""
    B, Nq = q.shape[0], q.shape[1]
    qh, kh = _heads(q, heads), _heads(k[:, :Nk], heads)
    q1 = _heads((q.to(F32) * c_log2(scale, F32)).to(F16), heads)
    mask = torch.full((Nq, Nk), float("-inf"), dtype=F64).triu(1) if causal else 0.0
    lse_ref, lse_q1, A = (torch.empty(B, heads, Nq, dtype=F64) for _ in range(3))
    for b in range(B):
        for h in range(heads):
            kt = kh[b, h].t()
            lse_ref[b, h] = torch.logsumexp((qh[b, h] @ kt).mul_(scale).add_(mask), -1) * LOG2E
            lse_q1[b, h] = torch.logsumexp((q1[b, h] @ kt).add_(mask).div_(LOG2E), -1) * LOG2E
            # (an upper bound is all that is needed of A: f32, a little raised)
            A[b, h] = (q1[b, h].abs().to(F32) @ kt.abs().to(F32)).amax(-1).to(F64) * (1 + 1e-5)
    n = Nk
    f32_part = 2.0 ** -24 * ((130 + 2 * n / 32) * A + LOG2E * (2 + 3 * n / 32 + n) + 2 * (lse_ref.abs() + A) + 2 * lse_ref.abs())
    f16_part = LOG2E * (2.0 ** -11 + n * 2.0 ** -25) if p_sum_f16 else 0.0
    return lse_ref, (lse_q1 - lse_ref).abs() + f16_part + f32_part


# which forward variant sums what (gn_attention_set_variant: 0 attention.hip, 4 attention_stream.hip, 5 attention_pwg.hip)
P_SUM_F16 = {0: True, 4: True, 5: False}


def assert_lse2(lse: Tensor, q: Tensor, k: Tensor, heads: int, Nk: int, scale: float, *, p_sum_f16: bool = True, causal: bool = False,
                what: str = "lse") -> float:
    """Every element of a forward kernel's lse within lse2_bound of the f64 value."""
    ref, bound = lse2_bound(q.detach().cpu(), k.detach().cpu(), heads, Nk, scale, p_sum_f16=p_sum_f16, causal=causal)
    print(f"{what}: bound median {float(bound.median()):.3e} max {float(bound.max()):.3e}")
    return assert_within(lse, ref, bound, what)


# ---- the forward's O: centre, bound, restatement ---------------------------------------------------------------------------------------------
# Every forward kernel (attention.hip in all its instantiations, attention_stream.hip, attention_pwg.hip) stores, per query row,
#     o = f16((sum_j p16_j v_j) * (1 / l)),   p16_j = f16(exp2(s'_j)),   s'_j = sum_d k_jd q'_d - m,   q' = f16(f32(q) c)
# with l = sum_j p16_j (v_dot2c_f32_f16 on the packed pairs: attention.hip, attention_stream.hip) or l = sum_j exp2(s'_j) (attention_pwg.hip)
# and m a maximum over some of the row's own keys (the first tile's, moved by the careful path; or the diagonal tile's, held fixed; after a
# flagged tile or block the max-tracking loop), so l >= 1 up to rounding: the key that gave m has p = 1.
#
# CENTRE.  O1 = the f64 attention of (q', k, v) with weights 2^(q'.k).  q -> q' is a deterministic function of the input (lse2_bound (1)), so
# the primary assertion is centred on what the code computes from q' and not widened by it; the distance |O1 - O(q)| to the function's value is
# evaluated and added only in the second assertion (assert_fwd_o prints its share).
#
# B1, per element, n = the row's live keys (under causal min(Nk, row + 1)), u = 2^-11, P_j the f64 weights of O1:
#   (a) 1/2 ulp16(O1)                                         the store
#   (b) min(U, Cn)                                            P -> f16 at unit roundoff u, in the numerator and in l
#         U  = u o_ab + (u + n 2^-25) |O1|,  o_ab = sum_j P_j |v_j|     numerator and denominator taken apart
#         Cn = 2 u / (1 - u) sum_j P_j |v_j - O1|                       ... together: where l is the sum of THE SAME f16 values that enter P.V the
#              weights p16_j / l sum to one exactly, o - O1 = sum_j (w_j - P_j)(v_j - O1) and each weight is off by at most 2 u / (1 - u) of
#              itself.  Valid for P_SUM_F16 kernels only; attention_pwg.hip sums the f32 exponentials and gets U alone.
#   (c) 2^-25 o_b,  o_b = sum_{j live} |v_j|                  half the f16 subnormal spacing per key for p_j < 2^-14, against l >= 1
#   (d) f32, in units of 2^-24 and relative to o_ab + |O1| (attention_dropout_ref.fwd_bound (3) without its inv_keep): the score behind each
#       p_j is off by (130 + 2 n / 32) A log2 units (lse2_bound (3)), ln 2 times that relative to p_j; v_exp_f32 at 1 ulp (2); alpha and the
#       two rescales once per 32 keys at most (3 n / 32); the P.V and row-sum chains (2 n); the pair sum of l, the division (2.5 ulp allowed:
#       5) and the product (7 in all); a split pwg block adds one addition per accumulator and one for l, the merge through LDS (2).
# No term is fitted to a device result.  What the bound cannot see (it is a worst-case bound): P rounded toward zero instead of to nearest, and
# O rounded to f16 before the division on zero-mean V, sit at 0.3 .. 1.0 of it (tests/test_attention_fwd_ref_cpu.py asserts that they do).
LN2 = 0.6931471805599453
PLIM = 8192.0  # attention_common.h: a lane sum of P beyond this re-references the row (attention.hip) or redoes the block (stream, pwg)


def q_prime(q: Tensor, scale: float) -> Tensor:
    """f16(f32(q) * c): the Q fragments as every forward kernel holds them."""
    return (q.to(F32) * c_log2(scale, F32)).to(F16)


def _dead(Nq: int, Nk: int, causal: bool) -> Tensor:
    return torch.ones(Nq, Nk, dtype=torch.bool).triu(1) if causal else torch.zeros(Nq, Nk, dtype=torch.bool)


def _centred_sum(P: Tensor, vv: Tensor, o1: Tensor) -> Tensor:
    """sum_j P_j |v_jd - o1_d| [Nq, d] from f64 P [Nq, Nk], vv [Nk, d], o1 [Nq, d].  (Only an upper bound is needed: f32 in row chunks, a
    little raised -- test_kernels_gpu.py calls this at 4096 x 4096.)"""
    Nq, Nk = P.shape
    P32, v32, o32 = P.to(F32), vv.to(F32), o1.to(F32)
    out = torch.empty(Nq, vv.shape[1], dtype=F32)
    step = max(1, (1 << 22) // max(1, Nk * vv.shape[1]))
    for r in range(0, Nq, step):
        dev = (v32[None] - o32[r:r + step, None]).abs_()
        out[r:r + step] = torch.bmm(P32[r:r + step, None], dev)[:, 0]
    return out.to(F64) * (1 + 1e-5)


def fwd_o_bound(q: Tensor, k: Tensor, v: Tensor, heads: int, Nk: int, scale: float, *, p_sum_f16: bool, causal: bool = False,
                split: bool = False):
    """-> namespace of f64 [B, Nq, C] tensors: o = O(q) (attn_fwd_ref's), o1 (the centre), b1 (the bound on |kernel - o1|), shift = |o1 - o|
    (the bound on |kernel - o| is b1 + shift), and the terms o_ab, o_b, var (item (b)), f32 (item (d)).  One (batch, head) at a time."""
    B, Nq, C = q.shape
    d = C // heads
    qh, kh, vh = _heads(q, heads), _heads(k[:, :Nk], heads), _heads(v[:, :Nk], heads)
    q1 = _heads(q_prime(q, scale), heads)
    dead = _dead(Nq, Nk, causal)
    mask = torch.zeros(Nq, Nk, dtype=F64).masked_fill_(dead, float("-inf"))
    live = (~dead).to(F64)
    n = live.sum(-1)[None, None, :, None]
    o, o1, o_ab, o_b, cn = (torch.zeros(B, heads, Nq, d, dtype=F64) for _ in range(5))
    A = torch.empty(B, heads, Nq, 1, dtype=F64)
    for b in range(B):
        for h in range(heads):
            kt, vv = kh[b, h].t(), vh[b, h]
            o[b, h] = torch.softmax((qh[b, h] @ kt).mul_(scale).add_(mask), -1) @ vv
            P = torch.softmax((q1[b, h] @ kt).mul_(LN2).add_(mask), -1)
            o1[b, h], o_ab[b, h], o_b[b, h] = P @ vv, P @ vv.abs(), live @ vv.abs()
            A[b, h, :, 0] = (q1[b, h].abs() @ kt.abs()).masked_fill_(dead, 0.0).amax(-1)  # over the row's live keys
            if p_sum_f16:
                cn[b, h] = _centred_sum(P, vv, o1[b, h])
    u = 2.0 ** -11
    var = u * o_ab + (u + n * 2.0 ** -25) * o1.abs()
    if p_sum_f16:
        var = torch.minimum(var, 2 * u / (1 - u) * cn)
    f32 = 2.0 ** -24 * (LN2 * (130 + 2 * n / 32) * A + 2 + 3 * n / 32 + 2 * n + 7 + (2 if split else 0)) * (o_ab + o1.abs())
    out = SimpleNamespace(o=_rows(o), o1=_rows(o1), o_ab=_rows(o_ab), o_b=_rows(o_b), var=_rows(var), f32=_rows(f32))
    out.b1 = 0.5 * ulp16(out.o1) + out.var + 2.0 ** -25 * out.o_b + out.f32
    out.shift = (out.o1 - out.o).abs()
    return out


def assert_fwd_o(o: Tensor, ref, what: str = "o") -> float:
    """A forward kernel's O against a fwd_o_bound result: every element within b1 of the centre o1 (the primary assertion) and within
    b1 + |o1 - O(q)| of the function's value O(q).  Prints the bound in f16 ulps and the shift's share; -> the largest err / b1."""
    share = ref.shift / ref.b1
    print(f"{what}: b1 median {float((ref.b1 / ulp16(ref.o1)).median()):.2f} f16 ulps; |O1 - O(q)| / b1 median {float(share.median()):.3f} max {float(share.max()):.2f}")
    ratio = assert_within(o, ref.o1, ref.b1, f"{what} vs O1")
    assert_within(o, ref.o, ref.b1 + ref.shift, f"{what} vs O(q)")
    return ratio


def _toward_zero(p: Tensor) -> Tensor:
    """(f16)p rounded toward zero, p >= 0: the bit pattern below where round-to-nearest went up."""
    p16 = p.to(F16)
    return (p16.view(torch.int16) - (p16.to(p.dtype) > p).to(torch.int16)).view(F16)


def emulate_fwd_f32(q: Tensor, k: Tensor, v: Tensor, heads: int, Nk: int, scale: float, *, causal: bool = False, walk: str = "first",
                    p_sum_f16: bool = True, tile: int = 64, split: bool = False, plant: str = "") -> Tensor:
    """The forward kernels' arithmetic in torch f32 / f16 on the CPU -> o [B, Nq, C] f16.  q' = f16(q c), f32 scores minus the reference,
    p16 = f16(exp2(s')), l = sum p16 (p_sum_f16) or sum exp2(s'), f32 P.V per ``tile`` keys (64; 32: the sub-tile order of attention_pwg.hip
    and of the redo loops), o = f16(O * (1 / l)).  The reference walk:
      "first"  attention.hip: the first tile's row maximum sets m; masked tiles and tiles whose row sums leave PLIM take the careful path
               (m moves up, O and l are rescaled), every other tile is optimistic (no maximum taken);
      "track"  every tile careful: the max-tracking loop the stream and pwg kernels fall back to;
      "diag"   attention_stream.hip / attention_pwg.hip: m = the row maximum over the diagonal tile min(row // 64, tiles - 1), held fixed;
               ``split``: the two key halves accumulate (O, l) apart, against the same m, and are added at the end.  A row sum beyond PLIM
               anywhere redoes everything with "track" at 32 keys, as the kernels do.
    It exists to show that the form of fwd_o_bound is met by plain evaluation (and to carry the planted errors of
    tests/test_attention_fwd_ref_cpu.py: ``plant``); no GPU test compares against it."""
    B, Nq, C = q.shape
    d = C // heads
    if plant == "scale_for_scale_log2":
        q1 = (q.to(F32) * torch.tensor(scale, dtype=F32)).to(F16)
    else:
        q1 = q_prime(q, scale)
    qh, kh, vh = _heads(q1, heads, F32), _heads(k[:, :Nk], heads, F32), _heads(v[:, :Nk], heads, F32)
    dead = _dead(Nq, Nk, causal)
    if plant == "causal_off_by_one":  # key >= row dead (row 0 keeps its key: a row without keys is another matter)
        dead = torch.ones(Nq, Nk, dtype=torch.bool).triu(0)
        dead[0, 0] = False
    if plant == "drop_last_key":      # the last key of a ragged tile
        dead = dead.clone()
        dead[:, Nk - 1] = True
    def p16_of(p):
        if plant == "trunc_p":
            return _toward_zero(p)
        p16 = p.to(F16)
        if plant == "flush_subnormal_p":
            p16 = torch.where(p16 < 2.0 ** -14, torch.zeros_like(p16), p16)
        return p16

    S = qh @ kh.transpose(-1, -2)  # [B, heads, Nq, Nk], all (batch, head) problems at once

    def walk_keys(lo, hi, mode, step, m_fixed=None):
        """-> (O [B, heads, Nq, d], l [B, heads, Nq], flagged) over the keys [lo, hi)."""
        m = torch.zeros(B, heads, Nq, dtype=F32) if m_fixed is None else m_fixed
        l, O = torch.zeros(B, heads, Nq, dtype=F32), torch.zeros(B, heads, Nq, d, dtype=F32)
        flagged, planted = False, False
        for t, j0 in enumerate(range(lo, hi, step)):
            sl = slice(j0, min(j0 + step, hi))
            s, dm = S[..., sl] - m[..., None], dead[:, sl]
            careful = mode == "track" or (mode == "first" and (t == 0 or j0 + step > Nk or bool(dm.any())))
            if not careful:
                p = torch.exp2(s.masked_fill(dm, float("-inf")))
                over = not bool((p16_of(p).to(F32).sum(-1) <= PLIM).all())
                flagged |= over and mode == "diag"
                careful = over and mode == "first"
            if careful:
                s = s.masked_fill(dm, float("-inf"))
                mx = s.amax(-1)
                delta = torch.where(mx == float("-inf"), torch.zeros_like(mx), mx if t == 0 else mx.clamp_min(0.0))
                alpha = torch.exp2(-delta)
                m, l = m + delta, l * alpha
                if plant == "no_alpha_on_o" and t > 0 and not planted and bool((delta > 0).any()):
                    planted = True  # O keeps the old reference on this one re-reference; l moves
                else:
                    O = O * alpha[..., None]
                p = torch.exp2(s - delta[..., None])
            p16 = p16_of(p)
            if plant == "drop_key_last_row" and sl.start <= Nk // 2 < sl.stop:  # one key never reaches the last live query row
                p16, p = p16.clone(), p.clone()
                p16[..., Nq - 1, Nk // 2 - sl.start], p[..., Nq - 1, Nk // 2 - sl.start] = 0, 0
            l = l + (p16.to(F32) if p_sum_f16 else p).sum(-1)
            O = O + p16.to(F32) @ vh[..., sl, :]
        return O, l, flagged

    if walk == "diag":
        assert Nk % 64 == 0 and not causal, "the stream / pwg kernels take whole unmasked tiles only"
        nt = Nk // 64
        tref = (torch.arange(Nq) // 64).clamp_max(nt - 1)
        Sm = S.masked_fill(dead, float("-inf"))
        m = Sm.reshape(B, heads, Nq, nt, 64).amax(-1).gather(-1, tref[None, None, :, None].expand(B, heads, Nq, 1))[..., 0]
        if split:
            O, l, f0 = walk_keys(0, Nk // 2, "diag", tile, m)
            m2 = m
            if plant == "split_refs_differ":  # the second half takes its own first tile as the reference; the merge adds as before
                m2 = Sm[..., Nk // 2:Nk // 2 + 64].amax(-1)
            O2, l2, f1 = walk_keys(Nk // 2, Nk, "diag", tile, m2)
            O, l, flagged = O + O2, l + l2, f0 or f1
        else:
            O, l, flagged = walk_keys(0, Nk, "diag", tile, m)
        if flagged:
            O, l, _ = walk_keys(0, Nk, "track", 32)
    else:
        O, l, _ = walk_keys(0, Nk, walk, tile)
    if plant == "early_o_round":  # O rounded to f16 before the division
        O = O.to(F16).to(F32)
    out = (O * (1.0 / l)[..., None]).to(F16)
    return _rows(out)


# ---- the cases of the forward tests (tests/test_attention_fwd_ref_cpu.py, tests/test_attention_fwd_gpu.py) ------------------------------------
# kernel -> (gn_attention_set_variant, D, row-major V).  Variants 1 / 2: attention.hip's 4 waves x 64 rows / 8 waves x 32 rows (256-row blocks).
FWD_KERNELS = {"att64": (0, 64, False), "att64_vrow": (0, 64, True), "att32": (0, 32, False), "block1": (1, 64, False), "block2": (2, 64, False),
               "stream": (4, 64, False), "pwg": (5, 64, False)}
# shapes (B, heads, Nq, Nk): the smallest at which each piece of decode or control flow is live
FWD_ATT64 = [(1, 1, 8, 8), (1, 2, 128, 64),
             (1, 2, 136, 72),     # second block with 8 live rows, a ragged tile of 8 keys, the NaN pads cleared in LDS
             (2, 3, 200, 77),
             (1, 2, 40, 200),     # optimistic middle tiles, ragged last
             (2, 4, 128, 128),    # 8 blocks: the XCD remap is taken
             (1, 3, 384, 192),    # 9 blocks: the remap is not taken
             (1, 1, 8, 1024)]
FWD_ATT64_CAUSAL = [(1, 2, 77, 77), (1, 2, 136, 136),  # nk_eff differs per block
                    (1, 1, 264, 264), (1, 1, 136, 72), (1, 1, 8, 136)]
FWD_ATT32 = [((1, 2, 8, 8), False), ((1, 2, 136, 72), False), ((1, 2, 40, 259), False),  # five register-staged tiles
             ((2, 2, 77, 77), True), ((1, 1, 136, 136), True)]
FWD_BLOCK256 = [((1, 1, 256, 64), False), ((1, 2, 264, 136), False), ((1, 1, 264, 264), True)]
FWD_STREAM = [(1, 1, 8, 128), (1, 2, 128, 128), (1, 2, 136, 192),
              (1, 2, 320, 128),   # the reference-tile clamp, Nq > Nk
              (2, 4, 128, 256),   # remap
              (1, 3, 384, 192), (1, 1, 128, 1024)]
FWD_PWG_FULL = [(1, 1, 256, 128), (1, 2, 320, 128),  # ragged rows
                (1, 1, 512, 448),   # seven tiles
                (1, 1, 512, 128)]   # clamp
FWD_PWG_SPLIT = [(1, 1, 256, 512), (2, 3, 256, 512),  # 12 split blocks
                 (1, 4, 256, 512),   # 8 split blocks, remap taken
                 (1, 1, 512, 1024)]
FWD_PWG_MIXED = [(1, 257, 256, 512),  # 256 full blocks plus the last head as two split blocks
                 (3, 86, 256, 512)]   # 258 blocks whose remainder is no whole head: none may split
FWD_FAMILIES = ["gauss", "sharp", "spike", "qzero", "vconst", "vpos", "voffset"]
# where the families beside gauss run: one ragged, one causal, one stream, one split and one 256-row case
FWD_FAMILY_CASES = [("att64", (1, 2, 136, 72), False), ("att64", (1, 2, 136, 136), True), ("stream", (1, 2, 136, 192), False),
                    ("pwg", (1, 1, 256, 512), False), ("pwg", (1, 2, 320, 128), False)]


def fwd_cases():
    """[(kernel, (B, heads, Nq, Nk), causal, family)]"""
    plain = ([(kn, s, False) for s in FWD_ATT64 for kn in ("att64", "att64_vrow")] + [(kn, s, True) for s in FWD_ATT64_CAUSAL for kn in ("att64", "att64_vrow")]
             + [("att32", s, c) for s, c in FWD_ATT32] + [(kn, s, c) for s, c in FWD_BLOCK256 for kn in ("block1", "block2")]
             + [("stream", s, False) for s in FWD_STREAM] + [("pwg", s, False) for s in FWD_PWG_FULL + FWD_PWG_SPLIT + FWD_PWG_MIXED])
    return [(kn, s, c, "gauss") for kn, s, c in plain] + [(kn, s, c, f) for f in FWD_FAMILIES[1:] for kn, s, c in FWD_FAMILY_CASES]


def fwd_case_id(case) -> str:
    kn, s, causal, family = case
    return f"{kn}-" + "x".join(str(i) for i in s) + ("-causal" if causal else "") + f"-{family}"


def pwg_split_heads(B: int, heads: int, Nq: int, Nk: int) -> int:
    """gn_launch_attention_pwg's split rule restated: how many of the LAST heads run as split blocks (128 rows, two key halves).  The remainder
    r of the 256-row block count over rounds of 256 splits, in whole heads, if 0 < r <= 128, Nq is a multiple of 256 and the tile count is
    even and at least 8."""
    nqb = (Nq + 255) // 256
    r, ntiles = (nqb * heads * B) % 256, Nk // 64
    if not (0 < r <= 128 and Nq % 256 == 0 and ntiles % 2 == 0 and ntiles >= 8):
        return 0
    return r // (B * nqb)


def fwd_inputs(case, seed: int = 0):
    """-> (q [B, Nq, C], k, v [B, Nk, C]) f16 of a forward case, D from its kernel."""
    kn, (B, heads, Nq, Nk), causal, family = case
    return make_inputs((B, heads, Nq, Nk, Nk), family, seed, d=FWD_KERNELS[kn][1])[:3]


_FWD_REFS: dict = {}


def fwd_ref_of(key: str, q, k, v, heads: int, Nk: int, scale: float, **kw):
    """fwd_o_bound of a problem, computed once under ``key`` and shared (leave it unchanged)."""
    if key not in _FWD_REFS:
        _FWD_REFS[key] = fwd_o_bound(q, k, v, heads, Nk, scale, **kw)
    return _FWD_REFS[key]


# the fallback constructions: scaled-down forms of tests/test_kernels_gpu.py's far_tile / one_row / every_tile, (B, heads) = (2, 3), D = 64
def fallback_inputs(where: str, Nq: int, Nk: int):
    """-> (q, k, v f16, intended): keys that beat a row's diagonal-tile reference by tens of log2 units, so that the stream and pwg kernels
    redo the block; intended = (batch elements, head, rows) whose excess the tests assert from the f64 scores (fallback_excess)."""
    B, heads = 2, 3
    C = heads * D
    g = torch.Generator().manual_seed(7 + Nq + Nk)
    q = torch.randn(B, Nq, C, generator=g)
    k, v = torch.randn(B, Nk, C, generator=g), torch.randn(B, Nk, C, generator=g)
    if where == "far_tile":    # one key of the last tile (the second key half) aligned with every query of head 0
        dd = torch.randn(D, generator=g)
        dd = dd / dd.norm()
        q[:, :, :D] += 6.0 * dd
        k[:, Nk - 40, :D] = 50.0 * dd
        intended = ([0, 1], 0, list(range(0, min(Nq, Nk - 64))))
    elif where == "one_row":   # a single query row with one huge key in the first tile (the first key half)
        row = Nq - 60
        k[0, 37, D:2 * D] = 12.0 * q[0, row, D:2 * D]
        intended = ([0], 1, [row])
    else:                      # the maximum keeps growing along the keys for all rows of head 2
        assert where == "every_tile", where
        dd = torch.randn(D, generator=g)
        dd = dd / dd.norm()
        q[:, :, 2 * D:] = 0.3 * q[:, :, 2 * D:] + 8.0 * dd
        k[:, :, 2 * D:] = 0.3 * k[:, :, 2 * D:] + torch.linspace(-4.0, 4.0, Nk)[None, :, None] * dd * 3.0
        intended = ([0, 1], 2, list(range(0, min(Nq, 64 * (3 * (Nk // 64) // 8)))))
    return q.to(F16), k.to(F16), v.to(F16), intended


def fallback_excess(q: Tensor, k: Tensor, heads: int, scale: float) -> Tensor:
    """[B, heads, Nq] f64: by how many log2 units a row's largest score q'.k exceeds its diagonal-tile reference (the maximum over the keys
    of tile min(row // 64, tiles - 1)).  More than 14 puts a probability above 2^14 > PLIM: the block's flag is set."""
    Nq, Nk = q.shape[1], k.shape[1]
    s = _heads(q_prime(q, scale), heads) @ _heads(k, heads).transpose(-1, -2)
    nt = Nk // 64
    tiles = s.reshape(*s.shape[:-1], nt, 64).amax(-1)                      # [B, heads, Nq, tiles]
    tref = (torch.arange(Nq) // 64).clamp_max(nt - 1)
    ref = tiles.gather(-1, tref[None, None, :, None].expand(*s.shape[:-1], 1))[..., 0]
    return s.amax(-1) - ref


# (kernel, block kind, where, Nq, Nk): split blocks need 256 | Nq and an even tile count >= 8; 448 keys are seven tiles (256-row blocks)
FWD_FALLBACKS = ([("stream", "128", w, 256, 256) for w in ("far_tile", "one_row", "every_tile")]
                 + [("pwg", "split", w, 256, 512) for w in ("far_tile", "one_row", "every_tile")]
                 + [("pwg", "256", w, 448, 448) for w in ("far_tile", "one_row", "every_tile")])


# ---- the cases of the backward tests (shared by the CPU and the GPU module, so that M32 is measured on what the GPU tests run) ----------
# (B, heads, Nq, Nk, Nk_rows)
BWD_SHAPES = [
    (1, 1, 8, 8, 8),           # smallest legal problem
    (1, 2, 64, 64, 64),        # exactly one tile
    (1, 2, 72, 72, 72),        # ragged last tile of 8 in both kernels
    (1, 2, 128, 128, 128),     # exactly one owner block
    (1, 2, 136, 136, 136),     # second owner block with 8 live rows
    (2, 3, 200, 77, 80),       # the cross-attention shape
    (1, 1, 8, 1024, 1024),     # extreme aspect
    (1, 1, 1024, 8, 8),        # extreme aspect
    (2, 4, 128, 128, 128),     # 8 blocks: the XCD remap is taken
    (1, 3, 384, 384, 384),     # 9 blocks: the remap is not taken
    (2, 4, 256, 256, 256),     # 16 blocks
]
FAMILY_SHAPES = [BWD_SHAPES[2], BWD_SHAPES[4], BWD_SHAPES[5], BWD_SHAPES[8]]
FAMILIES = ["gauss", "sharp", "spike", "qzero", "vconst", "dozero"]


def bwd_cases():
    return [(s, "gauss") for s in BWD_SHAPES] + [(s, f) for f in FAMILIES[1:] for s in FAMILY_SHAPES]


def case_id(case) -> str:
    return "x".join(str(i) for i in case[0]) + "-" + case[1]


def make_inputs(shape, family: str = "gauss", seed: int = 0, d: int = D):
    """-> f16 CPU tensors q [B, Nq, C], k, v [B, Nk_rows, C] (rows >= Nk zero, as gn_attn_bwd_desc requires), d_o [B, Nq, C]."""
    B, heads, Nq, Nk, Nkr = shape
    C = heads * d
    g = torch.Generator().manual_seed(1000 * seed + 7 * Nq + Nk + heads)
    q, d_o = torch.randn(B, Nq, C, generator=g), torch.randn(B, Nq, C, generator=g)
    k, v = torch.zeros(B, Nkr, C), torch.zeros(B, Nkr, C)
    k[:, :Nk], v[:, :Nk] = torch.randn(B, Nk, C, generator=g), torch.randn(B, Nk, C, generator=g)
    if family == "sharp":     # sharp rows; most P below the f16 normal range
        q *= 4
    elif family == "spike":   # one key that every query of every head looks at
        k[:, Nk // 3] *= 6
    elif family == "qzero":   # a query row of zeros: uniform P
        q[:, Nq // 2] = 0
    elif family == "vconst":  # v constant along the keys: O = v, dP = delta, dS = 0
        v[:, :Nk] = v[:, :1]
    elif family == "dozero":
        d_o.zero_()
    elif family == "vpos":    # |v|: nothing cancels in P.V, o_ab = |O|
        v.abs_()
    elif family == "voffset":  # v constant along the keys, off zero by 1: O = v, the centred term of the forward bound vanishes
        v[:, :Nk] = v[:, :1] + 1
    else:
        assert family == "gauss", family
    return tuple(t.to(F16) for t in (q, k, v, d_o))


_FIXTURES: dict = {}


def bwd_fixture(case):
    """(q, k, v, d_o, o16, lse32, ref) of a case, computed once and shared (leave it unchanged): o16 / lse32 are the f64 forward rounded to
    f16 / f32 -- what the backward kernel is handed in the tests of the backward alone -- and ref is attn_bwd_ref on exactly those."""
    key = case_id(case)
    if key not in _FIXTURES:
        (B, heads, Nq, Nk, Nkr), family = case
        q, k, v, d_o = make_inputs(*case)
        o, lse = attn_fwd_ref(q, k, v, heads, Nk, D ** -0.5)
        o16, lse32 = o.to(F16), lse.to(F32)
        _FIXTURES[key] = (q, k, v, d_o, o16, lse32, attn_bwd_ref(q, k, v, d_o, o16, lse32, heads, Nk, D ** -0.5))
    return _FIXTURES[key]
