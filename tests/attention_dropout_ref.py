"""CPU references and derived error bounds for attention-probability dropout (gn_attention_dropout_fwd / _bwd / _apply,
csrc/attention.hip, csrc/attention_bwd.hip; the mask is stated in include/genima_hip.h): tests/test_attention_dropout_cpu.py,
tests/test_attention_dropout_gpu.py, tests/test_act_attn_dropout_gpu.py.

TEST INFRASTRUCTURE ONLY, in the manner of tests/attention_ref.py (whose layouts and helpers it uses): the mask in numpy uint32, the
f64 forward and backward with a given mask, the bounds.  Nothing here goes through genima_amd.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import attention_ref as R
from act_ops_ref import ulp16

F64, F32, F16 = torch.float64, torch.float32, torch.float16
U32 = np.uint32
LN2 = 0.6931471805599453

# the seeds of the issue's known answers / statistics, and the seeds the GPU tests run (one with high bits set)
KNOWN_SEEDS = [0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1]
KNOWN_ANSWERS = [(0, 0, 0, 0, 0x8DFA131D), (1, 0, 0, 0, 0xC9C8482B), (0x0123456789ABCDEF, 5, 17, 200, 0x390B54C6), (2 ** 64 - 1, 15, 263, 263, 0xC6FB3B71)]


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
def mix(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 arrays (wrapping)."""
    x = np.array(x, dtype=U32, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7FEB352D)
        x ^= x >> U32(15)
        x *= U32(0x846CA68B)
        x ^= x >> U32(16)
    return x


def hash_r(seed: int, bh, i, j):
    """r of (seed, bh, query i, key j), broadcasting over integer arrays -> uint32 array."""
    lo, hi = U32(seed & 0xFFFFFFFF), U32((seed >> 32) & 0xFFFFFFFF)
    bh, i, j = (np.array(t, dtype=np.int64).astype(U32) for t in (bh, i, j))
    with np.errstate(over="ignore"):
        a = mix(lo ^ U32(0x6A09E667) ^ (bh * U32(0x9E3779B9)))
        row = mix((a ^ hi) + i * U32(0x85EBCA6B))
        return mix(row ^ (j * U32(0xC2B2AE35)))


def threshold(p: float) -> int:
    """min(2^32 - 1, floor(p 2^32)) in f64."""
    return min(2 ** 32 - 1, int(np.floor(np.float64(p) * 2.0 ** 32)))


def keep_mask(seed: int, p: float, BH: int, Nq: int, Nk: int) -> np.ndarray:
    """keep[bh, i, j] = r >= threshold(p) -> bool [BH, Nq, Nk]."""
    r = hash_r(seed, np.arange(BH)[:, None, None], np.arange(Nq)[None, :, None], np.arange(Nk)[None, None, :])
    return r >= U32(threshold(p))


def keep_tensor(seed: int, p: float, B: int, heads: int, Nq: int, Nk: int) -> torch.Tensor:
    """keep as f64 0 / 1 [B, heads, Nq, Nk] (bh = b * heads + h)."""
    return torch.from_numpy(keep_mask(seed, p, B * heads, Nq, Nk)).to(F64).reshape(B, heads, Nq, Nk)


# ---- f64 forward and backward with a given mask -----------------------------------------------------------------------------------------
def fwd_ref(q, k, v, heads: int, Nk: int, scale: float, keep: torch.Tensor, p: float):
    """O = ((softmax(S) o keep) / (1 - p)) V over keys [0, Nk) -> (O [B, Nq, C] f64, lse2 [B, heads, Nq]); lse2 is the undropped one.
    Also the magnitude sums the forward bound needs (see fwd_bound)."""
    qh, kh, vh = R._heads(q, heads), R._heads(k[:, :Nk], heads), R._heads(v[:, :Nk], heads)
    s = qh @ kh.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    Pm = torch.exp(s - lse[..., None]) * keep / (1.0 - p)
    out = SimpleNamespace(o=R._rows(Pm @ vh), lse2=lse * R.LOG2E)
    out.o_ab = R._rows(Pm @ vh.abs())
    out.o_b = R._rows((keep / (1.0 - p)) @ vh.abs())
    return out


def bwd_ref(q, k, v, d_o, heads: int, Nk: int, scale: float, keep: torch.Tensor, p: float, o16=None, lse2=None):
    """The f64 backward with dropout:
        delta = sum_d dO O, dV = (P o keep / (1 - p))^T dO, dP = (dO V^T) o keep / (1 - p), dS = scale P (dP - delta), dQ = dS K, dK = dS^T Q.
    With o16 / lse2 (what the flash backward kernel is handed) P = exp2(s scale log2e - lse2) and delta comes from o16, as in
    attention_ref.attn_bwd_ref; without them P is the f64 softmax and delta = sum_j P dP (the function's exact gradient: what the
    materialised route, which never sees o or lse, is compared with).  Magnitude sums as in attention_ref._bwd, the masked terms with
    their 1 / (1 - p)."""
    qh, kh, vh, gh = (R._heads(t, heads) for t in (q, k[:, :Nk], v[:, :Nk], d_o))
    ik = 1.0 / (1.0 - p)
    s = qh @ kh.transpose(-1, -2)
    if lse2 is not None:
        P = torch.exp2(s * (scale * R.LOG2E) - lse2.to(F64)[..., None])
    else:
        P = torch.softmax(s * scale, -1)
    dP = (gh @ vh.transpose(-1, -2)) * keep * ik
    if o16 is not None:
        oh = R._heads(o16, heads)
        delta, delta_ab = (gh * oh).sum(-1), (gh.abs() * oh.abs()).sum(-1)
    else:
        delta, delta_ab = (P * dP).sum(-1), (P * dP.abs()).sum(-1)
    dS = P * (dP - delta[..., None]) * scale
    Pk = P * keep * ik
    out = SimpleNamespace(delta=delta, delta_ab=delta_ab, dq=R._rows(dS @ kh), dk=R._rows(dS.transpose(-1, -2) @ qh), dv=R._rows(Pk.transpose(-1, -2) @ gh))
    aq, ak, av, ag = qh.abs(), kh.abs(), vh.abs(), gh.abs()
    dS32 = P * ((ag @ av.transpose(-1, -2)) * keep * ik + delta_ab[..., None]) * scale
    out.dq_ab, out.dq_ab32, out.dq_b = R._rows(dS.abs() @ ak), R._rows(dS32 @ ak), R._rows(ak.sum(-2, keepdim=True).expand_as(qh))
    out.dk_ab, out.dk_ab32, out.dk_b = (R._rows(dS.abs().transpose(-1, -2) @ aq), R._rows(dS32.transpose(-1, -2) @ aq),
                                        R._rows(aq.sum(-2, keepdim=True).expand_as(kh)))
    out.dv_ab = R._rows(Pk.transpose(-1, -2) @ ag)
    out.dv_ab32 = out.dv_ab
    out.dv_b = R._rows((keep * ik).transpose(-1, -2) @ ag)
    out.parts = SimpleNamespace(qh=qh, kh=kh, vh=vh, gh=gh, s=s, P=P, dP=dP, dS=dS, Pk=Pk, keep=keep, ik=ik)
    return out


# ---- bounds: the flash kernels -------------------------------------------------------------------------------------------------------
# Backward (attention_bwd.hip, DROP): the plain kernels' arithmetic (attention_ref.bwd_bounds: the f16 store, the left operand rounded to f16
# at unit roundoff 2^-11 / half the subnormal spacing 2^-25, M32 for everything f32) with two more f32 roundings: dP * inv_keep in front
# of "- delta" (dQ, dK) and accV * inv_keep in front of the store (dV), inv_keep itself the f32 rounding of 1 / (1 - p).  The masked terms
# carry 1 / (1 - p) inside the magnitude sums (bwd_ref).  M32 cannot be derived (it is a measured constant of attention_ref, from the f32
# restatement on the CPU, never from a GPU run): the dropout kernels get 2 x M32 for the extra rounding of the scale.
M32_DROP = {n: 2 * m for n, m in R.M32.items()}


def bwd_bounds(ref) -> dict:
    out = {}
    for n in ("dq", "dk", "dv"):
        x, ab, ab32, b = getattr(ref, n), getattr(ref, n + "_ab"), getattr(ref, n + "_ab32"), getattr(ref, n + "_b")
        out[n] = 0.5 * ulp16(x) + 2.0 ** -11 * ab + 2.0 ** -25 * b + M32_DROP[n] * ab32
    out["delta"] = 64 * 2.0 ** -24 * ref.delta_ab  # unchanged: an f32 sum of 64 exact products
    return out


# Forward (attention.hip, DROP), per output element o = inv_keep / l * sum_j p16_j keep_j v_j with p16_j = f16(exp2(s'_j)), l = sum_j p16_j:
#   (1) q' = f16(f32(q) c) is a rounding of the INPUT (attention_ref.lse2_bound (1)): evaluated, not bounded -- shift = |O(q') - O(q)| in f64;
#   (2) p_j -> f16: 2^-11 relative per kept term -> 2^-11 o_ab, o_ab = sum_j P_j keep_j |v_j| / (1 - p); half the subnormal spacing 2^-25 per kept
#       term against l >= 1 -> 2^-25 o_b, o_b = sum_j keep_j |v_j| / (1 - p); the same roundings in the denominator l move o by at most
#       (2^-11 + n 2^-25) |o|;
#   (3) f32, in units of 2^-24 and relative to o_ab + |o|: the score behind each p_j is off by (130 + 2 n / 32) A log2 units (lse2_bound (3): the
#       65 products-and-init, the reference kept in two registers), i.e. ln 2 times that relative to p_j; v_exp_f32 at 1 ulp (2); the
#       rescales alpha, once per 32 keys at most (3 n / 32); the P.V and row-sum chains (2 n); inv_keep, the division and the product (8);
#   (4) the store: 1/2 ulp16.
def fwd_bound(q, k, v, heads: int, Nk: int, scale: float, keep: torch.Tensor, p: float):
    """-> (fwd_ref result, per-element bound [B, Nq, C])."""
    ref = fwd_ref(q, k, v, heads, Nk, scale, keep, p)
    q1 = (q.to(F32) * R.c_log2(scale, F32)).to(F16)
    # the same formula on q' (already in exponent units: scale log2 e is inside)
    qh, kh, vh = R._heads(q1, heads), R._heads(k[:, :Nk], heads), R._heads(v[:, :Nk], heads)
    s1 = (qh @ kh.transpose(-1, -2)) * LN2
    o1 = R._rows((torch.softmax(s1, -1) * keep / (1.0 - p)) @ vh)
    shift = (o1 - ref.o).abs()
    A = (qh.abs() @ kh.abs().transpose(-1, -2)).amax(-1)  # [B, heads, Nq]
    n = Nk
    f32_rel = 2.0 ** -24 * (LN2 * (130 + 2 * n / 32) * A + 2 + 3 * n / 32 + 2 * n + 8)
    f32_rel = f32_rel[..., None].expand(*A.shape, q.shape[-1] // heads)
    f32_rel = R._rows(f32_rel)
    bound = (0.5 * ulp16(ref.o) + shift + 2.0 ** -11 * ref.o_ab + 2.0 ** -25 * ref.o_b + (2.0 ** -11 + n * 2.0 ** -25) * ref.o.abs()
             + f32_rel * (ref.o_ab + ref.o.abs()))
    return ref, bound


# ---- bounds: the materialised route (training.Graph.attention with flash_bwd off, or D != 64) -----------------------------------------------
# Other arithmetic, other bound.  The route never sees o or lse; it computes (u = 2^-11, n = Nk, every GEMM an f32 accumulation stored as f16)
#   S16 = f16(q k^T)                      |dS16| <= u |s| + 64 2^-24 sum_d |q||k|, in the exponent times scale: e_ij
#   P16 = f16(softmax(scale S16))         ln P_j moves by at most e_ij + max_l e_il; f32 exp / sum / divide (n + 8) 2^-24; the store u, or 2^-25 below
#                                         the normal range                                 -> eP  = P (expm1(e + emax) + (n + 8) 2^-24 + u) + 2^-25
#   dP16 = f16(dO v^T)                                                                     -> eD1 = u |dP| + 2^-25 + 64 2^-24 sum_d |dO||v|
#   dPm16 = f16(f32(dP16) inv_keep) o keep (gn_attention_dropout_apply)                    -> eDm = keep ik (eD1 + (u + 2^-23) |dP|) + 2^-25 keep
#   dot_i = sum_j P16 dPm16 (f32)         (gn_softmax_bwd)                                 -> eDot = sum_j (eP |dPm| + (P + eP) eDm) + n 2^-24 sum_j P |dPm|
#   dS16 = f16(scale P16 (dPm16 - dot))                                -> eS = scale (eP |dPm - dot| + (P + eP)(eDm + eDot)) + (u + 4 2^-24) |dS| + 2^-25
#   Pd16 = f16(f32(P16) inv_keep) o keep                                                   -> ePd = keep ik (eP + (u + 2^-23) P) + 2^-25 keep
#   dQ = f16(dS16 K), dK = f16(dS16^T Q), dV = f16(Pd16^T dO)         -> the operand's error through the product, rows 2^-24 of the magnitude sum
#                                                                        for the accumulation, 1/2 ulp16 for the store
# against bwd_ref(..., o16=None, lse2=None), the exact gradient.  The transposes are exact.
def gemm_route_bounds(ref, scale: float, Nq: int, Nk: int) -> dict:
    t = ref.parts
    u, n = 2.0 ** -11, Nk
    aq, ak, av, ag = t.qh.abs(), t.kh.abs(), t.vh.abs(), t.gh.abs()
    e = scale * (u * t.s.abs() + 64 * 2.0 ** -24 * (aq @ ak.transpose(-1, -2)))
    eP = t.P * (torch.expm1(e + e.amax(-1, keepdim=True)) + (n + 8) * 2.0 ** -24 + u) + 2.0 ** -25
    dP_raw = t.gh @ t.vh.transpose(-1, -2)
    eD1 = u * dP_raw.abs() + 2.0 ** -25 + 64 * 2.0 ** -24 * (ag @ av.transpose(-1, -2))
    eDm = t.keep * t.ik * (eD1 + (u + 2.0 ** -23) * dP_raw.abs()) + 2.0 ** -25 * t.keep
    eDot = (eP * t.dP.abs() + (t.P + eP) * eDm).sum(-1, keepdim=True) + n * 2.0 ** -24 * (t.P * t.dP.abs()).sum(-1, keepdim=True)
    eS = scale * (eP * (t.dP - ref.delta[..., None]).abs() + (t.P + eP) * (eDm + eDot)) + (u + 4 * 2.0 ** -24) * t.dS.abs() + 2.0 ** -25
    ePd = t.keep * t.ik * (eP + (u + 2.0 ** -23) * t.P) + 2.0 ** -25 * t.keep
    aS = t.dS.abs() + eS
    out = {
        "dq": R._rows(eS @ ak + n * 2.0 ** -24 * (aS @ ak)),
        "dk": R._rows(eS.transpose(-1, -2) @ aq + Nq * 2.0 ** -24 * (aS.transpose(-1, -2) @ aq)),
        "dv": R._rows(ePd.transpose(-1, -2) @ ag + Nq * 2.0 ** -24 * ((t.Pk + ePd).transpose(-1, -2) @ ag)),
    }
    for name in out:
        out[name] = out[name] + 0.5 * ulp16(getattr(ref, name))
    return out


def assert_all(got: dict, ref, bounds: dict, what: str, names) -> dict:
    """Every element of every named output within its bound; all outputs are looked at before it raises.  -> {name: max err / bound}."""
    ratios, failed = {}, []
    for n in names:
        try:
            ratios[n] = R.assert_within(got[n], getattr(ref, n), bounds[n], f"{what} {n}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return ratios


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------------
B, HEADS = 2, 2
# (Nq, Nk_rows, Nk valid)
SHAPES = [
    (24, 24, 22),      # the CVAE encoder / decoder self-attention size
    (24, 264, 258),    # the decoder cross-attention: a ragged last 64-key tile
    (264, 264, 258),   # three query blocks in the forward and the dQ kernel, three key blocks in dK / dV
    (136, 72, 72),
]
SHAPE_D32 = (24, 24, 22)  # D = 32: forward and apply only
PS = [0.1, 0.5]
SEEDS = [0x0123456789ABCDEF, 2 ** 64 - 1, 7]  # two with high bits set


def make_inputs(Nq: int, Nkr: int, Nk: int, D: int = 64, seed: int = 0):
    """-> f16 CPU tensors q [B, Nq, C], k, v [B, Nk_rows, C] (rows >= Nk zero), d_o [B, Nq, C], from a fixed generator."""
    C = HEADS * D
    g = torch.Generator().manual_seed(4000 + 1000 * seed + 7 * Nq + Nk + D)
    q, d_o = torch.randn(B, Nq, C, generator=g), torch.randn(B, Nq, C, generator=g)
    k, v = torch.zeros(B, Nkr, C), torch.zeros(B, Nkr, C)
    k[:, :Nk], v[:, :Nk] = torch.randn(B, Nk, C, generator=g), torch.randn(B, Nk, C, generator=g)
    return tuple(t.to(F16) for t in (q, k, v, d_o))
