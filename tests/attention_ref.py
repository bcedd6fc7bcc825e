"""CPU references and derived error bounds for the flash-attention backward (csrc/attention_bwd.hip) and the log2-domain lse of the
forward kernels (attention.hip, attention_stream.hip, attention_pwg.hip): tests/test_attention_ref_cpu.py, tests/test_attention_bwd_gpu.py.

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


def make_inputs(shape, family: str = "gauss", seed: int = 0):
    """-> f16 CPU tensors q [B, Nq, C], k, v [B, Nk_rows, C] (rows >= Nk zero, as gn_attn_bwd_desc requires), d_o [B, Nq, C]."""
    B, heads, Nq, Nk, Nkr = shape
    C = heads * D
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
