"""CPU references and derived per-element error bounds for gn_gemm: the block-tile kernels of csrc/gemm.hip, gemm_s3.hip, gemm_pp.hip, gemm_ppp.hip,
the split-K reduce, and the fused epilogue they share (csrc/gemm_common.h) -- dense, implicit-GEMM conv, GEGLU, f32 / accumulating output and the
LayerNorm fold: tests/test_gemm_ref_cpu.py, tests/test_gemm_f64_gpu.py, the two seeded sweeps of tests/test_gemm_tiles_gpu.py.

TEST INFRASTRUCTURE ONLY, in the manner of tests/norm_fwd_ref.py and tests/attention_ref.py: torch on the CPU, evaluated from the kernel's own
f16 / f32 inputs; nothing here goes through genima_amd.  gemm_ref(F64, ...) is the reference.  gemm_ref(F32, ...) restates the kernel's arithmetic
(gemm_common.h: accumulator + bias + shift, the residual before or after the activation, act_silu = x / (1 + expf(-x)), gelu_fast on the
Abramowitz-Stegun 7.1.26 fast_erf, act_quick_gelu, relu, out_scale, ONE rounding to f16 or none for GN_OUT_F32); it exists to measure K_ACT, to
show that the bound's form is met by plain f32 evaluation and to carry the plants.  No GPU test compares against it.

THE BOUND, per output element (derived from the code, never fitted to a device result):
    |got - ref| <= 1/2 ulp16(ref)          the one f16 store (absent for f32 output)
                 + S E_z                    the pre-activation error carried through the activation by its LARGEST slope on [z - E_z, z + E_z]
                 + K_act 2^-24 T_act        the activation's own f32 arithmetic (+ gelu_fast's approximation error, + the f32 underflow floor)
                 + 2^-24 |y s|              out_scale: one product
                 + 2^-24 (|y s| + |res|)    the residual added after the activation: one sum
    E_z = 2 (K + n_adds) 2^-24 (sum_k |x| |w| + |bias| + |shift| + |res_pre|)
two roundings per MFMA accumulate (the convention of attention_ref.lse2_bound), whatever the summation order -- so the split-K slabs, their
fixed-order reduce and tile 25's hand-offs are covered; n_adds = the epilogue's additions before the activation + the slabs a split K adds up.
No element is masked or left out.

The largest err / bound of a CORRECT result sits just below 1 (0.999 on the CPU restatement and on the device alike), and that is the half-ulp term at
work, not a lack of room: among 10^5 elements some f32 value lies within 1e-3 of an ulp of the midpoint of two f16 values, its stored value is then
1/2 ulp16 from the f32 value, and the other terms are what separates err from the bound.  ulp16(ref) is the spacing ABOVE |f16(ref)|, so a reference
at a binade boundary takes the wider spacing.  A wrong kernel is not a near miss at short K: the dense plants of tests/test_gemm_ref_cpu.py sit at 20 to 10^6 times the bound.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from act_ops_ref import ulp16
from attention_ref import assert_within  # noqa: F401  (re-exported: the GPU tests assert with it)
from norm_bwd_ref import MARGIN, U32, _cached, _gen, eps32
from norm_fwd_ref import old_bar_passes, silu_slope_max  # noqa: F401  (old_bar_passes: util.assert_close's two conditions as a predicate)

Tensor = torch.Tensor
F64, F32, F16 = torch.float64, torch.float32, torch.float16
ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_GEGLU = 0, 1, 2, 3, 4, 5
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_QUICK_GELU: "quick_gelu", ACT_RELU: "relu", ACT_GEGLU: "geglu"}
SMOOTH = (ACT_SILU, ACT_GELU, ACT_QUICK_GELU)
QG = 1.702
AS_ERF_ERR = 1.5e-7      # Abramowitz-Stegun 7.1.26: |erf - approximation| <= 1.5e-7, so gelu_fast is within 0.5 |z| 1.5e-7 of GELU before any rounding
# Where e^-z nears the f32 overflow (z < -87.3) the quotient z / (1 + e^-z) is below 87.4 x 2^-126 < 2^-119: a reciprocal flushed to zero or an
# exponential that overflowed returns 0 there.  Irrelevant beside any f16 spacing (2^-24); stated so that the `wide` family needs no mask.
F32_TINY = 2.0 ** -118
# largest (|f32 restatement - f64| - the stated absolute terms) / (2^-24 T_act) on the f32 pre-activation, over every case x family of the lists below
# (CPU; tests/test_gemm_ref_cpu.py::test_k_act_is_four_times_the_measured_f32_error prints and pins them); K_ACT = MARGIN x this for what the CPU
# lacks (v_exp_f32, v_rcp_f32, FMA contraction).  Never taken from a GPU run.
K_ACT_MEASURED = {
    "silu": 1.97,         # (97, 172, 136) cancel, residual before the activation
    "gelu": 3.038,        # (289, 332, 136) gauss, residual before the activation
    "quick_gelu": 1.178,  # (129, 136, 56) wide, residual before the activation
}
K_ACT = {n: MARGIN * v for n, v in K_ACT_MEASURED.items()}


# ---- activations ---------------------------------------------------------------------------------------------------------------------------
def _fast_erf32(x: Tensor) -> Tensor:
    """gemm_common.h fast_erf on f32 values (python scalars do not promote an f32 tensor: every constant is the kernel's `...f` literal)."""
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return torch.copysign(1.0 - poly * torch.exp(-ax * ax), x)


def _gelu(dt, z: Tensor, tanh: bool = False) -> Tensor:
    if tanh:
        return 0.5 * z * (1.0 + torch.tanh(0.7978845608028654 * (z + 0.044715 * z * z * z)))
    if dt == F64:
        return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    return 0.5 * z * (1.0 + _fast_erf32(z * 0.70710678118654752))


def _act(dt, z: Tensor, act: int, plant: str = "") -> Tensor:
    if act == ACT_SILU:
        return z / (1.0 + torch.exp(-z))
    if act == ACT_GELU:
        return _gelu(dt, z, tanh=plant == "tanh_gelu")
    if act == ACT_QUICK_GELU:
        return z / (1.0 + torch.exp(-QG * z))
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    assert act == ACT_NONE, act
    return z


GELU_ZSTAR, GELU_SMAX, GELU_SMIN = math.sqrt(2.0), 1.128905, 0.128905  # gelu'' = phi(z) (2 - z^2) = 0 at +-sqrt 2; gelu'(sqrt 2), -gelu'(-sqrt 2), rounded up


def _gelu_slope(z: Tensor) -> Tensor:
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def gelu_slope_max(lo: Tensor, hi: Tensor) -> Tensor:
    """max |gelu'| over [lo, hi], as norm_fwd_ref.silu_slope_max: gelu' = Phi + z phi falls from 0 to its minimum -0.1289 at -sqrt 2, rises to its
    maximum 1.1289 at +sqrt 2 and falls to 1, monotone in between; the largest magnitude is at an end or at whichever of +-sqrt 2 the interval holds."""
    m = torch.maximum(_gelu_slope(lo).abs(), _gelu_slope(hi).abs())
    m = torch.where((lo < GELU_ZSTAR) & (hi > GELU_ZSTAR), torch.full_like(m, GELU_SMAX), m)
    return torch.where((lo < -GELU_ZSTAR) & (hi > -GELU_ZSTAR), m.clamp_min(GELU_SMIN), m)


def slope_max(act: int, lo: Tensor, hi: Tensor) -> Tensor:
    if act == ACT_SILU:
        return silu_slope_max(lo, hi)
    if act == ACT_QUICK_GELU:  # quick_gelu(z) = silu(1.702 z) / 1.702: the same curve in 1.702 z
        return silu_slope_max(QG * lo, QG * hi)
    if act in (ACT_GELU, ACT_GEGLU):
        return gelu_slope_max(lo, hi)
    return torch.ones_like(lo)


def act_terms(act: int, z: Tensor):
    """-> (T_act, absolute) of the activation's own f32 arithmetic at the f64 pre-activation z:
    SiLU      T = |y| (1 + (1 + |z|) (1 - sigma(z)))       norm_fwd_ref.apply_bound: the quotient's roundings and the fast exponential's relative
                                                            (1 + |z|) 2^-24, which reaches y through e^-z / (1 + e^-z) = 1 - sigma
    QuickGELU the same in u = 1.702 z, one more for the product 1.702 z
    GELU      T = |y| + |z|: 1 + erf is O(1) and carries an ABSOLUTE error of a few 2^-24 (1 - poly e^-x^2, then 1 + .), which reaches y through
              0.5 z; the products add |y|.  absolute = 0.5 |z| 1.5e-7, the approximation itself.
    absolute also holds F32_TINY."""
    az = z.abs()
    if act == ACT_SILU:
        y = _act(F64, z, act)
        return y.abs() * (1 + (1 + az) * (1 - torch.sigmoid(z))), torch.full_like(z, F32_TINY)
    if act == ACT_QUICK_GELU:
        y = _act(F64, z, act)
        return y.abs() * (2 + (1 + QG * az) * (1 - torch.sigmoid(QG * z))), torch.full_like(z, F32_TINY)
    if act in (ACT_GELU, ACT_GEGLU):
        return _gelu(F64, z).abs() + az, 0.5 * az * AS_ERF_ERR + F32_TINY
    return torch.zeros_like(z), torch.zeros_like(z)


def act_bound(act: int, z: Tensor, Ez: Tensor) -> Tensor:
    """Bound of the kernel's act(z') against act(z) (f64) for |z' - z| <= Ez, before scale / residual / store."""
    if act in (ACT_NONE, ACT_RELU):  # fmaxf is exact and 1-Lipschitz
        return Ez
    T, absolute = act_terms(act, z)
    return slope_max(act, z - Ez, z + Ez) * Ez + K_ACT[ACT_NAME[ACT_GELU if act == ACT_GEGLU else act]] * U32 * T + absolute


def act_k(act: int, z32: Tensor) -> float:
    """The measured constant of one activation on f32 pre-activations: largest (|act32 - act64| - absolute) / (2^-24 T_act)."""
    zz = z32.to(F64)
    T, absolute = act_terms(act, zz)
    err = (_act(F32, z32, act).to(F64) - _act(F64, zz, act)).abs() - absolute
    rel = err.clamp_min(0) / (U32 * T.clamp_min(1e-300))
    return float(rel[T > 0].max()) if bool((T > 0).any()) else 0.0


# ---- the GEMM and its epilogue ---------------------------------------------------------------------------------------------------------------
def split_geglu(t: Tensor):
    """[M, 2 Nh] in packing.pack_geglu's layout (32-column blocks hidden | gate) -> (hidden, gate) [M, Nh] in output-column order."""
    M, N2 = t.shape
    b = t.reshape(M, N2 // 64, 2, 32)
    return b[:, :, 0].reshape(M, N2 // 2), b[:, :, 1].reshape(M, N2 // 2)


def pack_geglu_rows(t: Tensor) -> Tensor:
    """[2 Nh, ...] (hidden rows, then gate rows) -> 32-row blocks hidden | gate: packing.pack_geglu's layout, restated so that this file stands alone."""
    n2 = t.shape[0]
    h, g = t[: n2 // 2].reshape(n2 // 64, 32, *t.shape[1:]), t[n2 // 2:].reshape(n2 // 64, 32, *t.shape[1:])
    return torch.stack([h, g], 1).reshape(t.shape).contiguous()


def _accumulate(dt, x: Tensor, w: Tensor, plant: str = "") -> Tensor:
    xs, ws = x.to(dt), w.to(dt)
    if plant == "drop_last_k_last_row":  # a K-tail mask one element short on the last row
        xs = xs.clone()
        xs[-1, -1] = 0
    if plant == "acc_f16_per_ktile":     # the accumulator rounded to f16 once per 64-wide K tile
        acc = torch.zeros(x.shape[0], w.shape[0], dtype=dt)
        for k0 in range(0, x.shape[1], 64):
            acc = (acc + xs[:, k0:k0 + 64] @ ws[:, k0:k0 + 64].t()).to(F16).to(dt)
        return acc
    acc = xs @ ws.t()
    return acc.to(F16).to(dt) if plant == "acc_f16_before_bias" else acc


def _rows(shift: Tensor, rpb: int, M: int, dt) -> Tensor:
    """per-batch shift [B, N] -> [M, N]: row m takes batch m / rpb (epilogue_vals4)."""
    return shift.to(dt)[torch.arange(M) // rpb]


def gemm_ref(dt, x: Tensor, w: Tensor, bias=None, shift=None, rpb: int = 0, res=None, res_first: bool = False, act: int = ACT_NONE,
             out_scale: float = 1.0, *, out_f32: bool = False, old=None, splitk: int = 1, pre=None, plant: str = ""):
    """out = act(x w^T + bias + shift[m / rpb] (+ res if res_first)) out_scale (+ res if not res_first)  [+ old for the accumulating f32 output]
    x [M, K], w [N, K] f16; bias [N], shift [B, N], res [M, N] f16 or None; ``splitk``: the slabs a split K adds (0 / 1: none).
    ``pre`` = (acc, E_acc, T_acc) replaces x w^T, its error bound and its magnitude (the LayerNorm fold).
    GEGLU (act 5): (acc_h + b_h) gelu_fast(acc_g + b_g) over w's packed hidden | gate blocks -> [M, N / 2].
    -> namespace y (before the store; f64: the reference), and for dt = f64 without plant: bound, z, Ez.
    dt = f32: also y16, the stored value.  ``plant``: one deliberate error (tests/test_gemm_ref_cpu.py)."""
    M, K = x.shape
    if pre is None:
        acc = _accumulate(dt, x, w, plant)
    else:
        acc = pre[0].to(dt)
    z = acc
    adds = []
    if plant == "conv_bias_plus_shift_f16" and bias is not None and shift is not None:  # the two f16 vectors summed in f16, then added once
        z = z + (bias.to(F16)[None, :] + _rows(shift, rpb, M, F16)).to(dt)
    else:
        if bias is not None:
            z = z + bias.to(dt)
        if shift is not None:
            z = z + _rows(shift, rpb, M, dt)
    if bias is not None:
        adds.append(bias.to(F64).abs().expand(acc.shape))
    if shift is not None:
        adds.append(_rows(shift, rpb, M, F64).abs())
    r = res.to(dt) if res is not None else None
    pre_res = r is not None and res_first and plant != "res_after_for_res_first"
    if pre_res:
        z = z + r
        adds.append(r.to(F64).abs())
    out = SimpleNamespace()
    if act == ACT_GEGLU:
        h, g = split_geglu(z)
        if plant == "geglu_halves_swapped":
            h, g = g, h
        y = h * _gelu(dt, g, tanh=plant == "tanh_gelu")
    else:
        if plant == "scale_before_act":
            y = _act(dt, z * out_scale, act, plant)
        else:
            y = _act(dt, z, act, plant)
            if out_scale != 1.0:
                y = y * out_scale
        if plant == "act_f16_then_residual":  # the activation's output rounded to f16, then the residual added and rounded again
            y = y.to(F16).to(dt)
        if r is not None and not pre_res:
            y = y + r
    if old is not None:
        y = y + old.to(dt)
    out.y = y
    if dt != F64:
        out.y16 = y if out_f32 else y.to(F16)
        return out
    if plant:
        return out
    # ---- the bound ----
    if pre is None:
        T_acc = x.to(F64).abs() @ w.to(F64).abs().t()
        n_adds = len(adds) + (splitk if splitk > 1 else 0)
        Ez = 2 * (K + n_adds) * U32 * (T_acc + sum(adds))
    else:
        Ez = pre[1] + 2 * len(adds) * U32 * (pre[2] + sum(adds))
    out.z, out.Ez = z, Ez
    if act == ACT_GEGLU:
        (Eh, Eg), gel = split_geglu(Ez), _gelu(F64, g)
        Ea = act_bound(ACT_GEGLU, g, Eg)
        E = gel.abs() * Eh + h.abs() * Ea + Eh * Ea + U32 * y.abs()
    else:
        ya = _act(F64, z, act)
        E = act_bound(act, z, Ez)
        if out_scale != 1.0:
            ya = ya * out_scale
            E = E * abs(out_scale) + U32 * ya.abs()
        if r is not None and not pre_res:
            E = E + U32 * (ya.abs() + r.abs())
    if old is not None:
        E = E + U32 * (old.to(F64).abs() + (y - old.to(F64)).abs())
    out.bound = E if out_f32 else E + 0.5 * ulp16(y)
    return out


def accumulate_twice_ref(x: Tensor, w: Tensor, start: float):
    """Two accumulating f32-output calls onto a buffer full of ``start``: ref = start + 2 x w^T; each call adds E_z and the rounding of its sum,
    2^-24 (|old| + |new|)."""
    one = gemm_ref(F64, x, w, out_f32=True)
    old1 = torch.full_like(one.y, start)
    y1 = old1 + one.y
    y2 = y1 + one.y
    return SimpleNamespace(y=y2, bound=2 * one.Ez + U32 * (old1.abs() + one.y.abs()) + U32 * (y1.abs() + one.y.abs()))


# ---- implicit-GEMM conv: the same matrix by im2col in the packed weight's K order ---------------------------------------------------------------
def im2col(x: Tensor, x2, k: int, stride: int, pad, upsample2x: bool = False, plant: str = ""):
    """NHWC x (| x2 virtually concatenated along C), nearest-2x upsampled first where asked, zero-padded by pad = (top, left, bottom, right)
    -> ([B Ho Wo, k k C] with K ordered tap-major, channel-minor as the packed weight [Cout, k, k, C], (Ho, Wo)).  Keeps the dtype."""
    xin = torch.cat([x, x2], -1) if x2 is not None else x
    if upsample2x:
        xin = xin.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, C = xin.shape
    t, l, b, r = pad
    xp = torch.zeros(B, H + t + b, W + l + r, C, dtype=xin.dtype)
    xp[:, t:t + H, l:l + W] = xin
    if plant == "conv_tap_off_by_one_at_border" and r > 0:  # the right-hand padding column read as pixel W - 1
        xp[:, t:t + H, l + W:] = xin[:, :, W - 1:W]
    Ho, Wo = (H + t + b - k) // stride + 1, (W + l + r - k) // stride + 1
    cols = [xp[:, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride] for i in range(k) for j in range(k)]
    return torch.cat(cols, -1).reshape(B * Ho * Wo, k * k * C), (Ho, Wo)


def conv_ref(dt, x, x2, w, bias, k: int, stride: int = 1, pad=None, upsample2x: bool = False, shift=None, res=None, res_first: bool = False,
             act: int = ACT_NONE, out_scale: float = 1.0, splitk: int = 1, plant: str = ""):
    """Engine.conv2d's arithmetic: gemm_ref on the im2col matrix.  res [B, Ho, Wo, Cout].  -> gemm_ref's namespace, y / bound [B, Ho, Wo, Cout]."""
    pad = (k // 2,) * 4 if pad is None else pad
    cols, (Ho, Wo) = im2col(x, x2, k, stride, pad, upsample2x, plant)
    B, N = x.shape[0], w.shape[0]
    out = gemm_ref(dt, cols, w, bias, shift, Ho * Wo, None if res is None else res.reshape(-1, N), res_first, act, out_scale, splitk=splitk,
                   plant="" if plant == "conv_tap_off_by_one_at_border" else plant)
    for n in ("y", "y16", "bound"):
        if hasattr(out, n):
            setattr(out, n, getattr(out, n).reshape(B, Ho, Wo, N))
    return out


def conv2d_f64(x, x2, w, bias, k: int, stride: int, pad, upsample2x: bool) -> Tensor:
    """torch.nn.functional.conv2d in f64 on the same inputs -> [B, Ho, Wo, Cout]: what the im2col reference has to agree with."""
    xin = (torch.cat([x, x2], -1) if x2 is not None else x).to(F64).permute(0, 3, 1, 2)
    if upsample2x:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    t, l, b, r = (k // 2,) * 4 if pad is None else pad
    wt = w.to(F64).view(w.shape[0], k, k, -1).permute(0, 3, 1, 2)
    return F.conv2d(F.pad(xin, (l, r, t, b)), wt, None if bias is None else bias.to(F64), stride=stride).permute(0, 2, 3, 1)


# ---- LayerNorm folded into the GEMM (gemm_common.h ln_stats_step / ln_fold_apply) ----------------------------------------------------------------
def fold_layernorm(w: Tensor, gamma: Tensor, beta: Tensor, b):
    """packing.fold_layernorms on one Linear: f16 W gamma, f32 row sums of the ROUNDED matrix, c2 = W beta + b in f16 -- the kernel's inputs."""
    wg = (w.float() * gamma.float()[None, :]).to(F16)
    c1 = wg.float().sum(1).contiguous()
    c2 = (w.float() @ beta.float() + (b.float() if b is not None else 0)).to(F16)
    return wg.contiguous(), c1, c2


def ln_fold_ref(dt, x: Tensor, wg: Tensor, c1: Tensor, c2: Tensor, eps: float = 1e-5, res=None, act: int = ACT_NONE, plant: str = ""):
    """The folded formula itself from what the kernel is given (raw f16 rows x, f16 W gamma, f32 c1, f16 c2):
        rstd (sum_k x w' - mean c1) + c2,   mean, var the exact ones of the f16 row,   then the usual epilogue with c2 as the bias.
    f32: s1, s2 one-pass f32 sums, mean = s1 / K, var = max(s2 / K - mean^2, 0), rstd = rsqrt(var + eps), acc <- rstd acc + (-rstd mean) c1.
    Bound of the folded accumulator, per element (the way norm_fwd_ref.ln_bound is derived; in units u = 2^-24):
        dmean = (2 K + 4) u sum|x| / K                      fdot2 chain of K products + the cross-lane / cross-wave sums + 1 / K and its product
        dm2   = (2 K + 4) u sum x^2 / K
        dvar  = dm2 + 2 |mean| dmean + dmean^2 + 2 u (sum x^2 / K + mean^2)     relative to sum x^2 / K + mean^2, NOT to the variance
        drstd = rstd's change over [var - dvar, var + dvar] (evaluated) + 2 u rstd             the sum with eps, __frsqrt_rn
        E     = drstd |acc - mean c1| + rstd' (2 K u sum|x||w'| + dmean |c1|) + 3 u (rstd |acc| + rstd |mean c1|),   rstd' = rstd + drstd
    -rstd mean multiplies c1 with the SAME rstd the accumulator gets, so drstd scales the centred sum, not its two halves."""
    M, K = x.shape
    xs = x.to(dt)
    e = torch.tensor(eps32(eps), dtype=dt)
    acc = xs @ wg.to(dt).t()
    if dt == F64:
        mean, var = xs.mean(-1), xs.var(-1, unbiased=False)
    else:
        invk = torch.tensor(1.0, dtype=F32) / torch.tensor(float(K), dtype=F32)
        s1, s2 = xs.sum(-1), (xs * xs).sum(-1)
        mean = s1 * (torch.tensor(1.0, dtype=F32) / float(-(-K // 64) * 64) if plant == "ln_mean_of_padded_k" else invk)
        m2, mm = s2 * invk, mean * mean
        if plant == "ln_var_two_terms_f16":  # s2 / K and mean^2 each rounded to f16 before the subtraction
            m2, mm = m2.to(F16).to(F32), mm.to(F16).to(F32)
        var = (m2 - mm).clamp_min(0)
    rstd = torch.rsqrt(var + e)
    c1d = c1.to(dt)
    if dt == F64:
        zc = rstd[:, None] * (acc - mean[:, None] * c1d)
    else:
        zc = rstd[:, None] * acc + (mean * -rstd)[:, None] * c1d
    pre = None
    if dt == F64 and not plant:
        ax = x.to(F64).abs()
        m2 = (ax * ax).sum(-1) / K
        dmean = (2 * K + 4) * U32 * ax.sum(-1) / K
        dvar = (2 * K + 4) * U32 * m2 + 2 * mean.abs() * dmean + dmean * dmean + 2 * U32 * (m2 + mean * mean)
        hi, lo = torch.rsqrt((var + e - dvar).clamp_min(1e-300)), torch.rsqrt(var + e + dvar)
        drstd = torch.maximum(hi - rstd, rstd - lo) + 2 * U32 * hi
        r1 = (rstd + drstd)[:, None]
        Tw = ax @ wg.to(F64).abs().t()
        mc = mean.abs()[:, None] * c1d.abs()
        E = drstd[:, None] * (acc - mean[:, None] * c1d).abs() + r1 * (2 * K * U32 * Tw + dmean[:, None] * c1d.abs()) + 3 * U32 * rstd[:, None] * (acc.abs() + mc)
        pre = (zc, E, rstd[:, None] * (Tw + mc))
    out = gemm_ref(dt, x, wg, c2, None, 0, res, False, act, 1.0, pre=pre if pre is not None else (zc, None, None), plant=plant)
    out.mean, out.rstd = mean, rstd
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
# every distinct BM x BN of the library's tile table (tests/test_gemm_ref_cpu.py checks the list against gemm_tiles())
TILE_SHAPES = [(64, 64), (128, 64), (256, 64), (128, 128), (256, 128), (64, 160), (128, 160), (128, 256), (256, 256), (64, 320), (128, 320), (256, 320)]
SHARED_TRIPLES = [(1000, 328, 192), (300, 76, 128)]
EDGE_K = [8, 56, 64, 72, 136, 192]


def tile_triple(bm: int, bn: int, k_tail: bool = True):
    """The tile's own ragged problem: a second block with 33 live rows, a second column block with 12 live columns (N % 8 != 0: the 8-byte stores),
    K = 2 tiles of 64 + a tail of 8.  k_tail = False for the ping-pong kernel, which takes whole K tiles only (K = 192)."""
    return (bm + 33, bn + 12, 136 if k_tail else 192)


def edge_cases(bm: int, bn: int, whole_k: bool = False):
    """M in {1, 31, 33, BM - 1, BM, BM + 1}, N in {4, 8, 76, BN - 4, BN, BN + 8}, K in EDGE_K: one axis at its edge at a time.  The M list runs at K = 72 and the
    N list at K = 136 (a K tail on both); whole_k = True gives them K = 64 and K = 128 -- for the ping-pong kernel, which takes whole K tiles only
    (pp_eligible, csrc/gemm.hip: any other K runs the LDS-DMA 256 x 256 tile instead).  The K list is the same either way."""
    km, kn = (64, 128) if whole_k else (72, 136)
    cases = [(m, 76, km) for m in (1, 31, 33, bm - 1, bm, bm + 1)] + [(33, n, kn) for n in (4, 8, 76, bn - 4, bn, bn + 8)] + [(bm + 1, bn + 8, k) for k in EDGE_K]
    return list(dict.fromkeys(cases))


EDGE_TILE_SHAPES = [(128, 128), (256, 256)]  # the tiles the edge lists run on: 2 (register-staged), 9 (LDS-DMA), 16 (ring); 15 (ping-pong)
# ((M, N, K), splitk): explicit 2 and 5 slabs; 0 = the planner's own small-M split (plan_gemm: at most 16 slabs for an f16 output)
SPLITK_CASES = [((96, 320, 2560), 2), ((96, 320, 2560), 5), ((64, 1280, 11520), 0)]
AUTO_SPLITK_MAX = 16
GEGLU_CASES = [(200, 160, 136), (300, 192, 128)]  # (M, Nh, K): N = 320 (N % 128 != 0: the 8-byte stores, a ragged last block of every tile), N = 384 (the 16-byte store path)
LN_CASES = [(1000, 328, 320), (300, 192, 200)]
LN_MEANS = (0.0, 6.0, 20.0)  # |mean| / sigma of a row, cycling over the rows

FAMILIES = ["gauss", "cancel", "tiny", "wide"]


def sharp_cases():
    """The dense cases at which every plant has to show: K <= 200 and tens of thousands of elements (a rounding plant moves an element by a fraction
    of an f16 ulp; whether that crosses the bound is a matter of the element's position between two f16 values, so it needs elements)."""
    return SHARED_TRIPLES + [tile_triple(bm, bn) for bm, bn in TILE_SHAPES]


def dense_cases():
    cases = (sharp_cases() + [tile_triple(256, 256, k_tail=False)] + [c for bm, bn in EDGE_TILE_SHAPES for c in edge_cases(bm, bn)]
             + edge_cases(256, 256, whole_k=True))
    return list(dict.fromkeys(cases))


def _pm(shape, g, lo: float, hi: float) -> Tensor:
    """random signs x uniform magnitudes in [lo, hi)"""
    return (torch.rand(shape, generator=g) * (hi - lo) + lo) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


def dense_inputs(case, family: str = "gauss"):
    """-> f16 CPU x [M, K], w [N, K], bias [N], res [M, N].
    gauss   x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ 0.3 N(0, 1), res ~ N(0, 1)
    cancel  x = 2 + N(0, 1/4), w = N(0, 1 / K) + 0.5 (-1)^k: sum |x| |w| ~ K while the result is O(sqrt K) -- a reduced-precision accumulator shows at once
    tiny    operands in the NORMAL f16 range (|x| in 2^-6 [0.5, 1.5), |w| in 2^-8 K^-1/2 [0.5, 1.5) >= 1.4e-4, |bias|, |res| in 2^-13 [0.6, 1.4)), results
            around 2^-14: the f16 SUBNORMAL range and the first normal binades -- the store conversion there
    wide    gauss with a bias running linearly over N from -110 to 110: the pre-activation crosses every regime of __expf in the smooth activations,
            overflow to inf and underflow to 0 included"""
    M, N, K = case
    g = _gen(41, M, N, K, FAMILIES.index(family))
    if family == "tiny":
        x, w = _pm((M, K), g, 0.5, 1.5) * 2.0 ** -6, _pm((N, K), g, 0.5, 1.5) * 2.0 ** -8 * K ** -0.5
        b, r = _pm((N,), g, 0.6, 1.4) * 2.0 ** -13, _pm((M, N), g, 0.6, 1.4) * 2.0 ** -13
        return tuple(t.to(F16) for t in (x, w, b, r))
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    b, r = 0.3 * torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    if family == "cancel":
        x = 2 + 0.5 * x
        w = w + 0.5 * (1 - 2 * (torch.arange(K) % 2)).to(w.dtype)
    elif family == "wide":
        b = torch.linspace(-110.0, 110.0, N) if N > 1 else b
    else:
        assert family == "gauss", family
    return tuple(t.to(F16) for t in (x, w, b, r))


# the dense epilogue modes every activation is crossed with: (bias, residual, res_first, out_scale)
MODES = {
    "nobias": (False, False, False, 1.0),
    "bias": (True, False, False, 1.0),
    "bias_res": (True, True, False, 1.0),
    "bias_res_first": (True, True, True, 1.0),   # through the 1 x 1 conv2d view (Engine.linear has no residual_before_act)
    "scale": (True, True, False, 0.5),           # out_scale = 0.5 (+ bias, + residual after: so that the ORDER of the three is pinned); the 1 x 1 view too
}
ACTS = (ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_RELU)


def family_acts(family: str):
    return SMOOTH if family == "wide" else ACTS


def dense_combos(case, family: str):
    """(act, mode) pairs of a dense case: the sharp cases cross every activation with every mode on the Gaussian family; elsewhere every activation the family
    takes runs once and the modes rotate with the case."""
    acts = family_acts(family)
    if family == "gauss" and case in sharp_cases():
        return [(a, m) for a in acts for m in MODES]
    modes = list(MODES)
    return [(a, modes[(i + sum(case)) % len(modes)]) for i, a in enumerate(acts)]


def dense_ref(case, family: str, act: int, mode: str, splitk: int = 1):
    """The f64 reference namespace of one dense case / family / activation / mode: computed once, shared, to be left unchanged."""
    def make():
        x, w, b, r = dense_inputs(case, family)
        ub, ur, first, scale = MODES[mode]
        ref = gemm_ref(F64, x, w, b if ub else None, None, 0, r if ur else None, first, act, scale, splitk=splitk)
        return SimpleNamespace(y=ref.y, bound=ref.bound)  # (z and Ez dropped: 25 of these per case are kept)
    return _cached(("gemm", case, family, act, mode, splitk), make)


def dense_f32(case, family: str, act: int, mode: str, plant: str = ""):
    x, w, b, r = dense_inputs(case, family)
    ub, ur, first, scale = MODES[mode]
    return gemm_ref(F32, x, w, b if ub else None, None, 0, r if ur else None, first, act, scale, plant=plant)


# conv cases: B, H, W, C1, C2, Cout, k, stride, pad (None: k // 2 all round), upsample2x, shift, res, res_first, act, out_scale
CONV_FIELDS = ("B", "H", "W", "C1", "C2", "Cout", "k", "stride", "pad", "ups", "shift", "res", "res_first", "act", "out_scale")
CONV_CASES = [
    (3, 12, 20, 64, 0, 136, 3, 1, None, False, True, False, False, ACT_NONE, 1.0),          # ResnetBlock2D conv1 + time shift
    (2, 8, 10, 64, 64, 136, 3, 1, None, False, False, True, False, ACT_NONE, 1.0),          # virtual concat on 64-channel halves (the LDS-DMA kernels take it)
    (3, 12, 20, 64, 0, 76, 3, 2, None, False, False, True, False, ACT_SILU, 1.0),           # stride 2, ragged Cout (N % 8 != 0)
    (2, 5, 6, 8, 0, 8, 1, 1, None, False, False, True, False, ACT_NONE, 1.0),               # the smallest: 1 x 1, one 8-channel chunk
    (2, 8, 9, 24, 8, 76, 3, 1, None, False, True, True, False, ACT_SILU, 1.0),              # shift AND residual (the tile-by-tile residual path), concat inside a K tile
    (1, 7, 11, 72, 40, 136, 3, 2, None, False, False, True, False, ACT_NONE, 1.0),          # C = 112: every 64-wide K tile straddles a tap boundary; odd map, stride 2
    (2, 6, 7, 64, 0, 76, 3, 2, (0, 0, 1, 1), False, False, False, False, ACT_NONE, 1.0),    # Downsample2D's asymmetric pad
    (1, 5, 6, 24, 0, 136, 3, 1, None, True, False, True, False, ACT_NONE, 1.0),             # fused nearest-2x upsample -> 10 x 12
    (2, 9, 10, 72, 8, 8, 3, 1, None, False, False, True, True, ACT_RELU, 1.0),              # relu(conv + identity)
    (2, 12, 20, 8, 40, 76, 1, 1, None, False, False, True, False, ACT_GELU, 0.5),           # 1 x 1 over a concat, out_scale + residual
    (3, 6, 8, 72, 0, 136, 3, 1, None, False, True, False, False, ACT_QUICK_GELU, 0.5),      # shift, QuickGELU, out_scale
]
CONV_EVERY_TILE = [CONV_CASES[1], CONV_CASES[2]]


def conv_id(case) -> str:
    c = SimpleNamespace(**dict(zip(CONV_FIELDS, case)))
    return (f"b{c.B}-{c.H}x{c.W}-{c.C1}+{c.C2}-{c.Cout}-k{c.k}s{c.stride}" + ("-pad0011" if c.pad else "") + ("-ups" if c.ups else "") + ("-shift" if c.shift else "")
            + ("-res" if c.res else "") + ("first" if c.res_first else "") + f"-{ACT_NAME[c.act]}" + (f"-x{c.out_scale}" if c.out_scale != 1.0 else ""))


def conv_inputs(case):
    """-> namespace of f16 CPU tensors x, x2 (or None), w [Cout, k k (C1 + C2)] packed, bias, shift (or None), res (or None), and the case's fields."""
    c = SimpleNamespace(**dict(zip(CONV_FIELDS, case)))
    g = _gen(43, *[int(v) for v in case if isinstance(v, (int, bool))])
    Kc = c.k * c.k * (c.C1 + c.C2)
    c.x = torch.randn(c.B, c.H, c.W, c.C1, generator=g).to(F16)
    c.x2 = torch.randn(c.B, c.H, c.W, c.C2, generator=g).to(F16) if c.C2 else None
    c.w = (torch.randn(c.Cout, Kc, generator=g) * Kc ** -0.5).to(F16)
    c.bias = (0.3 * torch.randn(c.Cout, generator=g)).to(F16)
    pad = (c.k // 2,) * 4 if c.pad is None else c.pad
    Hin, Win = (2 * c.H, 2 * c.W) if c.ups else (c.H, c.W)
    c.Ho, c.Wo = (Hin + pad[0] + pad[2] - c.k) // c.stride + 1, (Win + pad[1] + pad[3] - c.k) // c.stride + 1
    c.shift_t = torch.randn(c.B, c.Cout, generator=g).to(F16) if c.shift else None
    c.res_t = torch.randn(c.B, c.Ho, c.Wo, c.Cout, generator=g).to(F16) if c.res else None
    return c


def conv_case_ref(dt, c, plant: str = ""):
    return conv_ref(dt, c.x, c.x2, c.w, c.bias, c.k, c.stride, c.pad, c.ups, c.shift_t, c.res_t, c.res_first, c.act, c.out_scale, plant=plant)


def conv_fixture(case):
    """(inputs namespace, f64 reference namespace): computed once, shared, to be left unchanged."""
    def make():
        c = conv_inputs(case)
        return c, conv_case_ref(F64, c)
    return _cached(("conv", case), make)


def ln_inputs(case, nh: int = 0, means=None):
    """-> f16 CPU x [M, K] (rows of spread 0.7 around means of 0, 6 and 20 spreads, signs alternating), w [N, K], b [N], gamma, beta [K], res [M, N].
    nh > 0: N = 2 nh rows, hidden then gate (to be packed)."""
    M, N, K = case
    g = _gen(47, M, N, K, nh)
    means = LN_MEANS if means is None else means
    lvl = torch.tensor(means)[torch.arange(M) % len(means)] * (1 - 2 * ((torch.arange(M) // len(means)) % 2)).to(F32)
    x = (0.7 * torch.randn(M, K, generator=g) + 0.7 * lvl[:, None]).to(F16)
    w, b = (torch.randn(N, K, generator=g) * K ** -0.5).to(F16), (0.3 * torch.randn(N, generator=g)).to(F16)
    gamma, beta = (1.0 + 0.3 * torch.randn(K, generator=g)).to(F16), (0.2 * torch.randn(K, generator=g)).to(F16)
    return x, w, b, gamma, beta, torch.randn(M, N, generator=g).to(F16)


def ln_shape(case, kind: str):
    """(M, N, K) of a LayerNorm-fold case under an epilogue kind: GEGLU needs whole 64-column hidden | gate blocks (328 -> 320), the q | k | V^T form three
    equal projections of a multiple of 32 columns (328 -> 288)."""
    M, N, K = case
    return (M, N // 64 * 64 if kind == "geglu" else N // 96 * 96 if kind == "qkv" else N, K)


def ln_fixture(case, kind: str, means=None):
    """kind 'res' (plain + residual), 'gelu', 'geglu' (w packed; N = 2 Nh), 'qkv' (no bias: c2 = W beta) -> (x, wg, c1, c2, res or None, f64 reference)."""
    def make():
        x, w, b, gamma, beta, r = ln_inputs(ln_shape(case, kind), nh=int(kind == "geglu"), means=means)
        if kind == "geglu":
            w, b = pack_geglu_rows(w), pack_geglu_rows(b)
        wg, c1, c2 = fold_layernorm(w, gamma, beta, None if kind == "qkv" else b)
        res = r if kind == "res" else None
        act = {"res": ACT_NONE, "gelu": ACT_GELU, "geglu": ACT_GEGLU, "qkv": ACT_NONE}[kind]
        return x, wg, c1, c2, res, ln_fold_ref(F64, x, wg, c1, c2, 1e-5, res, act)
    return _cached(("ln", case, kind, means), make)


LN_KINDS = ("res", "gelu", "geglu", "qkv")


def ln_f32(case, kind: str, plant: str = "", means=None):
    x, wg, c1, c2, res, _ = ln_fixture(case, kind, means)
    act = {"res": ACT_NONE, "gelu": ACT_GELU, "geglu": ACT_GEGLU, "qkv": ACT_NONE}[kind]
    return ln_fold_ref(F32, x, wg, c1, c2, 1e-5, res, act, plant=plant)


def geglu_inputs(case):
    """-> f16 CPU x [M, K], packed w [2 Nh, K], packed bias [2 Nh]."""
    M, Nh, K = case
    x, w, b, _ = dense_inputs((M, 2 * Nh, K), "gauss")
    return x, pack_geglu_rows(w), pack_geglu_rows(b)


def geglu_fixture(case):
    def make():
        x, wp, bp = geglu_inputs(case)
        return x, wp, bp, gemm_ref(F64, x, wp, bp, act=ACT_GEGLU)
    return _cached(("geglu", case), make)


# ---- K_ACT ----------------------------------------------------------------------------------------------------------------------------------------
def measure_k_act(verbose: bool = False) -> dict:
    """K_ACT_MEASURED re-measured: every activation on the f32 pre-activations (bias and the residual before the activation included) of every dense
    case x family, of the split-K, GEGLU, conv and LayerNorm-fold cases."""
    worst, where = {n: 0.0 for n in K_ACT_MEASURED}, {}

    def upd(z32, tag):
        for a in SMOOTH:
            v = act_k(a, z32)
            if v > worst[ACT_NAME[a]]:
                worst[ACT_NAME[a]], where[ACT_NAME[a]] = v, tag

    for case in dense_cases() + [c for c, _ in SPLITK_CASES[1:]]:
        for fam in FAMILIES:
            x, w, b, r = dense_inputs(case, fam)
            acc = x.float() @ w.float().t()
            upd(acc + b.float(), (case, fam))
            upd(acc + b.float() + r.float(), (case, fam, "res first"))
    for case in GEGLU_CASES:
        x, wp, bp = geglu_inputs(case)
        upd(split_geglu(x.float() @ wp.float().t() + bp.float())[1], ("geglu", case))
    for case in CONV_CASES:
        c = conv_inputs(case)
        cols, _ = im2col(c.x, c.x2, c.k, c.stride, (c.k // 2,) * 4 if c.pad is None else c.pad, c.ups)
        upd(cols.float() @ c.w.float().t() + c.bias.float(), ("conv", conv_id(case)))
    for case in LN_CASES:
        x, wg, c1, c2, _, _ = ln_fixture(case, "gelu")
        upd(ln_fold_ref(F32, x, wg, c1, c2, 1e-5, None, ACT_NONE).y, ("ln", case))
    if verbose:
        for n, tag in where.items():
            print(n, "worst at", tag)
    return worst


if __name__ == "__main__":
    for n, v in measure_k_act(verbose=True).items():
        print(f'    "{n}": {v:.4g},')
