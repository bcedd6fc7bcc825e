"""CPU references and derived per-element error bounds for the FORWARD normalisation kernels (csrc/norm.hip: layernorm_kernel<CH, ROWS>,
gn_fused_kernel, gn_stats / gn_finalize / gn_apply, the apply-from-bridge-statistics branch of gn_apply_kernel, the statistics-only call) and
softmax_rows_kernel (csrc/elementwise.hip): tests/test_norm_fwd_cpu.py, tests/test_norm_fwd_gpu.py.

TEST INFRASTRUCTURE ONLY, in the manner of tests/norm_bwd_ref.py, whose helpers it imports: torch on the CPU, evaluated from the kernels' own f16
inputs; nothing here goes through genima_amd.  Every ``_xxx(dt, ...)`` function holds one operation twice: dt = float64 is the closed form,
dt = float32 restates the kernel's arithmetic in its order of operations and its reduction shape.

THE BOUNDS.  For every output element
    |got - ref| <= 1/2 ulp16(ref) + K * 2^-24 * T
T is written out beside each function: the magnitudes that enter the element before they cancel.  Where an activation follows, the whole
pre-activation error is carried through it by the LARGEST slope on the interval it spans (silu_slope_max: evaluated, not linearised at the
point).  K = MARGIN x the largest |f32 restatement - f64| / (2^-24 T) over every case and family of the lists below (K_MEASURED, re-measured by
tests/test_norm_fwd_cpu.py::test_constants_are_the_measured_ones).  The GroupNorm output inherits the error of the statistics behind it as
|x| b_a + b_sh with (b_a, b_sh) the scale / shift bounds of the route that produced them (norm_bwd_ref.gn_saved_bounds; stats_in_bound for the
bridge).  No element is masked or left out.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

from act_ops_ref import ulp16
from norm_bwd_ref import (EPS, FWD_CASES, FWD_THREE, MARGIN, U32, _cached, _gen, _gn_saved, _pad_to, _seq, _wave_sum, _worst, _x_family, assert_within, breaks,
                          eps32, gn_fwd_route, gn_id, gn_inputs, gn_pick_chunks, gn_saved_bounds, gn_saved_f32, gn_saved_ref, ln_id)

Tensor = torch.Tensor
F64, F32, F16 = torch.float64, torch.float32, torch.float16
ACT_NONE, ACT_SILU = 0, 1
# largest |f32 restatement - f64| / (2^-24 T) over all cases x families (CPU); K = MARGIN x this
K_MEASURED = {
    "ln_y": 2.62,        # (8191, 320) tailmark
    "gn_z": 1.986,       # x a + s from the f32 (a, s) the kernel holds: two roundings; (1, 1024, 320, 0, 32) tailmark
    "silu": 1.956,       # z / (1 + e^-z) on the f32 z; (1, 4096, 512, 0, 32) tailmark
    "softmax_y": 0.9425, # (5, 8) valid 5 scale 0.125
}
K = {n: MARGIN * v for n, v in K_MEASURED.items()}
# median bound / |ref| over the Gaussian cases (CPU, test_the_bounds_are_not_vacuous): a correctly rounded f16 store alone is <= 2^-11 = 4.9e-4
TIGHTNESS = {"ln": 3.49e-4, "gn": 3.57e-4, "stats_in": 3.52e-4, "softmax": 3.53e-4}
FAMILIES = ["gauss", "offset", "lowvar", "tailmark"]


def old_bar_passes(got: Tensor, ref: Tensor) -> bool:
    """tests/util.py::assert_close as a predicate: relative L2 <= 1e-3 and every element within 2e-3 max|ref| + 1e-3."""
    g, r = got.to(F32).to(F64), ref.to(F32).to(F64)
    return bool((g - r).norm() / r.norm().clamp_min(1e-30) <= 1e-3) and bool((g - r).abs().max() <= 2e-3 * float(r.abs().max()) + 1e-3)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def ln_fwd_route(M: int, C: int):
    """-> (CH, ROWS) of layernorm_kernel<CH, ROWS> as gn_layernorm_fwd picks them."""
    ch = (C + 511) // 512
    if ch == 1:
        return 1, (4 if M >= 8192 else 2 if M >= 2048 else 1)
    if ch == 2:
        return 2, (2 if M >= 4096 else 1)
    return (4, 1) if ch <= 4 else (8, 1)


LN_ROUTES = [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (4, 1), (8, 1)]


def _ln_fwd(dt, x: Tensor, gamma: Tensor, beta: Tensor, eps: float = EPS, plant: str = ""):
    """LayerNorm over the rows of x [M, C] -> namespace y [M, C] (before the f16 store), mean, rstd [M].
        mean = sum x / C,  rstd = (sum (x - mean)^2 / C + eps)^-1/2,  y = (x - mean) rstd gamma + beta.
    f32: lane l of the row's wave owns the 8-channel chunks l, l + 64, .. (CH of them; lanes past the row hold zeros), chains its CH x 8
    elements, then wave_sum; the second pass chains (x - mean)^2 over the LIVE chunks only.  ROWS changes which wave owns a row, not its sums.
    ``plant``: one deliberate error (tests/test_norm_fwd_cpu.py).
    Magnitudes (f64, no plant), xh = (x - mean) rstd:
        T = 3/2 |xh gamma| + |beta| + rstd |gamma| mean|x|
    |xh gamma| + |beta| are the terms of the sum; an error of 2^-24 mean|x| in the mean shifts every y of the row by rstd |gamma| times it
    (to first order it leaves the variance alone: sum (x - mean) = 0); a relative error d of the variance moves rstd by d / 2."""
    M, C = x.shape
    CH, _ = ln_fwd_route(M, C)
    W = CH * 512
    xp, g, b = _pad_to(x.to(dt), 1, W), _pad_to(gamma.to(dt), 0, W), _pad_to(beta.to(dt), 0, W)
    e = torch.tensor(eps32(eps), dtype=dt)
    live = (torch.arange(W) < C).to(dt)
    if plant == "dead_lanes_in_variance":  # the lanes >= CC of the last chunk add (0 - mean)^2
        live = torch.ones(W, dtype=dt)
    if plant == "last_chunk_params":       # gamma / beta of the last chunk taken from the chunk before
        g, b = g.clone(), b.clone()
        g[C - 8:C], b[C - 8:C] = g[C - 16:C - 8].clone(), b[C - 16:C - 8].clone()

    def rowsum(t):  # [M, W] -> [M]
        if dt == F64:
            return t.sum(-1)
        lanes = t.reshape(M, CH, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, CH * 8)
        return _wave_sum(_seq(lanes, 2, dt), dt)

    Cf = torch.tensor(float(C), dtype=dt)
    mean = rowsum(xp) / Cf
    d = xp - mean[:, None]
    var = rowsum(d * d * live) / (Cf - 1 if plant == "variance_over_n_minus_1" else Cf)
    rstd = 1.0 / (torch.sqrt(var) + e) if plant == "eps_outside_sqrt" else torch.rsqrt(var + e)
    y = ((d * rstd[:, None]) * g + b)[:, :C]
    if plant == "last_row_unnormalised":   # the last live row of a ROWS > 1 wave
        y = y.clone()
        y[M - 1] = x[M - 1].to(dt)
    out = SimpleNamespace(y=y, mean=mean, rstd=rstd)
    if dt == F64 and not plant:
        xs = x.to(F64)
        out.T = 1.5 * y.sub(b[:C]).abs() + b[:C].abs() + (rstd * xs.abs().mean(-1))[:, None] * g[:C].abs()
    return out


def ln_fwd_ref(x, gamma, beta, eps: float = EPS, plant: str = ""):
    return _ln_fwd(F64, x, gamma, beta, eps, plant)


def ln_fwd_f32(x, gamma, beta, eps: float = EPS):
    """The kernel's arithmetic on the CPU; y before its f16 store in y32.  No GPU test compares against it."""
    out = _ln_fwd(F32, x, gamma, beta, eps)
    out.y32, out.y = out.y, out.y.to(F16)
    return out


def ln_bound(ref) -> Tensor:
    return 0.5 * ulp16(ref.y) + K["ln_y"] * U32 * ref.T


# ---- the apply step: y = act(x a + s) -----------------------------------------------------------------------------------------------------
SILU_ZSTAR, SILU_SMAX, SILU_SMIN = 2.3993572805154676, 1.09983933, 0.09983933  # silu'' = 0 at +-z*; silu'(z*) and -silu'(-z*), rounded up


def _silu(z: Tensor) -> Tensor:
    """common.h act_silu: x / (1 + __expf(-x))."""
    return z / (1.0 + torch.exp(-z))


def _silu_slope(z: Tensor) -> Tensor:
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def silu_slope_max(lo: Tensor, hi: Tensor) -> Tensor:
    """max |silu'| over [lo, hi]: silu' rises from its minimum -0.0998 at -z* to its maximum 1.0998 at +z* and is monotone on either side, so the
    largest magnitude sits at an end of the interval or at whichever of +-z* it holds."""
    m = torch.maximum(_silu_slope(lo).abs(), _silu_slope(hi).abs())
    m = torch.where((lo < SILU_ZSTAR) & (hi > SILU_ZSTAR), torch.full_like(m, SILU_SMAX), m)
    return torch.where((lo < -SILU_ZSTAR) & (hi > -SILU_ZSTAR), m.clamp_min(SILU_SMIN), m)


def _apply(dt, x: Tensor, a: Tensor, s: Tensor, act: int):
    """y = act(x a + s), x [B, HW, C] f16, a, s [B, C] AS GIVEN (f32 or f64 values) -> (y, z)."""
    z = x.to(dt) * a.to(dt)[:, None] + s.to(dt)[:, None]
    return (_silu(z) if act == ACT_SILU else z), z


def apply_bound(x: Tensor, a: Tensor, s: Tensor, b_a: Tensor, b_sh: Tensor, act: int):
    """Bound of f16(act(x a' + s')) against ref = act(x a + s) (f64), where the kernel's (a', s') are within (b_a, b_sh) of (a, s) [B, C]:
        E_z = K_z 2^-24 T_z + |x| b_a + b_sh,   T_z = |x a| + |s|          the pre-activation
        bound = 1/2 ulp16(ref) + S E_z + K_silu 2^-24 T_act
    S = 1 and T_act = 0 without activation; with SiLU S = silu_slope_max over [z - E_z, z + E_z] and T_act = |y| (1 + (1 + |z|) (1 - sigma(z))):
    the quotient's own roundings, and the fast exponential's relative (1 + |z|) 2^-24 which reaches y through e^-z / (1 + e^-z) = 1 - sigma.
    -> (ref y, bound)."""
    y, z = _apply(F64, x, a, s, act)
    ax = x.to(F64).abs()
    Ez = K["gn_z"] * U32 * (ax * a.to(F64).abs()[:, None] + s.to(F64).abs()[:, None]) + ax * b_a[:, None] + b_sh[:, None]
    if act != ACT_SILU:
        return y, 0.5 * ulp16(y) + Ez
    sg = 1.0 / (1.0 + torch.exp(-z))
    return y, 0.5 * ulp16(y) + silu_slope_max(z - Ez, z + Ez) * Ez + K["silu"] * U32 * y.abs() * (1 + (1 + z.abs()) * (1 - sg))


def apply_k(x: Tensor, a32: Tensor, s32: Tensor) -> dict:
    """The two constants of the apply step, measured on the f32 (a, s) a kernel would hold: |z32 - z64| / (2^-24 T_z) and, on the f32 z,
    |silu32(z) - silu64(z)| / (2^-24 T_act)."""
    (y32, z32), (_, z64) = _apply(F32, x, a32, s32, ACT_SILU), _apply(F64, x, a32, s32, ACT_NONE)
    Tz = x.to(F64).abs() * a32.to(F64).abs()[:, None] + s32.to(F64).abs()[:, None]
    zz = z32.to(F64)
    sg = 1.0 / (1.0 + torch.exp(-zz))
    return {"gn_z": _worst(z32, z64, Tz), "silu": _worst(y32, _silu(zz), _silu(zz).abs() * (1 + (1 + zz.abs()) * (1 - sg)))}


# ---- GroupNorm y on the fused and the three-launch route ----------------------------------------------------------------------------------------
def _cat(x1, x2):
    return torch.cat([x1, x2], -1) if x2 is not None else x1


def _gn_fwd(dt, x1, x2, gamma, beta, G: int, act: int, route: str, eps: float = EPS, plant: str = ""):
    """GroupNorm(+SiLU) of the concat x1 | x2 [B, HW, C] -> namespace y (before the f16 store), sv (norm_bwd_ref._gn_saved).
    f32, route 'fused' (gn_fused_kernel): a0 = rstd gamma, s0 = beta - mean a0 from the kernel's f32 statistics, y = act(x a0 + s0); route 'three'
    (gn_apply_kernel): the same from the scsh gn_finalize_kernel wrote.  T: apply_bound."""
    x = _cat(x1, x2)
    sv = _gn_saved(dt, x, gamma, beta, G, eps, route)
    a, s = sv.scsh[..., 0], sv.scsh[..., 1]
    if plant == "stats_of_x1_only":  # the group straddling x | x2 takes its statistics from its x1 channels alone
        C1, cpg = x1.shape[-1], x.shape[-1] // G
        g0 = C1 // cpg
        part = x[..., g0 * cpg:C1].to(dt)
        mu, r = part.mean((1, 2)), torch.rsqrt(part.var((1, 2), unbiased=False) + eps32(eps))
        a, s = a.clone(), s.clone()
        sl = slice(g0 * cpg, (g0 + 1) * cpg)
        a[:, sl] = r[:, None] * gamma[sl].to(dt)
        s[:, sl] = beta[sl].to(dt) - mu[:, None] * a[:, sl]
    if plant == "silu_before_affine":
        y = _silu(x.to(dt)) * a[:, None] + s[:, None]
    else:
        y = _apply(dt, x, a, s, act)[0]
    return SimpleNamespace(y=y, sv=sv)


def gn_fwd_f32(x1, x2, gamma, beta, G: int, act: int, route: str):
    out = _gn_fwd(F32, x1, x2, gamma, beta, G, act, route)
    out.y32, out.y = out.y, out.y.to(F16)
    return out


def gn_fwd_bound(x1, x2, gamma, beta, sv, act: int):
    """(ref y, bound) of a fused / three-launch GroupNorm from its f64 saved reference ``sv``."""
    b = gn_saved_bounds(sv, gamma, beta)["scsh"]
    return apply_bound(_cat(x1, x2), sv.scsh[..., 0], sv.scsh[..., 1], b[..., 0], b[..., 1], act)


# ---- GroupNorm from bridge statistics (stats_in) ------------------------------------------------------------------------------------------------
STATS_LINE, FIX, FIXSQ = 16, float(1 << 24), float(1 << 12)  # GN_STATS_LINE, 2^GN_STATS_SHIFT, 2^GN_STATS_SHIFT_SQ
STATS_SENTINEL = 0x5A5A5A5A5A5A5A5A


def host_stats_block(x: Tensor, G: int, reps: int, seed: int = 0) -> Tensor:
    """The statistics block int64 [reps, B, G, 16] of x [B, HW, C] (the concat), built on the host as tests/test_gn_bridge_gpu.py::_host_stats
    does: word 0 = round(sum 2^24), word 1 = round(sum of squares 2^12), the integer totals split at random (negative parts included) over
    the replicas; words 2 .. 15 hold a sentinel the consumer must ignore."""
    B, HW, C = x.shape
    xg = x.to(F64).reshape(B, HW, G, C // G)
    tot = torch.stack([xg.sum((1, 3)).mul(FIX).round().to(torch.int64), (xg * xg).sum((1, 3)).mul(FIXSQ).round().to(torch.int64)], -1)
    blk = torch.full((reps, B, G, STATS_LINE), STATS_SENTINEL, dtype=torch.int64)
    parts = torch.randint(-(1 << 40), 1 << 40, (max(reps - 1, 0), B, G, 2), generator=_gen(23, B, HW, C, G, reps, seed), dtype=torch.int64)
    blk[:reps - 1, ..., :2] = parts
    blk[reps - 1, ..., :2] = tot - parts.sum(0)
    return blk


def _gn_stats_in(dt, x: Tensor, gamma, beta, blk: Tensor, G: int, act: int, eps: float = EPS, plant: str = ""):
    """gn_apply_kernel's stats_in branch, from the block the kernel is handed: per (b, g) the replicas' words summed AS INTEGERS (S0, S1),
        m = S0 2^-24 / n,  var = max(S1 2^-12 / n - m^2, 0),  rstd = (var + eps)^-1/2        (f64 in the kernel too: gn_group_mean_rstd)
        a = rstd gamma,  s = beta - m a,  y = act(x a + s)                                     (f32 in the kernel, from f32(m), f32(rstd))
    so the quantisation of the bridge is an input, not an error.  -> namespace y, mean, rstd [B, G], a, s [B, C]."""
    B, HW, C = x.shape
    cpg = C // G
    use = blk[:8] if plant == "ninth_replica_dropped" else blk
    S = use[..., :2].sum(0)  # int64
    inv = 1.0 / (float(HW) * float(cpg))
    m = S[..., 0].to(F64) * (1.0 / FIX) * inv
    var = (S[..., 1].to(F64) * (1.0 / FIXSQ) * inv - m * m).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps32(eps))
    m, rstd = m.to(dt), rstd.to(dt)
    grp = torch.arange(C) // cpg
    if plant == "chunk_first_group":  # all 8 channels of a chunk given the group of the chunk's first channel
        grp = (torch.arange(C) // 8 * 8) // cpg
    a = rstd[:, grp] * gamma.to(dt)
    s = beta.to(dt) - m[:, grp] * a
    return SimpleNamespace(y=_apply(dt, x, a, s, act)[0], mean=m, rstd=rstd, a=a, s=s)


def stats_in_bound(x: Tensor, gamma, beta, ref, act: int):
    """(ref y, bound).  The kernel's f32 (a, s) against the f64 ones, roundings of 2^-24 counted: 1 for f32(m); 2 for rstd (its f64 evaluation
    and the f32 store -- the f64 cancellation of S1 / n - m^2 is 2^-53 m^2 / (var + eps), nothing here); 1 for rstd gamma; 2 for m a and the
    difference.  The same form as norm_bwd_ref.gn_saved_bounds without its summation terms: the sums are exact integers."""
    grp = torch.arange(x.shape[-1]) // (x.shape[-1] // ref.mean.shape[1])
    am, g = ref.mean.abs()[:, grp], gamma.to(F64).abs()
    b_a = 2 * U32 * ref.rstd[:, grp] * g + U32 * ref.a.abs()
    b_sh = am * b_a + ref.a.abs() * U32 * am + 2 * U32 * (am * ref.a.abs() + beta.to(F64).abs())
    return apply_bound(x, ref.a, ref.s, b_a, b_sh, act)


# ---- softmax_rows -------------------------------------------------------------------------------------------------------------------------------
def _softmax(dt, x: Tensor, scale: float, valid: int, plant: str = ""):
    """softmax_rows_kernel over x [rows, cols] f16: v = x scale (columns >= valid: -inf), e = exp(v - max v), y = e (1 / sum e); columns >= valid
    come out as zeros.  f32: lane l chains the e of its chunks l, l + 64, .. (8 each), then wave_sum.  -> (y before the f16 store, T):
        T = y (t + sum_j y_j t_j),   t = 1 + |v| + |max v| + |v - max v|
    the roundings of x scale at both ends of v - max, of the difference, and the fast exponential's relative |v - max| 2^-24; the same,
    weighted by y_j, for the sum; 1 for the reciprocal and the product."""
    rows, cols = x.shape
    sc = torch.tensor(scale, dtype=F32).to(dt)
    masked = torch.arange(cols) >= valid
    v_all = x.to(dt) * sc
    v = v_all.masked_fill(masked, float("-inf"))
    if plant == "masked_columns_given_mass":  # the mask is not applied at all
        v = v_all
    mx = v.max(-1).values
    e = torch.exp(v - mx[:, None])
    es = torch.exp(v_all - mx[:, None]) if plant == "row_sum_before_mask" else e
    if dt == F64:
        tot = es.sum(-1)
    else:
        lanes = _pad_to(es, 1, 4096).reshape(rows, 8, 64, 8).permute(0, 2, 1, 3).reshape(rows, 64, 64)
        tot = _wave_sum(_seq(lanes, 2, dt), dt)
    y = e * (1.0 / tot)[:, None]
    T = None
    if dt == F64 and not plant:
        vv = v_all.masked_fill(masked, 0.0)
        t = 1 + vv.abs() + mx.abs()[:, None] + (vv - mx[:, None]).abs()
        T = y * (t + (y * t).sum(-1, keepdim=True))
    return y, T


def softmax_ref(x, scale: float, valid: int, plant: str = ""):
    return _softmax(F64, x, scale, valid, plant)


def softmax_bound(y: Tensor, T: Tensor) -> Tensor:
    return 0.5 * ulp16(y) + K["softmax_y"] * U32 * T


# ---- cases and inputs -------------------------------------------------------------------------------------------------------------------------
LN_CASES = ([(M, C) for C in (8, 320, 512, 520, 1024, 1032, 2048, 2056, 4096) for M in (1, 3, 5)]
            + [(M, 320) for M in (2047, 2048, 2049, 8191, 8192, 8193)] + [(M, 520) for M in (4095, 4096, 4097)] + [(8195, 64)])
# (B, HW, C1, C2, G)
GN_THREE_MORE = [
    (1, 1024, 2560, 0, 32),    # CC = 320 > 256: the cx += TX loop of gn_stats_kernel and gn_apply_kernel
    (1, 4096, 328, 184, 32),   # cpg = 16: group 20 = channels 320 .. 335 straddles x | x2 at 328
    (1, 4100, 512, 0, 32),     # ragged apply slab: HW outside the four-rows-in-flight trip
]
GN_CASES = FWD_CASES + GN_THREE_MORE
GN_ROUTE = {c: ("three" if c in GN_THREE_MORE or c in FWD_THREE else "fused") for c in GN_CASES}
STATS_ONLY_CASES = [(2, 64, 320, 0, 32), (2, 64, 72, 0, 8)]  # fused-eligible; three-launch (odd cpg)
# (B, HW, C1, C2, G, replicas): every cpg of (2, 4, 10, 12, 20, 30, 80, 256) at HW 9, 64, 1000, the replica count rotating so that every cpg and
# every HW meets 1, 3 and 9; and a concatenated input
_SI_G = {2: 32, 4: 32, 10: 32, 12: 8, 20: 32, 30: 32, 80: 32, 256: 2}
SI_CASES = [(1 if cpg == 80 else 2, HW, cpg * _SI_G[cpg], 0, _SI_G[cpg], (1, 3, 9)[(i + j) % 3])
            for i, cpg in enumerate((2, 4, 10, 12, 20, 30, 80, 256)) for j, HW in enumerate((9, 64, 1000))] + [(2, 64, 640, 320, 32, 9)]
SOFTMAX_CASES = [(rows, cols) for cols in (8, 72, 256, 520, 4096) for rows in (1, 5, 33)]
SOFTMAX_SCALES = (1.0, 0.125)


def softmax_valids(cols: int):
    return (cols, cols - 3, 1)


def _mark(t: Tensor, g, shift: float) -> Tensor:
    return 4 * torch.randn(t.shape, generator=g) + shift


def ln_inputs(case, family: str):
    """-> f16 CPU x [M, C], gamma, beta [C].  tailmark: the last row and the last 8-channel chunk stand out (x 4, shifted by +-3)."""
    M, C = case
    g = _gen(29, M, C, FAMILIES.index(family))
    x = _x_family((M, C), "gauss" if family == "tailmark" else family, g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    if family == "tailmark":
        x[M - 1] = _mark(x[M - 1], g, 3.0)
        x[:, C - 8:] = _mark(x[:, C - 8:], g, -3.0)
    return x.to(F16), gamma.to(F16), beta.to(F16)


def gn_fwd_inputs(case, family: str):
    """-> f16 CPU x1, x2 (or None), gamma, beta.  gauss / offset / lowvar: norm_bwd_ref.gn_inputs.  tailmark: the last pixel, the last 8-channel
    chunk and the last channel of every group (so the last channel of a straddling group too) stand out."""
    B, HW, C1, C2, G = case[:5]
    if family != "tailmark":
        return gn_inputs(case[:5], family)[:4]
    C = C1 + C2
    g = _gen(31, B, HW, C1, C2, G)
    x = torch.randn(B, HW, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    x[:, HW - 1] = _mark(x[:, HW - 1], g, 3.0)
    x[..., C - 8:] = _mark(x[..., C - 8:], g, -3.0)
    last = torch.arange(C) % (C // G) == C // G - 1
    x[..., last] = _mark(x[..., last], g, 2.0)
    x = x.to(F16)
    return x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None), gamma.to(F16), beta.to(F16)


def softmax_inputs(case):
    """f16 scores [rows, cols] x 3; with more than one row, row 1 carries a spike of +60 at its first column and row 2 equal scores."""
    rows, cols = case
    x = 3 * torch.randn(rows, cols, generator=_gen(37, rows, cols))
    if rows > 2:
        x[1, 0] = 60.0
        x[2] = 1.5
    return x.to(F16)


def ln_fixture(case, family: str):
    """(x, gamma, beta, ref, bound), computed once and shared: leave it unchanged."""
    def make():
        x, gamma, beta = ln_inputs(case, family)
        ref = ln_fwd_ref(x, gamma, beta)
        return x, gamma, beta, ref, ln_bound(ref)
    return _cached(("lnf", case, family), make)


def gn_fixture(case, family: str):
    """(x1, x2, gamma, beta, sv) with sv the f64 saved reference: shared, leave it unchanged."""
    def make():
        x1, x2, gamma, beta = gn_fwd_inputs(case, family)
        return x1, x2, gamma, beta, gn_saved_ref(x1, x2, gamma, beta, case[4])
    return _cached(("gnf", case, family), make)


def si_fixture(case, family: str):
    """(x [B, HW, C], x1, x2, gamma, beta, block) of a stats_in case: shared, leave it unchanged."""
    def make():
        x1, x2, gamma, beta = gn_fwd_inputs(case, family)
        x = _cat(x1, x2)
        return x, x1, x2, gamma, beta, host_stats_block(x, case[4], case[5], FAMILIES.index(family))
    return _cached(("sif", case, family), make)


def si_id(case) -> str:
    return "x".join(str(i) for i in case[:5]) + f"-r{case[5]}"


def measure_constants(verbose: bool = False) -> dict:
    """The K_MEASURED figures, re-measured over every case x family."""
    worst, where = {n: 0.0 for n in K_MEASURED}, {}

    def upd(name, v, tag):
        if v > worst[name]:
            worst[name], where[name] = v, tag

    for case in LN_CASES:
        for fam in FAMILIES:
            x, gamma, beta, ref, _ = ln_fixture(case, fam)
            upd("ln_y", _worst(ln_fwd_f32(x, gamma, beta).y32, ref.y, ref.T), (case, fam))
    for case in GN_CASES:
        for fam in FAMILIES:
            x1, x2, gamma, beta, _ = gn_fixture(case, fam)
            s32 = gn_saved_f32(x1, x2, gamma, beta, case[4], route=GN_ROUTE[case]).scsh
            for n, v in apply_k(_cat(x1, x2), s32[..., 0], s32[..., 1]).items():
                upd(n, v, (case, fam))
    for case in SI_CASES:
        for fam in FAMILIES:
            x, _, _, gamma, beta, blk = si_fixture(case, fam)
            r32 = _gn_stats_in(F32, x, gamma, beta, blk, case[4], ACT_NONE)
            for n, v in apply_k(x, r32.a, r32.s).items():
                upd(n, v, (case, fam))
    for case in SOFTMAX_CASES:
        x = softmax_inputs(case)
        for valid in softmax_valids(case[1]):
            for scale in SOFTMAX_SCALES:
                (y64, T), (y32, _) = _softmax(F64, x, scale, valid), _softmax(F32, x, scale, valid)
                upd("softmax_y", _worst(y32, y64, T), (case, valid, scale))
    if verbose:
        for n, tag in where.items():
            print(n, "worst at", tag)
    return worst


if __name__ == "__main__":
    for n, v in measure_constants(verbose=True).items():
        print(f'    "{n}": {v:.4g},')
