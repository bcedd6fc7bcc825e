"""CPU references and derived per-element error bounds for the LayerNorm / GroupNorm(+SiLU) backward (csrc/backward.hip: layernorm_bwd_kernel,
gnb_partial / gnb_finalize / gnb_param / gnb_apply), the statistics the GroupNorm forward saves for it (csrc/norm.hip: gn_fused_kernel and the
three-launch gn_stats / gn_finalize path) and their pointwise neighbours act_bwd, geglu_bwd, softmax_bwd:
tests/test_norm_bwd_cpu.py, tests/test_norm_bwd_gpu.py.

TEST INFRASTRUCTURE ONLY, in the manner of tests/attention_ref.py: torch on the CPU, evaluated from the kernels' own f16 inputs; nothing here goes
through genima_amd.  Every ``_xxx(dt, ...)`` function holds one operation twice: dt = float64 is the closed-form reference, dt = float32 restates
the kernel's f32 arithmetic -- the same order of operations and the same reduction shape (which thread adds what, in which order, and how the
partial sums fold) -- so that the constants of the bounds are measured on the CPU and never taken from a GPU run.

THE BOUNDS.  For every output element
    |got - ref| <= 1/2 ulp16(ref)          the store (f16 outputs only; the f32 outputs dgamma / dbeta / stats / scsh have no such term -- dgamma and
                                           dbeta have 2^-24 (|prior| + |sum|) instead, the one f32 addition onto what the buffer held)
                 + K * 2^-24 * T           everything f32: T is the sum of the magnitudes that enter the reductions behind the element (the
                                           condition of the sums, before they cancel -- not max|ref|), written out beside each _xxx below
with K = MARGIN x the largest |f32 restatement - f64| / (2^-24 T) over every case and family of the case lists below.  MARGIN = 4 is the
convention of act_ops_ref.m32_of / attention_ref.M32: it covers what the CPU restatement does not have -- the device's v_exp_f32 / v_rsq_f32 /
erff at 1 .. 2 ulp and the compiler's contraction of a * b + c into one rounding.  K_MEASURED holds the measured figures;
tests/test_norm_bwd_cpu.py::test_constants_are_the_measured_ones re-measures and pins them.  No element is masked or left out.
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import torch

from act_ops_ref import ulp16

Tensor = torch.Tensor
F64, F32, F16 = torch.float64, torch.float32, torch.float16
ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_RELU = 0, 1, 2, 3, 4  # include/genima_hip.h
EPS = 1e-5
U32 = 2.0 ** -24
MARGIN = 4.0
# largest |f32 restatement - f64| / (2^-24 T) per output over all cases x families (CPU, test_constants_are_the_measured_ones); K = MARGIN x this,
# so the restatement's own worst err / bound of the f32 part is 1 / MARGIN = 0.25
K_MEASURED = {
    "ln_dx": 5.88, "ln_dgamma": 2.62, "ln_dbeta": 0.913,   # (8161, 320) chanmark; (3, 1280) rowmark; (3, 1032) gauss
    "gn_dx": 3.56, "gn_dgamma": 2.95, "gn_dbeta": 1.27,    # (2, 64, 1280, 1280, 32) chanmark; (2, 64, 1280, 640, 32) rowmark; (1, 9, 64, 0, 32) rowmark SiLU
    "fwd_mean": 3.21, "fwd_var": 10.1,                     # (1, 4096, 320, 0, 32) lowvar, fused; (2, 64, 72, 0, 8) lowvar, three-launch
    "act": 2.27, "geglu": 2.54, "softmax": 3.12,           # GELU; blk = 32; (33, 4096)
}
K = {n: MARGIN * v for n, v in K_MEASURED.items()}


def eps32(eps: float) -> float:
    """eps as the kernels hold it (a float argument)."""
    return float(torch.tensor(eps, dtype=F32))


def _seq(t: Tensor, dim: int, dt) -> Tensor:
    """Sum along ``dim``: f64 -> the plain sum; f32 -> one accumulator walking the dimension in order, as a thread's loop does."""
    if dt == F64:
        return t.sum(dim)
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def _pad_to(t: Tensor, dim: int, mult: int) -> Tensor:
    """Zero-pad ``dim`` to a multiple of ``mult`` (x + 0 is exact: an idle lane's or a missing row's contribution)."""
    n = t.shape[dim]
    m = (n + mult - 1) // mult * mult
    if m == n:
        return t
    shape = list(t.shape)
    shape[dim] = m - n
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim)


_X1 = torch.arange(64) ^ 1
_X2 = torch.arange(64) ^ 2
_HM = (torch.arange(64) & ~7) | (7 - (torch.arange(64) & 7))    # row_half_mirror
_RM = (torch.arange(64) & ~15) | (15 - (torch.arange(64) & 15))  # row_mirror


def _wave_sum(v: Tensor, dt) -> Tensor:
    """common.h wave_sum over the last dimension (64 lanes): quad xor 1, xor 2, half-row mirror, row mirror, then (r0 + r16) + (r32 + r48)."""
    if dt == F64:
        return v.sum(-1)
    for perm in (_X1, _X2, _HM, _RM):
        v = v + v[..., perm]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------------------
def lnb_rows_per_block(M: int) -> int:
    """backward.hip lnb_rows_per_block."""
    rpb = 64
    while rpb > 8 and (M + rpb - 1) // rpb < 256:
        rpb >>= 1
    return rpb


def lnb_route(M: int, C: int):
    """-> (CH, R, rows per block) of layernorm_bwd_kernel<CH, R> as gn_layernorm_bwd picks them."""
    CC = C // 8
    CH, R = ((1, 4) if CC <= 64 else (2, 2) if CC <= 128 else (3, 1) if CC <= 192 else (4, 1))
    return CH, R, lnb_rows_per_block(M)


def _reduce_rows(part: Tensor, dt) -> Tensor:
    """reduce_rows_f32_kernel over dim 0: wave w of 4 sums rows w, w + 4, .. with four accumulators, then the waves fold."""
    if dt == F64:
        return part.sum(0)
    Rn = part.shape[0]
    waves = []
    for w in range(4):
        s = [torch.zeros_like(part[0]) for _ in range(4)]
        r = w
        while r + 12 < Rn:
            for u in range(4):
                s[u] = s[u] + part[r + 4 * u]
            r += 16
        while r < Rn:
            s[0] = s[0] + part[r]
            r += 4
        waves.append((s[0] + s[1]) + (s[2] + s[3]))
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def _ln_bwd(dt, x: Tensor, gamma: Tensor, dy: Tensor, eps: float = EPS, plant: str = ""):
    """LayerNorm backward in dtype ``dt``: x, dy [M, C], gamma [C] (f16) -> namespace dx [M, C], dgamma, dbeta [C] (no prior contents added).
        mu = mean x, r = (mean (x - mu)^2 + eps)^-1/2, xh = (x - mu) r, gv = dy gamma, m1 = mean gv, m2 = mean gv xh,
        dx = r (gv - m1 - xh m2), dgamma = sum_m dy xh, dbeta = sum_m dy.
    f32: lane l of the wave owns the 8-channel chunks l, l + 64, ..; a row sum is the lane's chain over its <= 32 elements, then wave_sum;
    dgamma / dbeta: each wave's chain over its rows of the block (rows w R + 4 R k + r), then reduce_rows_f32_kernel over blocks x 4 partials.
    ``plant``: one deliberate error (tests/test_norm_bwd_cpu.py).
    Magnitudes (f64, no plant), with Dl = r mean|x| (a rounding error of mu shifts every xh of the row by up to ~ 2^-24 Dl):
        dx_T = r (|gv| + mean|gv| + Dl |m2| + |xh| (mean|gv xh| + Dl |m1|)),   dgamma_T = sum_m |dy| (|xh| + Dl),   dbeta_T = sum_m |dy|."""
    M, C = x.shape
    CH, R, rpb = lnb_route(M, C)
    xs, g, d = x.to(dt), gamma.to(dt), dy.to(dt)
    e = torch.tensor(eps32(eps), dtype=dt)

    def rowsum(t):  # [M, C] -> [M]
        if dt == F64:
            return t.sum(-1)
        lanes = _pad_to(t, 1, 512).reshape(M, -1, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, -1)  # [M, lane, (chunk i, e)]
        return _wave_sum(_seq(lanes, 2, dt), dt)

    invC = (torch.tensor(1.0, dtype=F32) / torch.tensor(float(C), dtype=F32)).to(dt) if dt == F32 else 1.0 / C
    mu = rowsum(xs) * invC
    dlt = xs - mu[:, None]
    r = torch.rsqrt(rowsum(dlt * dlt) * invC + e)
    xh = dlt * r[:, None]
    gv = d * g
    inv1 = (1.0 / (C + 8)) if plant == "m1_over_c_plus_8" else invC
    m1, m2 = rowsum(gv) * inv1, rowsum(gv * xh) * invC
    core = gv - m1[:, None] - xh * m2[:, None]
    if plant == "dx_twice_f16":  # the value passes through f16 twice on its way to the store / the add
        core = core.to(F16).to(dt)
    out = SimpleNamespace(dx=r[:, None] * core)
    if dt == F64:
        dg, db = (d * xh).sum(0), d.sum(0)
    else:
        blocks, trips = (M + rpb - 1) // rpb, (rpb + 4 * R - 1) // (4 * R)
        # row of (block, wave w, trip k, slot r): block rpb + w R + 4 R k + r; rows past the block's end or past M are zeros in the kernel
        k_, r_ = torch.arange(trips), torch.arange(R)
        local = (torch.arange(4)[:, None, None] * R + k_[None, :, None] * 4 * R + r_[None, None, :]).reshape(1, 4, trips * R)
        rows = (torch.arange(blocks)[:, None, None] * rpb + local).reshape(blocks * 4, trips * R)
        live = (rows < M) & (local < rpb).expand(blocks, 4, trips * R).reshape(blocks * 4, trips * R)
        rows = rows.clamp_max(M - 1)
        pg = _seq((d * xh)[rows] * live[..., None], 1, dt)  # [blocks * 4, C]
        pb = _seq(d[rows] * live[..., None], 1, dt)
        dg, db = _reduce_rows(pg, dt), _reduce_rows(pb, dt)
    if plant == "dgamma_scaled":
        dg = dg.clone()
        dg[C - 1] *= 1 + 2.0 ** -9
    out.dgamma, out.dbeta = dg, db
    if dt == F64 and not plant:
        Dl = (r * xs.abs().mean(-1))[:, None]
        agv = gv.abs()
        out.dx_T = r[:, None] * (agv + agv.mean(-1, keepdim=True) + Dl * m2.abs()[:, None]
                                 + xh.abs() * ((agv * xh.abs()).mean(-1, keepdim=True) + Dl * m1.abs()[:, None]))
        out.dgamma_T = (d.abs() * (xh.abs() + Dl)).sum(0)
        out.dbeta_T = d.abs().sum(0)
    return out


def ln_bwd_ref(x, gamma, dy, eps: float = EPS):
    return _ln_bwd(F64, x, gamma, dy, eps)


def ln_bwd_f32(x, gamma, dy, eps: float = EPS, plant: str = ""):
    """The kernel's arithmetic on the CPU; dx before its f16 store in dx32.  No GPU test compares against it."""
    out = _ln_bwd(F32, x, gamma, dy, eps, plant)
    out.dx32, out.dx = out.dx, out.dx.to(F16)
    return out


def ln_bounds(ref, prior: Tensor | None = None) -> dict:
    """{dx, dgamma, dbeta: bound}.  prior [2, C]: what dgamma | dbeta held (the reference adds it; one more f32 addition)."""
    p = prior.to(F64).abs() if prior is not None else torch.zeros(2, ref.dgamma.numel(), dtype=F64)
    return {"dx": 0.5 * ulp16(ref.dx) + K["ln_dx"] * U32 * ref.dx_T,
            "dgamma": K["ln_dgamma"] * U32 * ref.dgamma_T + U32 * (p[0] + ref.dgamma.abs()),
            "dbeta": K["ln_dbeta"] * U32 * ref.dbeta_T + U32 * (p[1] + ref.dbeta.abs())}


# ---- GroupNorm: what the forward saves ----------------------------------------------------------------------------------------------------
def _groups(t: Tensor, G: int) -> Tensor:
    """[B, HW, C] -> [B, G, HW * cpg]"""
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)


def gn_fwd_route(B: int, HW: int, C1: int, C2: int, G: int) -> str:
    """norm.hip gn_launch_groupnorm with save_scsh set and GN_GROUPNORM_FUSED unset: 'fused' (gn_fused_kernel) or 'three' (stats / finalize /
    apply).  GNF_MAX_LDS = 96 KB, GNF_THREADS = 512."""
    C = C1 + C2
    cpg = C // G
    slab = HW * cpg * 2
    small = B * HW * C * 2 <= (4 << 20)
    fused = cpg % 2 == 0 and (cpg >> 1) <= 512 and C1 % 2 == 0 and slab <= 96 * 1024 and (B * G >= 64 or small)
    return "fused" if fused else "three"


def gn_pick_chunks(B: int, HW: int) -> int:
    return max(1, min((1024 + B - 1) // B, (HW + 15) // 16))


def _gn_saved(dt, x: Tensor, gamma: Tensor, beta: Tensor, G: int, eps: float = EPS, route: str = "fused"):
    """What the GroupNorm forward saves, x [B, HW, C] the concatenated input: stats[b][g] = (mean, rstd), scsh[b][c] = (rstd gamma, beta - mean rstd gamma).
    f32, route 'fused' (gn_fused_kernel): thread (pair j, pixel lane p0) chains its pixels p0, p0 + pstep, .. adding (a + b) and (a a + b b),
    wave_sum, the 8 waves in order; var = tss / n - mean mean in f32.  Route 'three': gn_stats_kernel's f32 per-slab sums (a pixel lane's chain,
    then channels x lanes in order), combined in f64 by gn_finalize_kernel.
    Magnitudes: mean_T = mean|x|, var_T = mean x^2 (which bounds mean^2 and |mean| mean|x| as well)."""
    B, HW, C = x.shape
    cpg = C // G
    n = HW * cpg
    xs = x.to(dt)
    e = torch.tensor(eps32(eps), dtype=dt)
    if dt == F64:
        xg = _groups(xs, G)
        mean = xg.mean(-1)
        var = (xg * xg).mean(-1) - mean * mean
        rstd = torch.rsqrt(var + e)
    elif route == "fused":
        hpg = cpg // 2
        pstep = 512 // hpg
        xp = _pad_to(xs, 1, pstep).reshape(B, -1, pstep, G, hpg, 2)  # [B, trip, p0, g, j, 2]
        s = _seq(xp[..., 0] + xp[..., 1], 1, dt)                      # [B, p0, g, j]
        ss = _seq(xp[..., 0] * xp[..., 0] + xp[..., 1] * xp[..., 1], 1, dt)
        # thread id = p0 * hpg + j; threads >= hpg * pstep idle (zeros)
        thr = lambda t: _pad_to(t.permute(0, 2, 1, 3).reshape(B, G, pstep * hpg), 2, 512).reshape(B, G, 8, 64)
        ts, tss = _seq(_wave_sum(thr(s), dt), 2, dt), _seq(_wave_sum(thr(ss), dt), 2, dt)
        nf = torch.tensor(float(HW), dtype=F32) * torch.tensor(float(cpg), dtype=F32)
        mean = ts / nf
        var = (tss / nf - mean * mean).clamp_min(0)
        rstd = torch.rsqrt(var + e)
    else:
        chunks = gn_pick_chunks(B, HW)
        rows = (HW + chunks - 1) // chunks
        chunks = (HW + rows - 1) // rows
        CC = C // 8
        TX = min(CC, 256)
        PY = 256 // TX
        xp = _pad_to(_pad_to(xs, 1, rows).reshape(B, chunks, rows, C), 2, PY).reshape(B, chunks, -1, PY, C)
        ls, lq = _seq(xp, 2, dt), _seq(xp * xp, 2, dt)                                      # [B, chunks, PY, C]
        fold = lambda t: _seq(t.reshape(B, chunks, PY, G, cpg).permute(0, 1, 3, 4, 2).reshape(B, chunks, G, cpg * PY), 3, dt)
        ts, tss = fold(ls).to(F64).sum(1), fold(lq).to(F64).sum(1)
        m64 = ts / n
        mean = m64.to(F32)
        rstd = (1.0 / torch.sqrt((tss / n - m64 * m64).clamp_min(0) + e.to(F64))).to(F32)
        var = (tss / n - m64 * m64).to(F32)
    gm, bt = gamma.to(dt), beta.to(dt)
    a = rstd.repeat_interleave(cpg, 1) * gm
    sh = bt - mean.repeat_interleave(cpg, 1) * a
    out = SimpleNamespace(mean=mean, rstd=rstd, var=var, stats=torch.stack([mean, rstd], -1), scsh=torch.stack([a, sh], -1))
    if dt == F64:
        xg = _groups(xs, G)
        out.mean_T, out.var_T = xg.abs().mean(-1), (xg * xg).mean(-1)
    return out


def gn_saved_ref(x1, x2, gamma, beta, G: int, eps: float = EPS):
    x = torch.cat([x1, x2], -1) if x2 is not None else x1
    return _gn_saved(F64, x, gamma, beta, G, eps)


def gn_saved_f32(x1, x2, gamma, beta, G: int, eps: float = EPS, route: str = "fused"):
    x = torch.cat([x1, x2], -1) if x2 is not None else x1
    return _gn_saved(F32, x, gamma, beta, G, eps, route)


def gn_saved_bounds(ref, gamma: Tensor, beta: Tensor, eps: float = EPS) -> dict:
    """{stats [B, G, 2], scsh [B, C, 2]: bound}, f32 outputs.  mean: its sum and one rounding.  rstd: the worst the f32 error dv = K 2^-24 mean x^2
    of var can do, evaluated (not linearised: at a spread of a few f16 ulps dv is a few per cent of var + eps), plus the rsqrt and the store.
    scale = rstd gamma and shift = beta - mean scale inherit them through one product / one product and one difference.
    The small integers count roundings of 2^-24 each: 4 for rstd = var + eps, the reciprocal square root at up to 2 ulp (v_rsq_f32; sqrt and a
    division in f64 on the three-launch path) and the store; 1 for the product rstd gamma; 2 for mean scale and the difference.  dv is capped
    at 3/4 of var + eps so that the worst case stays finite -- no case here comes near (the largest is 0.20 of it, lowvar)."""
    cpg = gamma.numel() // ref.mean.shape[1]
    b_mean = K["fwd_mean"] * U32 * ref.mean_T + U32 * ref.mean.abs()
    v = ref.var + eps32(eps)
    dv = torch.minimum(K["fwd_var"] * U32 * ref.var_T, 0.75 * v)
    b_rstd = (torch.rsqrt(v - dv) - ref.rstd) + 4 * U32 * ref.rstd
    g = gamma.to(F64).abs()
    a, sh = ref.scsh[..., 0].abs(), ref.scsh[..., 1].abs()
    b_a = b_rstd.repeat_interleave(cpg, 1) * g + U32 * a
    mu = ref.mean.abs().repeat_interleave(cpg, 1)
    b_sh = mu * b_a + a * b_mean.repeat_interleave(cpg, 1) + 2 * U32 * (mu * a + beta.to(F64).abs())
    return {"stats": torch.stack([b_mean, b_rstd], -1), "scsh": torch.stack([b_a, b_sh], -1)}


# ---- GroupNorm(+SiLU) backward ---------------------------------------------------------------------------------------------------------------
def gnb_slabs(HW: int):
    """gn_groupnorm_bwd's slab arithmetic -> (chunks used for the workspace offsets, rows per slab, slabs launched)."""
    chunks = max(1, min(64, HW // 16))
    rows = (HW + chunks - 1) // chunks
    return chunks, rows, (HW + rows - 1) // rows


def _silu_grad(z: Tensor) -> Tensor:
    s = 1.0 / (1.0 + torch.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def _gn_bwd(dt, x1, x2, gamma, dy, stats: Tensor, scsh: Tensor, G: int, act: int, plant: str = ""):
    """GroupNorm(+SiLU) backward over the NHWC concat x = x1 | x2 [B, HW, C], from the stats [B, G, 2] and scsh [B, C, 2] THE KERNEL IS GIVEN:
        dyh = dy silu'(x a + s) (a, s = scsh) or dy;  S1 = sum_hw dyh, S2 = sum_hw dyh x  per (b, c);
        per (b, g), n = HW cpg:  c1 = sum_c gamma (S2 - mu S1) r / n,  c2 = sum_c gamma S1 / n  (mu, r = stats);
        dx = (r gamma) dyh + (-r^2 c1) x + (r^2 c1 mu - r c2);   dgamma = sum_b (S2 - mu S1) r,  dbeta = sum_b S1.
    -> namespace dx [B, HW, C] (dx1 | dx2), dgamma, dbeta [C] (no prior contents added).
    f32: gnb_partial_kernel (row lane ty of TY chains rows ty, ty + TY, .. of its slab, the lanes fold in order), gnb_finalize_kernel (chunk lane
    cl of L = 256 / cpg chains slabs cl, cl + L, .., the lanes fold in order; thread 0 chains the group's channels), gnb_param_kernel (b in
    order), gnb_apply_kernel (k0 d + k1 x + k2).
    Magnitudes (f64, no plant), D = |dy| (1.1 + (|x a| + |s|) / 2) for SiLU (|silu'| <= 1.1, |silu''| <= 1/2: the rounding of x a + s reaches dyh
    through it) and |dy| otherwise:  A1 = sum_hw D, A2 = sum_hw D |x|, U1 = sum_c |gamma| r (A2 + |mu| A1), U2 = sum_c |gamma| A1,
        dx_T = r |gamma| D + r^2 (U1 / n) (|x| + |mu|) + r U2 / n,   dgamma_T = sum_b r (A2 + |mu| A1),   dbeta_T = sum_b A1."""
    x = (torch.cat([x1, x2], -1) if x2 is not None else x1).to(dt)
    B, HW, C = x.shape
    cpg = C // G
    n = float(HW * cpg)
    d, gm = dy.to(dt), gamma.to(dt)
    a, s = scsh[..., 0].to(dt)[:, None, :], scsh[..., 1].to(dt)[:, None, :]
    mu, r = stats[..., 0].to(dt), stats[..., 1].to(dt)
    dyh = d * _silu_grad(x * a + s) if act == ACT_SILU else d
    chunks, rows, nslab = gnb_slabs(HW)
    if dt == F64:
        dd = dyh
        if plant == "slab_last_row":  # the last row of slab 0 never reaches S1 / S2
            dd = dyh.clone()
            dd[:, min(HW, rows) - 1] = 0
        S1, S2 = dd.sum(1), (dd * x).sum(1)
    else:
        CC = C // 8
        TX = min(CC, 256)
        TY = 256 // TX

        def slabsum(t):  # [B, HW, C] -> [B, C]
            if plant == "slab_last_row":
                t = t.clone()
                t[:, min(HW, rows) - 1] = 0
            tp = _pad_to(_pad_to(t, 1, rows).reshape(B, nslab, rows, C), 2, TY).reshape(B, nslab, -1, TY, C)
            part = _seq(_seq(tp, 2, dt), 2, dt)  # rows of a lane, then the lanes -> [B, nslab, C]
            L = 256 // cpg
            pl = _pad_to(part, 1, L).reshape(B, -1, L, C)
            return _seq(_seq(pl, 1, dt), 1, dt)
        S1, S2 = slabsum(dyh), slabsum(dyh * x)
    mu_c, r_c = mu.repeat_interleave(cpg, 1), r.repeat_interleave(cpg, 1)
    w1, w2 = gm * (S2 - mu_c * S1) * r_c, gm * S1
    if plant == "group_last_channel":  # the sums over the group's channels stop one short
        w1, w2 = w1.clone(), w2.clone()
        w1[:, cpg - 1::cpg], w2[:, cpg - 1::cpg] = 0, 0
    t1, t2 = _seq(w1.reshape(B, G, cpg), 2, dt), _seq(w2.reshape(B, G, cpg), 2, dt)
    nn = torch.tensor(float(HW), dtype=F32) * torch.tensor(float(cpg), dtype=F32) if dt == F32 else n
    c1, c2 = (t1 / nn).repeat_interleave(cpg, 1), (t2 / nn).repeat_interleave(cpg, 1)
    k0, k1, k2 = r_c * gm, -r_c * r_c * c1, r_c * r_c * c1 * mu_c - r_c * c2
    out = SimpleNamespace(dx=k0[:, None] * dyh + k1[:, None] * x + k2[:, None])
    dg, db = _seq((S2 - mu_c * S1) * r_c, 0, dt), _seq(S1, 0, dt)
    if plant == "dgamma_scaled":  # the last channel of the middle group
        dg = dg.clone()
        dg[C // 2 + cpg - 1] *= 1 + 2.0 ** -9
    out.dgamma, out.dbeta = dg, db
    if dt == F64 and not plant:
        ax = x.abs()
        D = d.abs() * (1.1 + 0.5 * ((x * a).abs() + s.abs())) if act == ACT_SILU else d.abs()
        A1, A2 = D.sum(1), (D * ax).sum(1)
        amu = mu_c.abs()
        U1 = (gm.abs() * r_c * (A2 + amu * A1)).reshape(B, G, cpg).sum(-1).repeat_interleave(cpg, 1)
        U2 = (gm.abs() * A1).reshape(B, G, cpg).sum(-1).repeat_interleave(cpg, 1)
        out.dx_T = (r_c * gm.abs())[:, None] * D + (r_c * r_c * U1 / n)[:, None] * (ax + amu[:, None]) + (r_c * U2 / n)[:, None]
        out.dgamma_T = (r_c * (A2 + amu * A1)).sum(0)
        out.dbeta_T = A1.sum(0)
    return out


def gn_bwd_ref(x1, x2, gamma, dy, stats, scsh, G: int, act: int):
    return _gn_bwd(F64, x1, x2, gamma, dy, stats, scsh, G, act)


def gn_bwd_f32(x1, x2, gamma, dy, stats, scsh, G: int, act: int, plant: str = ""):
    out = _gn_bwd(F32, x1, x2, gamma, dy, stats, scsh, G, act, plant)
    out.dx32, out.dx = out.dx, out.dx.to(F16)
    return out


def gn_bounds(ref, prior: Tensor | None = None) -> dict:
    p = prior.to(F64).abs() if prior is not None else torch.zeros(2, ref.dgamma.numel(), dtype=F64)
    return {"dx": 0.5 * ulp16(ref.dx) + K["gn_dx"] * U32 * ref.dx_T,
            "dgamma": K["gn_dgamma"] * U32 * ref.dgamma_T + U32 * (p[0] + ref.dgamma.abs()),
            "dbeta": K["gn_dbeta"] * U32 * ref.dbeta_T + U32 * (p[1] + ref.dbeta.abs())}


# ---- pointwise -----------------------------------------------------------------------------------------------------------------------------
def _gelu_parts(dt, z: Tensor):
    """-> (Phi(z) = (1 + erf(z / sqrt 2)) / 2, z phi(z), their magnitudes before the cancellation of 1 + erf)."""
    er = torch.erf(z * torch.tensor(0.70710678118654752, dtype=dt))
    zphi = z * torch.tensor(0.3989422804014327, dtype=dt) * torch.exp(-0.5 * z * z)
    return 0.5 * (1.0 + er), zphi, 0.5 * (1.0 + er.abs()), zphi.abs() * (1.0 + 0.5 * z * z)


def act_bwd_terms(dt, dy: Tensor, z: Tensor, act: int):
    """dz = dy act'(z) (backward.hip act_grad) -> (value, T).  T: SiLU / QuickGELU s (1 + k z (1 - s)), s = 1 / (1 + e^-kz): the fast exponential
    is relative (1 + |kz|) 2^-24, 1 - s cancels for large kz -> |dy| s (1 + |kz|) (1 + (1 - s)(1 + |kz|)); GELU: |dy| ((1 + |erf|) / 2 +
    |z| phi (1 + z^2 / 2)); ReLU and the identity are exact (T = 0: the bits of dy, or zero)."""
    d, zz = dy.to(dt), z.to(dt)
    if act in (ACT_SILU, ACT_QUICK_GELU):
        k = 1.0 if act == ACT_SILU else float(torch.tensor(1.702, dtype=F32))
        kz = zz * torch.tensor(k, dtype=dt)
        s = 1.0 / (1.0 + torch.exp(-kz))
        return d * (s * (1.0 + kz * (1.0 - s))), d.abs() * s * (1 + kz.abs()) * (1 + (1 - s) * (1 + kz.abs()))
    if act == ACT_GELU:
        Phi, zphi, aPhi, azphi = _gelu_parts(dt, zz)
        return d * (Phi + zphi), d.abs() * (aPhi + azphi)
    if act == ACT_RELU:
        return d * (zz > 0).to(dt), torch.zeros_like(d)
    return d.clone(), torch.zeros_like(d)


def geglu_split(hg: Tensor, blk: int):
    """[M, 2 Hd] -> (hidden, gate) [M, Hd]: blk == 0 halves, blk > 0 alternating blk-column blocks."""
    M, H2 = hg.shape
    if blk == 0:
        return hg[:, :H2 // 2], hg[:, H2 // 2:]
    v = hg.reshape(M, -1, 2, blk)
    return v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1)


def geglu_join(dh: Tensor, dg: Tensor, blk: int) -> Tensor:
    M, Hd = dh.shape
    if blk == 0:
        return torch.cat([dh, dg], -1)
    return torch.stack([dh.reshape(M, -1, blk), dg.reshape(M, -1, blk)], 2).reshape(M, 2 * Hd)


def geglu_bwd_terms(dt, dy: Tensor, hg: Tensor, blk: int):
    """out = hidden gelu(gate): d hidden = dy gelu(gate), d gate = dy hidden gelu'(gate), in hg's layout -> (value, T) [M, 2 Hd]."""
    h, g = (t.to(dt) for t in geglu_split(hg, blk))
    d = dy.to(dt)
    Phi, zphi, aPhi, azphi = _gelu_parts(dt, g)
    return (geglu_join(d * (g * Phi), d * h * (Phi + zphi), blk),
            geglu_join(d.abs() * g.abs() * aPhi, d.abs() * h.abs() * (aPhi + azphi), blk))


def softmax_bwd_terms(dt, p: Tensor, dp: Tensor, scale: float):
    """ds = scale p (dp - sum_j p dp) over rows [rows, cols] -> (value, T = |scale| p (|dp| + sum_j |p dp|)).  f32: lane l chains its chunks
    l, l + 64, .. (8 products each), then wave_sum."""
    pp, dd = p.to(dt), dp.to(dt)
    rows, cols = pp.shape
    prod = pp * dd
    if dt == F64:
        dot = prod.sum(-1)
    else:
        lanes = _pad_to(prod, 1, 512).reshape(rows, -1, 64, 8).permute(0, 2, 1, 3).reshape(rows, 64, -1)
        dot = _wave_sum(_seq(lanes, 2, dt), dt)
    sc = torch.tensor(scale, dtype=F32).to(dt)
    return sc * pp * (dd - dot[:, None]), sc.abs() * pp.abs() * (dd.abs() + prod.abs().sum(-1, keepdim=True))


def pointwise_bound(ref: Tensor, T: Tensor, name: str) -> Tensor:
    return 0.5 * ulp16(ref) + K[name] * U32 * T


# ---- comparing -----------------------------------------------------------------------------------------------------------------------------
def assert_within(got: Tensor, ref: Tensor, bound: Tensor, what: str = "", quiet: bool = False) -> float:
    """Every element: |got - ref| <= bound (where the bound is zero: equality).  Prints and returns the largest err / bound."""
    got, ref = got.detach().cpu().to(F64), ref.detach().to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max())
    if not quiet:
        print(f"{what}: max err/bound {ratio:.3f}, max |err| {float(err.max()):.3e}")
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), (f"{what}: |got - ref| {float(err.flatten()[worst]):.6e} > bound {float(bound.flatten()[worst]):.6e} at flat index "
                                        f"{worst} of {tuple(got.shape)} (got {float(got.flatten()[worst])!r}, ref {float(ref.flatten()[worst])!r}); "
                                        f"{int((err > bound).sum())} elements out")
    return ratio


def breaks(got: Tensor, ref: Tensor, bound: Tensor) -> bool:
    """Some element is outside its bound (the planted-error tests)."""
    return bool(((got.detach().to(F64) - ref).abs() > bound).any())


# ---- cases and input families ------------------------------------------------------------------------------------------------------------------
FAMILIES = ["gauss", "offset", "lowvar", "rowmark", "chanmark", "dyzero"]
LN_C = [8, 320, 512, 520, 640, 1024, 1032, 1280, 1536, 1544, 2048]
LN_CASES = [(M, C) for C in LN_C for M in (1, 3, 7, 300)] + [(M, 320) for M in (4081, 8161, 16321)]
# (B, HW, C1, C2, G): what each reaches
GN_CASES = [
    (2, 144, 64, 0, 32),      # baseline
    (2, 64, 320, 0, 32),      # cpg = 10: L = 25, 6 idle threads in gnb_finalize_kernel; TY = 6 with 16 idle threads in gnb_partial_kernel
    (3, 64, 640, 0, 32),      # B > 2 in gnb_param_kernel; cpg = 20
    (2, 64, 640, 320, 32),    # cpg = 30: group 21 straddles x | x2
    (2, 64, 1280, 640, 32),   # cpg = 60
    (2, 64, 1280, 1280, 32),  # C = 2560: two cb passes; cpg = 80
    (1, 9, 64, 0, 32),        # HW < 16: one slab
    (2, 100, 320, 0, 32),     # slabs of 17 rows, the last one 15
    (1, 1000, 64, 0, 32),     # 59 slabs launched, 62 in the workspace offsets
    (1, 1024, 320, 0, 32),    # 64 slabs of 16 rows
    (1, 4096, 320, 0, 32),    # 64-row slabs: the four-rows-in-flight loop and its remainder at TY = 6
    (1, 6400, 64, 0, 32),     # 100-row slabs: the same at TY = 32 (remainder only: 100 <= 3 * 32 + ty for ty >= 4)
    (1, 64, 256, 0, 1),       # cpg = 256, L = 1
    (2, 64, 64, 0, 8),        # cpg = 8, L = 32
]
# the forward's saved statistics: every case above takes gn_fused_kernel (gn_fwd_route); these take the three-launch path -- a slab of
# HW cpg 2 = 128 KB > GNF_MAX_LDS, and an odd cpg = 9
FWD_THREE = [(1, 4096, 512, 0, 32), (2, 64, 72, 0, 8)]
FWD_CASES = GN_CASES + FWD_THREE
FWD_FAMILIES = ["gauss", "offset", "lowvar"]
SOFTMAX_CASES = [(rows, cols) for cols in (8, 256, 520, 4096) for rows in (1, 33)]


def ln_id(case) -> str:
    return f"M{case[0]}-C{case[1]}"


def gn_id(case) -> str:
    return "x".join(str(i) for i in case)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _x_family(shape, family: str, g) -> Tensor:
    if family == "offset":   # mean >> spread: S2 - mu S1 and mean x^2 - mean^2 cancel
        return 8 + 0.25 * torch.randn(shape, generator=g)
    if family == "lowvar":   # a few f16 ulps (2^-10) around 1: rstd ~ 250
        return 1 + torch.randint(-3, 4, shape, generator=g).to(torch.float32) * 2.0 ** -10
    return torch.randn(shape, generator=g)


def ln_inputs(case, family: str = "gauss", seed: int = 0):
    """-> f16 CPU x [M, C], gamma [C], dy [M, C].  rowmark: dy lives in the last row of every block of lnb_rows_per_block(M) rows (the row a
    short last trip or a short last block would drop); chanmark: in channel C - 1 alone."""
    M, C = case
    assert family in FAMILIES, family
    g = _gen(M, C, FAMILIES.index(family), seed)
    x = _x_family((M, C), family, g)
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g)
    if family == "rowmark":
        rpb = lnb_rows_per_block(M)
        keep = torch.zeros(M, dtype=torch.bool)
        keep[torch.arange(rpb - 1, M + rpb - 1, rpb).clamp_max(M - 1)] = True
        dy = dy * keep[:, None]
    elif family == "chanmark":
        dy[:, :C - 1] = 0
    elif family == "dyzero":
        dy.zero_()
    return x.to(F16), gamma.to(F16), dy.to(F16)


def gn_inputs(case, family: str = "gauss", seed: int = 0):
    """-> f16 CPU x1 [B, HW, C1], x2 [B, HW, C2] or None, gamma, beta [C], dy [B, HW, C].  rowmark: dy lives in the last pixel of every slab of
    gnb_slabs(HW); chanmark: in each group's last channel."""
    B, HW, C1, C2, G = case
    C = C1 + C2
    assert family in FAMILIES, family
    g = _gen(B, HW, C1, C2, G, FAMILIES.index(family), seed)
    x = _x_family((B, HW, C), family, g)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(B, HW, C, generator=g)
    if family == "rowmark":
        _, rows, _ = gnb_slabs(HW)
        keep = torch.zeros(HW, dtype=torch.bool)
        keep[torch.arange(rows - 1, HW + rows - 1, rows).clamp_max(HW - 1)] = True
        dy = dy * keep[None, :, None]
    elif family == "chanmark":
        dy = dy * (torch.arange(C) % (C // G) == C // G - 1)
    elif family == "dyzero":
        dy.zero_()
    x = x.to(F16)
    return x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None), gamma.to(F16), beta.to(F16), dy.to(F16)


_FIX: "OrderedDict" = OrderedDict()
_FIX_CAP = 1 << 28  # bytes of tensors kept; the oldest fixtures go first (one family of M = 16321 x 320 is 0.1 GB)


def _nbytes(v) -> int:
    if isinstance(v, Tensor):
        return v.numel() * v.element_size()
    if isinstance(v, SimpleNamespace):
        v = tuple(vars(v).values())
    return sum(_nbytes(i) for i in v) if isinstance(v, (tuple, list)) else 0


def _cached(key, make):
    """make() once per key while it fits: the fixtures are shared between the tests of a module, and are to be left unchanged."""
    if key in _FIX:
        _FIX.move_to_end(key)
        return _FIX[key]
    val = _FIX[key] = make()
    total = sum(_nbytes(v) for v in _FIX.values())
    while total > _FIX_CAP and len(_FIX) > 1:
        total -= _nbytes(_FIX.popitem(last=False)[1])
    return val


def _worst(v32: Tensor, v64: Tensor, T: Tensor) -> float:
    """Largest |v32 - v64| / (2^-24 T) over the elements with T > 0."""
    rel = (v32.to(F64) - v64).abs() / (U32 * T.clamp_min(1e-300))
    return float(rel[T > 0].max()) if bool((T > 0).any()) else 0.0


def _k_of(r32, ref, prefix: str) -> dict:
    return {prefix + n: _worst(getattr(r32, "dx32" if n == "dx" else n), getattr(ref, n), getattr(ref, n + "_T")) for n in ("dx", "dgamma", "dbeta")}


def ln_fixture(case, family: str):
    """(x, gamma, dy, ref) of a case, computed once and shared: leave it unchanged."""
    def make():
        x, gamma, dy = ln_inputs(case, family)
        return x, gamma, dy, ln_bwd_ref(x, gamma, dy)
    return _cached(("ln", case, family), make)


def _saved_fixture(case, family: str):
    def make():
        x1, x2, gamma, beta, _ = gn_inputs(case, family)
        return gn_saved_ref(x1, x2, gamma, beta, case[4])
    return _cached(("gnsaved", case, family), make)


def gn_fixture(case, family: str, act: int):
    """(x1, x2, gamma, beta, dy, stats32, scsh32, saved, ref): stats32 / scsh32 are the f64 forward's saved values rounded to f32 -- what the
    backward kernel is handed in the tests of the backward alone -- and ref is gn_bwd_ref on exactly those.  Shared: leave it unchanged."""
    def make():
        x1, x2, gamma, beta, dy = gn_inputs(case, family)
        sv = _saved_fixture(case, family)
        st, sc = sv.stats.to(F32), sv.scsh.to(F32)
        return x1, x2, gamma, beta, dy, st, sc, sv, gn_bwd_ref(x1, x2, gamma, dy, st, sc, case[4], act)
    return _cached(("gn", case, family, act), make)


def ln_restated(case, family: str):
    """ln_bwd_f32 of a case's fixture, with .k = {output: its largest |f32 - f64| / (2^-24 T)} (before the f16 store)."""
    def make():
        x, gamma, dy, ref = ln_fixture(case, family)
        r32 = ln_bwd_f32(x, gamma, dy)
        r32.k = _k_of(r32, ref, "ln_")
        return r32
    return _cached(("ln32", case, family), make)


def gn_restated(case, family: str, act: int):
    """gn_bwd_f32 of a case's fixture, with .k as ln_restated."""
    def make():
        x1, x2, gamma, beta, dy, st, sc, sv, ref = gn_fixture(case, family, act)
        r32 = gn_bwd_f32(x1, x2, gamma, dy, st, sc, case[4], act)
        r32.k = _k_of(r32, ref, "gn_")
        return r32
    return _cached(("gn32", case, family, act), make)


def fwd_fixture(case, family: str):
    """(x1, x2, gamma, beta, saved reference) of a forward case, shared: leave it unchanged."""
    def make():
        x1, x2, gamma, beta, _ = gn_inputs(case, family)
        return x1, x2, gamma, beta, _saved_fixture(case, family)
    return _cached(("fwd", case, family), make)


def act_inputs(seed: int = 0):
    """dy, z [n] f16, n % 8 == 0: Gaussian z x 3, a sweep of |z| up to 30, and +-0."""
    g = _gen(11, seed)
    z = torch.cat([3 * torch.randn(2048, generator=g), torch.linspace(-30, 30, 1016), torch.tensor([0.0, -0.0, 30.0, -30.0, 0.0, -0.0, 1e-4, -1e-4])])
    return torch.randn(z.numel(), generator=g).to(F16), z.to(F16)


def geglu_inputs(M: int = 37, Hd: int = 64, seed: int = 0):
    g = _gen(13, M, Hd, seed)
    hg = 2 * torch.randn(M, 2 * Hd, generator=g)
    hg[0, :16] = torch.linspace(-12, 12, 16)
    hg[1, -16:] = torch.linspace(-12, 12, 16)
    return torch.randn(M, Hd, generator=g).to(F16), hg.to(F16)


def softmax_inputs(case, seed: int = 0):
    """p (softmax rows of scores x 3, f16), dp [rows, cols]."""
    rows, cols = case
    g = _gen(17, rows, cols, seed)
    return torch.softmax(3 * torch.randn(rows, cols, generator=g), -1).to(F16), torch.randn(rows, cols, generator=g).to(F16)


def measure_constants(verbose: bool = False) -> dict:
    """The K_MEASURED figures, re-measured: the largest |f32 restatement (before its f16 store) - f64| / (2^-24 T) over every case x family.
    Self-contained: whatever it needs it computes (or finds in the fixture cache)."""
    worst, where = {n: 0.0 for n in K_MEASURED}, {}

    def upd(name, v, tag):
        if v > worst[name]:
            worst[name], where[name] = v, tag

    for case in LN_CASES:
        for fam in FAMILIES:
            for n, v in ln_restated(case, fam).k.items():
                upd(n, v, (case, fam))
    for case in GN_CASES:
        for fam in FAMILIES:
            for act in (ACT_NONE, ACT_SILU):
                for n, v in gn_restated(case, fam, act).k.items():
                    upd(n, v, (case, fam, act))
    for case in FWD_CASES:  # the restatement of the route the launcher picks for the case
        for fam in FWD_FAMILIES:
            x1, x2, gamma, beta, sv = fwd_fixture(case, fam)
            s32 = gn_saved_f32(x1, x2, gamma, beta, case[4], route=gn_fwd_route(*case))
            upd("fwd_mean", _worst(s32.mean, sv.mean, sv.mean_T), (case, fam))
            upd("fwd_var", _worst(s32.var, sv.var, sv.var_T), (case, fam))
    dy, z = act_inputs()
    for act in (ACT_SILU, ACT_GELU, ACT_QUICK_GELU):
        (v64, T), (v32, _) = act_bwd_terms(F64, dy, z, act), act_bwd_terms(F32, dy, z, act)
        upd("act", _worst(v32, v64, T), act)
    for blk in (0, 32):
        d, hg = geglu_inputs()
        (v64, T), (v32, _) = geglu_bwd_terms(F64, d, hg, blk), geglu_bwd_terms(F32, d, hg, blk)
        upd("geglu", _worst(v32, v64, T), blk)
    for case in SOFTMAX_CASES:
        p, dp = softmax_inputs(case)
        (v64, T), (v32, _) = softmax_bwd_terms(F64, p, dp, 0.125), softmax_bwd_terms(F32, p, dp, 0.125)
        upd("softmax", _worst(v32, v64, T), case)
    if verbose:
        for n, tag in where.items():
            print(n, "worst at", tag)
    return worst


if __name__ == "__main__":
    for n, v in measure_constants(verbose=True).items():
        print(f'    "{n}": {v:.4g},')
