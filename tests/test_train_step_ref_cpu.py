"""-m "not gpu": the references of tests/train_step_ref.py against independent f64 sources (torch.optim.AdamW, clip_grad_norm_, F.mse_loss and
F.conv2d autograd, F.gelu, numpy's f16 cast), the m32_of figure behind every M32_* constant of tests/test_train_step_ops_gpu.py, and the
conditions that module's inputs are chosen to meet."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_train_step_ops_gpu as G
import train_step_ref as R
from act_ops_ref import bits_equal, m32_of

F16, F32, F64 = torch.float16, torch.float32, torch.float64


def close64(a, b, rel=1e-12, what=""):
    a, b = a.to(F64), b.to(F64)
    err = float((a - b).abs().max())
    assert err <= rel * max(float(b.abs().max()), 1e-300), (what, err)


# ---- the references against independent f64 sources ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", R.MSE_LAYOUTS)
def test_mse_terms_against_autograd(layout):
    Cc = layout[0]
    pred, target = R.mse_inputs(1024, layout)
    x = pred[:, :Cc].to(F64).clone().requires_grad_(True)
    loss = F.mse_loss(x, target[:, :Cc].to(F64))
    for gs in R.MSE_GRAD_SCALES:
        (g,) = torch.autograd.grad(loss * gs, x, retain_graph=True)
        (l64, lt), (d64, dt_) = R.mse_terms(F64, pred, target, Cc, gs)
        close64(l64, loss.detach().reshape(1), what="loss")
        close64(d64[:, :Cc], g, what="dpred")
        assert bits_equal(d64[:, Cc:].to(F16), torch.zeros(pred.shape[0], pred.shape[1] - Cc, dtype=F16)), "pad channels: +0"
        assert float(lt) == float(l64) and bool((dt_ == d64.abs()).all())


def test_sumsq_and_clip_against_clip_grad_norm():
    x = R.sumsq_inputs(5003)
    s64, _ = R.sumsq_terms(F64, x)
    w = (x.to(F64) / R.LOSS_SCALE).clone().requires_grad_(True)
    for max_norm in (1.0, 1000.0):  # clipped / not clipped
        w.grad = w.detach().clone()
        norm = torch.nn.utils.clip_grad_norm_([w], max_norm)
        # s64 is the f64 sum of squares of f32 values; handed over as a Python float it would be rounded to f32 -- compare on that value
        coef, nrm, flag = R.clip_terms(F64, float(s64), max_norm, 1.0 / R.LOSS_SCALE)
        assert flag == 0.0 and abs(nrm - float(norm)) <= 1e-7 * float(norm)
        got = float((w.grad / w.detach()).mean())
        assert abs(coef - got) <= 1e-6 * got and (coef == 1.0) == (max_norm == 1000.0)


@pytest.mark.parametrize("wd", R.ADAMW_WDS)
@pytest.mark.parametrize("step", R.ADAMW_STEPS)
def test_adamw_terms_against_torch_adamw(step, wd):
    """One f64 torch.optim.AdamW step from a random (m, v >= 0) state at ``step`` (its hyper-parameters the f32 values the kernel receives)."""
    H = R.ADAMW_HYPER
    p, g, m, v = R.adamw_inputs(5000, 1.0)
    w = p.to(F64).clone().requires_grad_(True)
    opt = torch.optim.AdamW([w], lr=R.f32v(H["lr"]), betas=(R.f32v(H["beta1"]), R.f32v(H["beta2"])), eps=R.f32v(H["eps"]), weight_decay=R.f32v(wd))
    w.grad = g.to(F64).clone()
    opt.state[w] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(F64).clone(), exp_avg_sq=v.to(F64).clone())
    opt.step()
    (m64, _), (v64, _), (u64, _), (p64, _) = R.adamw_terms(F64, p, g, m, v, **H, wd=wd, step=step)
    st = opt.state[w]
    assert int(st["step"]) == step
    close64(m64, st["exp_avg"], what="m")
    close64(v64, st["exp_avg_sq"], what="v")
    close64(u64, w.detach() - p.to(F64), rel=1e-9, what="update")  # the right side went through p's f64 rounding
    close64(p64, w.detach(), what="p")
    assert float(u64[0]) == -(float(p[0]) * (R.f32v(H["lr"]) * R.f32v(wd))) and bool(torch.isfinite(u64).all())  # g = m = v = 0: the decay alone
    # clip and grad_scale enter as one factor on the gradient
    (m2, _), _, _, _ = R.adamw_terms(F64, p, g * 4, m, v, **H, wd=wd, step=step, clip0=0.5, grad_scale=0.5)
    close64(m2, m64)


def test_bias_correction_f32_power_against_f64():
    """What the fix is about: 1 - powf(beta2, step) formed in f32 against the f64 value, steps 1 .. 10 (largest at step 2)."""
    worst = {}
    for step in range(1, 11):
        b64 = R.adamw_bias_corrections(0.9, 0.999, step)
        for b, ref in zip((0.9, 0.999), b64):
            f32 = float(np.float32(1.0) - np.power(np.float32(b), np.float32(step)))
            worst[step] = max(worst.get(step, 0.0), abs(f32 - ref) / ref)
            assert abs(float(np.float32(ref)) - ref) <= 2.0 ** -24 * ref  # rounded once
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) > 2e-6  # an f32 power is this far off: more than 30 f32 roundings


def test_ema_f32_against_f64():
    g = R._gen(8)
    s, q = torch.randn(1028, generator=g), torch.randn(1028, generator=g)
    for omd in R.EMA_OMDS:
        ref = s.to(F64) - R.f32v(omd) * (s.to(F64) - q.to(F64))
        assert float((R.ema_f32(s, q, omd).to(F64) - ref).abs().max()) <= 3 * 2.0 ** -24 * float(ref.abs().max() + (s - q).abs().max())
    assert bits_equal(R.ema_f32(s, q, 1.0), s - (s - q))


@pytest.mark.parametrize("case", R.IM2COL_CASES)
def test_im2col_t_against_conv2d_autograd(case):
    """dW of a convolution IS dY^T im2col^T: the reference image against F.conv2d's weight gradient (f64)."""
    B, H, W, Cc, k, stride, pad = case
    Ho, Wo = R.conv_out_hw(H, W, k, stride, pad)
    assert (B * Ho * Wo) % 8 == 0 and Cc % 8 == 0
    x = R.map_inputs(B, H, W, Cc)
    cols = R.im2col_t_ref(x, k, stride, pad)
    assert cols.shape == (k * k * Cc, B * Ho * Wo) and cols.dtype == F16
    N = 5
    w = torch.zeros(N, Cc, k, k, dtype=F64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2).to(F64), w, None, stride, pad)
    dy = torch.randn(y.shape, generator=R._gen(9), dtype=F64)
    y.backward(dy)
    dyt = dy.permute(1, 0, 2, 3).reshape(N, -1)  # [N, m]
    dw = (dyt @ cols.to(F64).t()).view(N, k * k, Cc).permute(0, 2, 1).reshape(N, Cc, k, k)
    close64(dw, w.grad, rel=1e-12, what="wgrad through im2col^T")
    if pad:
        assert int((cols == 0).sum()) > 0


@pytest.mark.parametrize("case", R.POOL_CASES)
def test_zero_upsample_and_sumpool_against_conv2d_autograd(case):
    """Zero insertion is the data gradient of a stride-2 subsampling; the 2x2 sum is the data gradient of a nearest 2x upsampling."""
    B, H, W, Cc = case
    x = R.map_inputs(B, H, W, Cc)
    up = R.zero_upsample_ref(x)
    big = torch.zeros(B, Cc, 2 * H, 2 * W, dtype=F64, requires_grad=True)
    big[:, :, 0::2, 0::2].backward(x.permute(0, 3, 1, 2).to(F64))
    assert torch.equal(up.to(F64), big.grad.permute(0, 2, 3, 1))
    xb = R.pool_inputs(case, False)
    small = torch.zeros(B, Cc, H, W, dtype=F64, requires_grad=True)
    F.interpolate(small, scale_factor=2, mode="nearest").backward(xb.permute(0, 3, 1, 2).to(F64))
    s64, t64 = R.sumpool_terms(F64, xb)
    close64(s64, small.grad.permute(0, 2, 3, 1), what="sumpool")
    assert bits_equal(R.sumpool_terms(F64, up)[0].to(F16), x)  # sumpool(zero_upsample(x)) == x
    xc = R.pool_inputs(case, True)
    sc, tc = R.sumpool_terms(F64, xc)
    assert float((sc.abs() / tc)[..., 0::2].max()) < 2e-3, "the even channels' blocks cancel"


@pytest.mark.parametrize("case", R.GEGLU_CASES)
def test_geglu_fwd_terms_against_gelu(case):
    M, Hd, blk = case
    hg = R.geglu_inputs(case)
    assert hg.shape == (M, 2 * Hd)
    hid, gate = R.geglu_split(hg, blk)
    ref, Tm = R.geglu_fwd_terms(F64, hg, blk)
    want = hid.to(F64) * F.gelu(gate.to(F64))
    assert float((ref - want).abs().max()) <= 1e-15 * float(Tm.max())
    assert bool((ref.abs() <= Tm * (1 + 1e-15)).all())
    assert float(ref.abs().max()) < R.F16_MAX and float(hid.abs().max()) <= 0.99  # finite in f16 for every finite gate
    if case == (64, 1024, 0):
        got = sorted(gate.reshape(-1)[:2 * 0x7C00].view(torch.int16).tolist())
        assert got == sorted(R.finite_f16().view(torch.int16).tolist()) and len(set(got)) == 2 * 0x7C00
        assert float(ref.abs().max()) > 60000  # the largest gates do reach the top of the f16 range


@pytest.mark.parametrize("case", R.COLSUM_CASES)
def test_colsum_terms_and_chunking(case):
    nb, rpb, cols, ld = case
    for fam in R.COLSUM_FAMILIES:
        x = R.colsum_inputs(case, fam)
        assert x.shape == (nb * rpb, ld) and (ld == cols or bool(torch.isnan(x[:, cols:]).all()))
        prior = torch.randn(nb, cols, generator=R._gen(10))
        s, a = R.colsum_terms(F64, x, nb, rpb, cols, prior)
        want = torch.stack([x[b * rpb:(b + 1) * rpb, :cols].to(F64).sum(0) for b in range(nb)]) + prior.to(F64)
        close64(s, want, what="colsum")
        s0, a0 = R.colsum_terms(F64, x, nb, rpb, cols)
        if fam == "cancel" and rpb > 1:
            assert float((s0.abs() / a0).max()) < 0.02, "columns cancel"
    chunks = R.colsum_chunks(nb, rpb)
    rows_per = R.cdiv(rpb, chunks)
    empty = sum(1 for c in range(chunks) if c * rows_per >= rpb)
    assert {(1, 9000, 136, 136): (128, 1), (1100, 128, 8, 8): (1, 0), (4, 130, 320, 328): (2, 0)}.get(case, (chunks, empty)) == (chunks, empty)
    assert chunks <= 128 and chunks * rows_per >= rpb


# ---- the M32 figures -------------------------------------------------------------------------------------------------------------------------
def measure_m32() -> dict:
    H = R.ADAMW_HYPER
    out = {}
    mse = [(R.mse_inputs(n, lay), lay[0], gs) for n in R.MSE_SIZES for lay in R.MSE_LAYOUTS for gs in R.MSE_GRAD_SCALES]
    out["M32_MSE_LOSS"] = max(m32_of(R.pick(R.mse_terms, 0), *pt, Cc, gs) for pt, Cc, gs in mse)
    out["M32_MSE_DPRED"] = max(m32_of(R.pick(R.mse_terms, 1), *pt, Cc, gs) for pt, Cc, gs in mse)
    out["M32_SUMSQ"] = max(m32_of(R.sumsq_terms, R.sumsq_inputs(n)) for n in R.SUMSQ_ALIGNED + R.SUMSQ_MISALIGNED)
    mv, up = 0.0, 0.0
    for n in R.ADAMW_NS:
        for step in R.ADAMW_STEPS:
            for wd in R.ADAMW_WDS:
                for gs in R.ADAMW_GRAD_SCALES:
                    for clip0 in R.ADAMW_CLIPS:
                        a = R.adamw_inputs(n, gs)
                        kw = dict(H, wd=wd, step=step, clip0=clip0, grad_scale=gs)
                        mv = max(mv, m32_of(R.pick(R.adamw_terms, 0), *a, **kw), m32_of(R.pick(R.adamw_terms, 1), *a, **kw))
                        up = max(up, m32_of(R.pick(R.adamw_terms, 2), *a, **kw))
    out["M32_ADAMW_MV"], out["M32_ADAMW"] = mv, up
    out["M32_GEGLU"] = max(m32_of(R.geglu_fwd_terms, R.geglu_inputs(c), c[2]) for c in R.GEGLU_CASES)
    return out


def test_m32_constants_are_the_measured_ones():
    meas = measure_m32()
    for n, m in meas.items():
        rec = G.M32_MEASURED[n]
        print(f"{n}: measured {m:.3e}, recorded {rec:.3e}, constant {getattr(G, n):.3e}")
        assert 0.8 * rec <= m <= 1.0005 * rec, (n, m, rec)
        assert getattr(G, n) == 4 * rec
    assert set(meas) == set(G.M32_MEASURED)
    # the sums that have no term arithmetic (exact f16 -> f32 conversions), and the fixed three additions of the 2x2 sum
    for case in R.COLSUM_CASES[:3]:
        assert m32_of(R.colsum_terms, R.colsum_inputs(case, "gauss"), *case[:3]) == 0.0
    for case in R.POOL_CASES:
        assert m32_of(R.sumpool_terms, R.pool_inputs(case, True)) <= G.M32_SUMPOOL == 3 * 2.0 ** -24


# ---- the conditions the GPU module's inputs meet -----------------------------------------------------------------------------------------------
def test_mse_conditions():
    assert R.MSE_THREADS == 65536 and [n - R.MSE_THREADS * (n // R.MSE_THREADS) for n in R.MSE_SIZES] == [1024, 296, 8]
    assert [R.mse_chain(n) for n in R.MSE_SIZES] == [11, 12, 14]
    for n in R.MSE_SIZES:
        for lay in R.MSE_LAYOUTS:
            Cc, ldp, ldt = lay
            pred, target = R.mse_inputs(n, lay)
            assert pred.shape == (n // ldp, ldp) and target.shape == (n // ldp, ldt)
            assert not bool(torch.isnan(pred[:, :Cc]).any()) and (ldp == Cc or bool(torch.isnan(pred[:, Cc:]).all()))
            assert ldt == Cc or bool(torch.isnan(target[:, Cc:]).all())
            for gs in R.MSE_GRAD_SCALES:
                d64 = R.mse_terms(F64, pred, target, Cc, gs)[1][0]
                assert float(d64.abs().max()) < R.F16_MAX, "no reference dpred overflows f16"
    assert R.MSE_GRAD_SCALES[1] == 16384.0


def test_sumsq_conditions():
    S = R.SUMSQ_S
    assert S == 524288 and max(R.SUMSQ_ALIGNED) * 4 <= 25.2e6 + 64  # the largest buffer: 25 MB
    paths = {n: {R.sumsq_path(n, i, True) for i in list(range(0, n, max(1, n // 4001))) + list(range(max(0, n - 4), n))} for n in R.SUMSQ_ALIGNED}
    assert paths[4 * S] == {"remainder"} and paths[5003] == {"remainder", "tail"} and paths[3] == {"tail"}
    assert paths[4 * (S + 1) + 1] == {"first", "second", "remainder", "tail"}
    assert R.sumsq_path(4 * (S + 1) + 1, 4 * S, True) == "second" and R.sumsq_path(4 * (S + 1) + 1, 0, True) == "first"
    assert R.sumsq_path(4 * (S + 1) + 1, 4, True) == "remainder"
    assert paths[4 * (2 * S + 77) + 3] == paths[4 * (3 * S + 5) + 2] == {"first", "second", "remainder", "tail"}
    n = max(R.SUMSQ_ALIGNED)
    plants = R.sumsq_plants(n, True)
    assert {p for p, _ in plants} == {"first", "second", "remainder", "tail"}
    for name, idx in plants:
        assert R.sumsq_path(n, idx, True) == name, (name, idx)
    assert plants[2][1] >> 2 >= 2 * S and plants[3][1] >> 2 >= 3 * S  # the second unrolled trip's two loads as well
    nm = max(R.SUMSQ_MISALIGNED)
    pm = R.sumsq_plants(nm, False)
    assert pm[0][1] < S <= pm[1][1] < nm
    assert [R.sumsq_chain(n, True) for n in (5, 4 * S, 4 * (S + 1) + 1, 4 * (3 * S + 5) + 2)] == [14, 14, 16, 18]
    assert [R.sumsq_chain(n, False) for n in R.SUMSQ_MISALIGNED] == [13, 13, 14]
    x = R.sumsq_inputs(5003)
    assert float(R.sumsq_terms(F64, x)[0]) < 1e30 and abs(float(x.std()) / R.LOSS_SCALE - 1) < 0.05


def test_clip_conditions():
    by = {c[0]: c[1:] for c in R.CLIP_CASES}
    want_flag = dict(zero=0, tiny=0, below=0, above=0, **{"1e30": 0, "past 3e38": 1}, inf=1, nan=1)
    for name, (ss, mx, inv) in by.items():
        c64, n64, f64_ = R.clip_terms(F64, ss, mx, inv)
        c32, n32, f32_ = R.clip_terms(F32, ss, mx, inv)
        assert f64_ == f32_ == want_flag[name], name
        if f64_:
            assert c64 == c32 == 0.0
            continue
        assert abs(n32 - n64) <= R.CLIP_NORM_ROUNDINGS * 2.0 ** -24 * n64 and abs(c32 - c64) <= R.CLIP_COEF_ROUNDINGS * 2.0 ** -24 * c64
        # exactly 1 below max_norm, below 1 above it, and no case within the error of the threshold
        margin = 1 - 4 * R.CLIP_COEF_ROUNDINGS * 2.0 ** -24
        assert (n64 + R.f32v(1e-6) <= mx * margin) or (n64 + R.f32v(1e-6) >= mx / margin), name
        assert (c64 == 1.0) == (name in ("zero", "tiny", "below")) and (c32 == 1.0) == (c64 == 1.0), name
    n_below, n_above = R.clip_terms(F64, *by["below"])[1], R.clip_terms(F64, *by["above"])[1]
    assert 0.9998 < n_below < 1.0 < n_above < 1.0002
    ss, _, inv = by["past 3e38"]
    assert math.isfinite(R.f32v(ss)) and 3.0e38 < math.sqrt(R.f32v(ss)) * R.f32v(inv) < 3.4e38  # finite in f32, past the kernel's threshold


def test_adamw_conditions():
    H = R.ADAMW_HYPER
    for gs in R.ADAMW_GRAD_SCALES:
        for n in R.ADAMW_NS:
            p, g, m, v = R.adamw_inputs(n, gs)
            assert bool((v >= 0).all()) and all(t.dtype == F32 and t.shape == (n,) for t in (p, g, m, v))
            if n < 2:
                continue
            assert float(g[0]) == 0 == float(m[0]) == float(v[0])
            gi = float(g[1]) * R.f32v(gs)
            assert 0.9e18 < abs(gi) < 1.1e18 and math.isfinite(R.f32v(gi * gi)) and math.isfinite(R.f32v(float(g[1])))
            for step in (1, 1000):
                for clip0 in R.ADAMW_CLIPS:
                    for dt in (F32, F64):
                        r = R.adamw_terms(dt, p, g, m, v, **H, wd=1e-2, step=step, clip0=clip0, grad_scale=gs)
                        assert all(bool(torch.isfinite(val).all()) for val, _ in r)
                        assert float(r[2][0][0]) == -float(p[0].to(dt) * (R._c(H["lr"], dt) * R._c(1e-2, dt)))  # no 0 / 0: the decay alone
    # eps matters for some elements and not for others; the small parameters resolve the step
    p, g, m, v = R.adamw_inputs(5000, 1.0)
    (_, _), (v64, _), (u64, tu), _ = R.adamw_terms(F64, p, g, m, v, **H, wd=0.0, step=3)
    r = v64.sqrt() / R.f32v(H["eps"])
    assert int((r < 1e3).sum()) > 100 and int((r > 1e6).sum()) > 100
    small = p.abs() < 1e-3
    assert int(small.sum()) > 2000 and float((u64.abs() / p.to(F64).abs())[small].median()) > 1
    assert R.ADAMW_OFFSET % 2 == 1


def test_cast_values_are_what_they_claim():
    v = R.cast_values()
    h, mid, below, above = v["exact"], v["mid"], v["below"], v["above"]
    bits = torch.arange(0, 0x7C00, dtype=torch.int16)
    assert bits_equal(h.half(), bits.view(F16)) and h.numel() == 31744
    lo, hi = h[:-1].to(F64), h[1:].to(F64)
    assert bool((mid.to(F64) * 2 == lo + hi).all()) and bool((lo < below.to(F64)).all()) and bool((below < mid).all()) and bool((mid < above).all())
    assert bool((above.to(F64) < hi).all())
    even = torch.where(bits[:-1] % 2 == 0, bits[:-1], bits[1:])
    assert bits_equal(mid.half(), even.view(F16)), "ties go to even"
    assert bits_equal(below.half(), bits[:-1].view(F16)) and bits_equal(above.half(), bits[1:].view(F16))
    sp = v["special"]
    want = {65504.0: 65504.0, 65520.0: math.inf, float(np.nextafter(np.float32(65520), np.float32(0))): 65504.0, 2.0 ** -25: 0.0,
            float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))): 2.0 ** -24, float(np.nextafter(np.float32(2.0 ** -25), np.float32(0))): 0.0,
            2.0 ** -149: 0.0, 1e30: math.inf}
    got = {float(a): float(b) for a, b in zip(sp, sp.half()) if a == a}
    for a, b in want.items():
        assert got[R.f32v(a)] == b, (a, b)
        assert -R.f32v(a) not in got or got[-R.f32v(a)] == -b, (a, b)
    assert abs(float(np.nextafter(np.float32(65520), np.float32(0))) - 65519.996) < 1e-3
    assert int(torch.isnan(sp).sum()) == 1 and any(math.copysign(1, float(a)) < 0 and a == 0 for a in sp)
    x = R.cast_input()
    assert x.numel() % 256 != 0 and x.dtype == F32
    with np.errstate(over="ignore"):
        assert bits_equal(x.half(), torch.from_numpy(x.numpy().astype(np.float16))), "torch's CPU cast is numpy's (round to nearest even)"


def test_layout_conditions():
    for B, H, W, Cc, k, stride, pad in R.IM2COL_CASES:
        Ho, Wo = R.conv_out_hw(H, W, k, stride, pad)
        assert (B * Ho * Wo) % 8 == 0 and Cc % 8 == 0
    assert any(c[1] != c[2] for c in R.IM2COL_CASES) and all(c[1] != c[2] or c[4] == 1 for c in R.IM2COL_CASES)  # H != W wherever k > 1
    assert all(c[3] % 8 == 0 for c in R.POOL_CASES) and any(c[1] != c[2] for c in R.POOL_CASES)
    x = R.upsample_input(R.POOL_CASES[1])
    xi = x.view(torch.int16)
    assert int((xi == -0x8000).sum()) > 0 and int(torch.isnan(x).sum()) >= 2 and len(set(xi[torch.isnan(x)].tolist())) >= 2  # -0, two NaN payloads
    for case in R.GEGLU_CASES:
        M, Hd, blk = case
        assert Hd % 8 == 0 and blk % 8 == 0 and (blk == 0 or Hd % blk == 0)
