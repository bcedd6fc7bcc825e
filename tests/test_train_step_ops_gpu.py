"""-m gpu: the kernels of csrc/backward.hip that turn the prediction into a loss (gn_mse_loss), the gradient into a norm and a clip coefficient
(gn_sumsq_f32, gn_clip_coef) and the clipped gradient into new parameters (gn_adamw_flat, gn_ema_flat, gn_cast_f32_f16), the column sums of
the bias / shift gradients (gn_colsum_f32), the layout helpers of the conv backward (gn_im2col_t, gn_zero_upsample2x, gn_sumpool2x2) and
gn_geglu_fwd, each against the float64 / exact CPU reference of tests/train_step_ref.py evaluated from the kernel's own inputs, PER ELEMENT.
Bounds as in tests/test_small_ops_gpu.py: moves and explicitly rounded f32 sequences bit for bit; f16 outputs of a short f32 formula within
ulp16(ref64) + M32 * sum|terms|; f32 sums within (n * 2^-24 + M32) * sum|t_i| with n the longest addition chain read off the kernel
(train_step_ref.*_chain); f32 outputs of a short formula within M32 * sum|terms|.  tests/test_train_step_ref_cpu.py checks the references,
the M32 figures and the conditions the inputs are chosen to meet.

Path -> case:
  mse grid-stride trips 1 (idle threads) / 2 (296 threads) / 3 + 8          MSE_SIZES x (C, ld_pred, ld_target) x grad_scale {1, 16384}; dpred = NULL
  sumsq remainder only / unrolled once (thread 0) / all unrolled + 77 /      n = 4S / 4(S+1)+1 / 4(2S+77)+3 / 4(3S+5)+2 (S = 2048 * 256); n = 1 .. 5003: tail
  two unrolled trips (5 threads); misaligned scalar loop, 1 and 2 trips      a view one float into the buffer, n = 5, 5003, S + 100
  an inf / NaN on every one of those loads reaches clip[2]                   test_sumsq_planted_nonfinite
  colsum one chunk / two / the 128 cap with an empty last chunk / want = 1   COLSUM_CASES, gauss and cancelling columns, accumulate 0 / 1, NaN pads

Largest err / bound measured on MI355X (printed with -s after the module's last test):
  mse dpred 0.5000, mse loss 0.060      sumsq 0.083      clip norm 0.139, clip coef 0.087      adamw m 0.217, v 0.194, update 0.493
  colsum 0.018      sumpool 0.4999      geglu fwd 0.4997      (ema, cast, im2col_t, zero_upsample2x: bit for bit)
The f16 outputs sit at 0.5 because half an f16 ulp IS reached (a tie of the store) and the bound grants a whole one.  The AdamW update's
figure before / after the bias corrections moved to f64: test_adamw_flat.  The module (116 tests) takes 10 s."""
import pytest
import torch

import train_step_ref as R
from act_ops_ref import assert_f16_formula, assert_f32_sum, bits_equal, ulp16
from genima_amd import train_ops as T
from genima_amd._lib import GenimaHipError, check
from test_norm_bwd_gpu import SENTINEL16, SENTINEL32, nan_workspace, sent16, sent32
from test_small_ops_gpu import _guard_intact, _guarded, _NanEmpty

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
U32 = 2.0 ** -24

# act_ops_ref.m32_of over the inputs of this file, measured on the CPU (tests/test_train_step_ref_cpu.py re-measures them), then x 4:
M32_MEASURED = {
    "M32_MSE_LOSS": 5.02e-8,    # mse_terms, the loss: d, d * d and the f32 1 / (pixels C), every size x layout x grad_scale: 5.02e-8 -> 2.01e-7
    "M32_MSE_DPRED": 1.271e-7,  # mse_terms, dpred: d, the host's gs, gs * d: 1.271e-7 -> 5.08e-7
    "M32_SUMSQ": 2.70e-8,       # sumsq_terms: the rounding of x * x, every n: 2.70e-8 -> 1.08e-7
    "M32_ADAMW_MV": 1.16e-7,    # adamw_terms, m' and v', every n x step x wd x grad_scale x clip: 1.16e-7 -> 4.64e-7
    "M32_ADAMW": 3.69e-7,       # adamw_terms, the update, the same runs: 3.69e-7 -> 1.48e-6
    "M32_GEGLU": 1.50e-7,       # geglu_fwd_terms, every case (every finite gate among them): 1.50e-7 -> 6.00e-7
}
M32_MSE_LOSS = 4 * M32_MEASURED["M32_MSE_LOSS"]
M32_MSE_DPRED = 4 * M32_MEASURED["M32_MSE_DPRED"]
M32_SUMSQ = 4 * M32_MEASURED["M32_SUMSQ"]
M32_ADAMW_MV = 4 * M32_MEASURED["M32_ADAMW_MV"]
M32_ADAMW = 4 * M32_MEASURED["M32_ADAMW"]   # no allowance for the bias corrections: the host forms them in f64 and rounds once
M32_GEGLU = 4 * M32_MEASURED["M32_GEGLU"]
M32_SUMPOOL = 3 * U32                       # not measured: three f32 additions ((a + b) + c) + d of exactly converted f16 values

WORST: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the largest err / bound per kernel (with -s), the figures of the docstring; each was asserted <= 1 where measured."""
    yield
    for n in sorted(WORST):
        print(f"\n{n}: {WORST[n]:.4f}", end="")


def note(name: str, got, ref, bound):
    err = (got.detach().cpu().to(F64) - ref.to(F64)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.to(F64).clamp_min(1e-300))
    WORST[name] = max(WORST.get(name, 0.0), float(r.max()))


def nan32(n: int, guard: int = 64):
    """-> (NaN-filled f32 device tensor [n], the flat allocation it heads: ``guard`` more NaNs behind it)."""
    flat = torch.full((n + guard,), NAN, dtype=F32, device="cuda")
    return flat[:n], flat


# ---- gn_mse_loss --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", R.MSE_GRAD_SCALES)
@pytest.mark.parametrize("layout", R.MSE_LAYOUTS, ids=lambda c: "C%d-ldp%d-ldt%d" % c)
@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse_loss(engine, n, layout, gs):
    Cc, ldp, ldt = layout
    pred, target = R.mse_inputs(n, layout)
    (l64, lt), (d64, dterms) = R.mse_terms(F64, pred, target, Cc, gs)
    pred_d, target_d = pred.cuda(), target.cuda()
    pixels = pred.shape[0]
    dpred, flat = _guarded((pixels, ldp))
    loss, loss_flat = nan32(1)
    ws = nan_workspace(engine, 4096)
    check(engine.lib.gn_mse_loss(engine._ctx, pred_d.data_ptr(), target_d.data_ptr(), dpred.data_ptr(), loss.data_ptr(), ws.data_ptr(), pixels, Cc, ldp, ldt,
                                 float(gs)), "gn_mse_loss")
    what = f"mse n {n} {layout} gs {gs}"
    note("mse dpred", dpred, d64, ulp16(d64) + M32_MSE_DPRED * dterms)
    assert_f16_formula(dpred, d64, dterms, M32_MSE_DPRED, what + " dpred")
    assert ldp == Cc or bits_equal(dpred[:, Cc:], torch.zeros(pixels, ldp - Cc, dtype=F16)), "pad channels: +0"
    assert _guard_intact(flat, pixels * ldp) and bool(torch.isnan(loss_flat[1:]).all())
    chain = R.mse_chain(n)
    note("mse loss", loss, l64, (chain * U32 + M32_MSE_LOSS) * lt)
    assert_f32_sum(loss, l64, lt, chain, M32_MSE_LOSS, what + " loss")
    # dpred = NULL: the same loss bits
    loss2, _ = nan32(1)
    check(engine.lib.gn_mse_loss(engine._ctx, pred_d.data_ptr(), target_d.data_ptr(), None, loss2.data_ptr(), ws.data_ptr(), pixels, Cc, ldp, ldt, float(gs)),
          "gn_mse_loss")
    assert bits_equal(loss2, loss)
    # the wrapper the trainer calls
    loss3, dpred3 = T.mse_loss(engine, pred_d, target_d, Cc, gs)
    assert bits_equal(loss3, loss) and bits_equal(dpred3, dpred)
    assert bits_equal(pred_d, pred) and bits_equal(target_d, target)


# ---- gn_sumsq_f32 -------------------------------------------------------------------------------------------------------------------------------
def sumsq_view(x, aligned: bool):
    """x on the device inside a NaN-filled allocation (a read past either end poisons the sum): at its start, or one float in."""
    off = 0 if aligned else 1
    buf = torch.full((x.numel() + off + 8,), NAN, dtype=F32, device="cuda")
    view = buf[off:off + x.numel()]
    view.copy_(x)
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


SUMSQ_RUNS = [(n, True) for n in R.SUMSQ_ALIGNED] + [(n, False) for n in R.SUMSQ_MISALIGNED]


@pytest.mark.parametrize("n,aligned", SUMSQ_RUNS)
def test_sumsq(engine, n, aligned):
    x = R.sumsq_inputs(n)
    s64, t64 = R.sumsq_terms(F64, x)
    out, flat = nan32(1)
    nan_workspace(engine, 8192)
    T.sumsq(engine, sumsq_view(x, aligned), out)
    chain = R.sumsq_chain(n, aligned)
    note("sumsq", out, s64, (chain * U32 + M32_SUMSQ) * t64)
    assert_f32_sum(out, s64, t64, chain, M32_SUMSQ, f"sumsq n {n} aligned {aligned} (chain {chain})")
    assert bool(torch.isnan(flat[1:]).all())


@pytest.mark.parametrize("aligned", [True, False])
def test_sumsq_planted_nonfinite(engine, aligned):
    """One inf, -inf or NaN on each load path of the largest buffer: clip[2] = 1 and clip[0] = 0 through gn_clip_coef."""
    n = max(R.SUMSQ_ALIGNED if aligned else R.SUMSQ_MISALIGNED)
    view = sumsq_view(R.sumsq_inputs(n), aligned)
    out, clip = torch.zeros(1, device="cuda"), torch.zeros(3, device="cuda")

    def run():
        out.fill_(NAN), clip.fill_(NAN)
        T.sumsq(engine, view, out)
        T.clip_coef(engine, out, clip, 1.0, 1.0 / R.LOSS_SCALE)
        return clip.cpu().tolist()

    c = run()
    assert c[2] == 0.0 and 0 < c[0] < 1 and c[1] > 1, c
    for path, idx in R.sumsq_plants(n, aligned):
        assert R.sumsq_path(n, idx, aligned) == path
        keep = view[idx].clone()
        for bad in (INF, -INF, NAN):
            view[idx] = bad
            c = run()
            assert c[2] == 1.0 and c[0] == 0.0, f"{bad} at index {idx} ({path} load) was dropped: clip {c}"
        view[idx] = keep
    assert run()[2] == 0.0


# ---- gn_clip_coef -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CLIP_CASES, ids=lambda c: c[0])
def test_clip_coef(engine, case):
    name, ss, max_norm, inv = case
    c64, n64, f64_ = R.clip_terms(F64, ss, max_norm, inv)
    clip, flat = nan32(3)
    T.clip_coef(engine, torch.tensor([ss], dtype=F32).cuda(), clip, max_norm, inv)
    got = flat.cpu().to(F64)
    coef, norm, flag = (float(v) for v in got[:3])
    print(f"clip {name}: coef {coef!r} (ref {c64!r}), norm {norm!r} (ref {n64!r}), flag {flag}")
    assert bool(torch.isnan(got[3:]).all())
    assert flag == f64_, "the found-inf flag is exact"
    if f64_:
        assert coef == 0.0 and (norm != norm if name == "nan" else norm > 3.0e38)
        if name == "past 3e38":
            assert abs(norm - n64) <= R.CLIP_NORM_ROUNDINGS * U32 * n64
        return
    assert abs(norm - n64) <= R.CLIP_NORM_ROUNDINGS * U32 * n64
    assert abs(coef - c64) <= R.CLIP_COEF_ROUNDINGS * U32 * c64
    if c64 == 1.0:
        assert coef == 1.0, "below max_norm the coefficient is exactly 1"
    else:
        assert coef < 1.0
    if n64 > 0:
        WORST["clip norm"] = max(WORST.get("clip norm", 0.0), abs(norm - n64) / (R.CLIP_NORM_ROUNDINGS * U32 * n64))
        WORST["clip coef"] = max(WORST.get("clip coef", 0.0), abs(coef - c64) / (R.CLIP_COEF_ROUNDINGS * U32 * c64))


# ---- gn_adamw_flat ------------------------------------------------------------------------------------------------------------------------------
def flat_slice(t, fill=NAN):
    """t [n] -> (the slice [OFFSET : OFFSET + n] holding t, its flat device allocation, filled with ``fill`` around it)."""
    n, off = t.numel(), R.ADAMW_OFFSET
    flat = torch.full((off + n + 64,), fill, dtype=t.dtype, device="cuda")
    flat[off:off + n] = t.cuda()
    return flat[off:off + n], flat


def around_intact(flat, n):
    off = R.ADAMW_OFFSET
    return bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + n:]).all())


def adamw_run(engine, tensors, step, wd, gs, clip, half: bool, zero_grad: bool):
    """One gn_adamw_flat call on fresh odd-offset slices -> the CPU copies (p, g, m, v, half or None) and whether everything around the
    slices kept its NaN."""
    n = tensors[0].numel()
    (p, pf), (g, gf), (m, mf), (v, vf) = (flat_slice(t) for t in tensors)
    h, hf = flat_slice(torch.full((n,), NAN, dtype=F16)) if half else (None, None)
    T.adamw(engine, p, g, m, v, **R.ADAMW_HYPER, wd=wd, step=step, clip=clip, grad_scale=gs, half_out=h, zero_grad=zero_grad)
    ok = all(around_intact(f, n) for f in (pf, gf, mf, vf)) and (hf is None or around_intact(hf, n))
    return p.cpu(), g.cpu(), m.cpu(), v.cpu(), (None if h is None else h.cpu()), ok


def adamw_update_error(p_old, p_dev, u64, tu):
    """-> (|device update - f64 update|, its bound): the update p' - p formed in f64 from the device's f32 values; M32_ADAMW * terms for the
    update's own arithmetic plus the roundings of p (train_step_ref.adamw_p_rounding)."""
    return (p_dev.to(F64) - p_old.to(F64) - u64).abs(), M32_ADAMW * tu + R.adamw_p_rounding(p_old, p_dev)


def adamw_update_deviation(engine, steps=range(1, 11)) -> dict:
    """step -> worst |device update - f64 update| / sum|terms| over the elements whose parameter is small (|p| < 1e-3: p's own rounding is
    < 1e-8 of the step) and whose step is not (terms > 1e-3): what the arithmetic of the step -- its bias corrections included -- costs."""
    out = {}
    t = R.adamw_inputs(5000, 1.0)
    for step in steps:
        p_dev = adamw_run(engine, t, step, 0.0, 1.0, None, False, False)[0]
        _, _, (u64, tu), _ = R.adamw_terms(F64, *t, **R.ADAMW_HYPER, wd=0.0, step=step)
        sel = (t[0].abs() < 1e-3) & (tu > 1e-3)
        out[step] = float(((p_dev.to(F64) - t[0].to(F64) - u64).abs() / tu)[sel].max())
    return out


@pytest.mark.parametrize("step", R.ADAMW_STEPS)
@pytest.mark.parametrize("n", R.ADAMW_NS)
def test_adamw_flat(engine, n, step):
    """Single steps from a random state on odd-offset slices of flat buffers, over clip {absent, 0.37, skip} x grad_scale {1, 1 / 65536} x wd {0,
    1e-2} x half_out x zero_grad.  m, v: M32_ADAMW_MV * their two terms.  The update p' - p: M32_ADAMW * its two terms + the roundings of p.

    The bias corrections 1 - beta^step.  Worst |update - f64| / terms over the small-parameter elements at steps 1 .. 10
    (adamw_update_deviation), measured on MI355X: with the host forming them as 1.0f - powf(beta, step) 3.65e-6 (step 2; 3.21e-6, 3.19e-6,
    2.57e-6 at steps 3 - 5, 2.4e-7 at step 1), which is 2.5 x M32_ADAMW = 1.48e-6 -- this test failed at steps 2 and 3 for every n; with
    (float)(1.0 - pow((double)beta, step)) 2.96e-7 (step 6; 2.3e-7 .. 3.0e-7 at every step), 0.20 x M32_ADAMW."""
    H = R.ADAMW_HYPER
    refs = {}
    for wd in R.ADAMW_WDS:
        for gs in R.ADAMW_GRAD_SCALES:
            t = R.adamw_inputs(n, gs)
            p0, g0, m0, v0 = t
            for mode in ("none", "clip", "skip"):
                clip0 = None if mode == "none" else R.ADAMW_CLIPS[1]
                clip = None if mode == "none" else torch.tensor([clip0, 123.0, 1.0 if mode == "skip" else 0.0], dtype=F32).cuda()
                key = (wd, gs, clip0)
                if mode != "skip" and key not in refs:
                    refs[key] = R.adamw_terms(F64, *t, **H, wd=wd, step=step, clip0=clip0, grad_scale=gs)
                for half in (False, True):
                    for zg in (False, True):
                        what = f"adamw n {n} step {step} wd {wd} gs {gs} clip {mode} half {half} zero_grad {zg}"
                        p, g, m, v, h, ok = adamw_run(engine, t, step, wd, gs, clip, half, zg)
                        assert ok, what + ": wrote outside its slice"
                        assert bits_equal(g, torch.zeros(n)) if zg else bits_equal(g, g0), what + ": gradient"
                        if mode == "skip":
                            assert bits_equal(p, p0) and bits_equal(m, m0) and bits_equal(v, v0), what + ": a skipped step wrote"
                            assert h is None or bool(torch.isnan(h).all()), what + ": half_out written on a skipped step"
                            continue
                        (m64, tm), (v64, tv), (u64, tu), _ = refs[key]
                        assert bool(torch.isfinite(p).all()), what
                        note("adamw m", m, m64, M32_ADAMW_MV * tm), note("adamw v", v, v64, M32_ADAMW_MV * tv)
                        assert_f32_sum(m, m64, tm, 0, M32_ADAMW_MV, what + " m")
                        assert_f32_sum(v, v64, tv, 0, M32_ADAMW_MV, what + " v")
                        err, bound = adamw_update_error(p0, p, u64, tu)
                        WORST["adamw update"] = max(WORST.get("adamw update", 0.0), float((err / bound.clamp_min(1e-300)).max()))
                        worst = int((err - bound).argmax())
                        assert bool((err <= bound).all()), (f"{what}: |update - ref| {float(err[worst]):.6e} > bound {float(bound[worst]):.6e} at {worst} "
                                                            f"(p {float(p0[worst])!r} -> {float(p[worst])!r}, ref update {float(u64[worst])!r})")
                        if n >= 2:  # g = m = v = 0: 0 / (0 + eps), the decay alone
                            assert float(m[0]) == 0.0 and float(v[0]) == 0.0 and (wd != 0.0 or bits_equal(p[:1], p0[:1]))
                        assert h is None or bits_equal(h, p.half()), what + ": half_out"


def test_adamw_bias_corrections_measured(engine):
    dev = adamw_update_deviation(engine)
    print("adamw update deviation by step:", {k: f"{v:.3e}" for k, v in dev.items()})
    assert max(dev.values()) <= M32_ADAMW + 1e-8  # (1e-8: what is left of p's rounding on the selected elements)


# ---- gn_ema_flat --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("omd", R.EMA_OMDS)
@pytest.mark.parametrize("n", R.EMA_NS)
def test_ema_flat(engine, n, omd):
    g = R._gen(11, n)
    s, q = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    flat = torch.full((n + 64,), NAN, dtype=F32, device="cuda")
    flat[:n] = s.cuda()
    q_d = q.cuda()
    T.ema_flat(engine, flat[:n], q_d, omd)
    assert bits_equal(flat[:n], R.ema_f32(s, q, omd)), "s - omd * (s - q), each operation rounded"
    assert bool(torch.isnan(flat[n:]).all()) and bits_equal(q_d, q)
    if omd == 1.0:
        assert float((flat[:n].cpu() - q).abs().max()) <= 2 * U32 * float(s.abs().max() + q.abs().max())


@pytest.mark.parametrize("n", [1022, 3, 0])
def test_ema_flat_refusal(engine, n):
    shadow, param = sent32(1024), torch.zeros(1024, device="cuda")
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_ema_flat"):
        check(engine.lib.gn_ema_flat(engine._ctx, shadow.data_ptr(), param.data_ptr(), n, 0.5), "gn_ema_flat")
    engine.synchronize()
    assert bool((shadow.view(torch.int32) == SENTINEL32).all())


# ---- gn_cast_f32_f16 ----------------------------------------------------------------------------------------------------------------------------
def test_cast_f32_f16(engine):
    x = R.cast_input()
    n = x.numel()
    assert n % 256 != 0
    out, flat = _guarded((n,))
    x_d = x.cuda()
    T.cast_f32_f16(engine, x_d, out)
    want = x.half()
    got = out.cpu()
    diff = (got.view(torch.int16) != want.view(torch.int16)).nonzero().flatten()
    assert diff.numel() == 0, (f"{diff.numel()} values differ from the CPU cast, first: {float(x[diff[0]])!r} -> {float(got[diff[0]])!r} "
                               f"(CPU {float(want[diff[0]])!r})")
    assert _guard_intact(flat, n) and bits_equal(x_d, x)


# ---- gn_colsum_f32 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.COLSUM_FAMILIES)
@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_colsum(engine, case, family):
    nb, rpb, cols, ld = case
    x = R.colsum_inputs(case, family)
    x_d = x.cuda()
    chain = R.colsum_chain(nb, rpb)
    prior = torch.randn(nb, cols, generator=R._gen(12, nb, cols)) * 3
    for acc in (0, 1):
        out, flat = nan32(nb * cols)
        if acc:
            out.copy_(prior.view(-1))
        nan_workspace(engine, engine.lib.gn_colsum_workspace_bytes(nb, rpb, cols))
        T.colsum(engine, x_d, out, nb, rpb, cols, ld, accumulate=bool(acc))
        ref, terms = R.colsum_terms(F64, x, nb, rpb, cols, prior if acc else None)
        what = f"colsum {case} {family} accumulate {acc} (chain {chain})"
        note("colsum", out.view(nb, cols), ref, chain * U32 * terms)
        assert_f32_sum(out.view(nb, cols), ref, terms, chain, 0.0, what)
        assert bool(torch.isnan(flat[nb * cols:]).all()), what + ": wrote past out"
    assert bits_equal(x_d, x)


# ---- gn_im2col_t --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_im2col_t(engine, case, monkeypatch):
    B, H, W, Cc, k, stride, pad = case
    x = R.map_inputs(B, H, W, Cc)
    ref = R.im2col_t_ref(x, k, stride, pad)
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.im2col_t(engine, x.cuda(), k, stride, pad)
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr()
    assert tuple(out.shape) == tuple(ref.shape)
    assert bits_equal(out, ref)  # every element written (no NaN left), the padding taps +0
    assert _guard_intact(fake.flats[0], out.numel())


@pytest.mark.parametrize("what", ["M % 8", "C % 8"])
def test_im2col_t_refusals(engine, what):
    B, H, W, Cc, k, stride, pad = (1, 7, 9, 16, 3, 2, 1) if what == "M % 8" else (1, 4, 6, 12, 3, 1, 1)  # M = 20; C = 12
    x, out = torch.zeros(B, H, W, 16, dtype=F16, device="cuda"), sent16(9 * 16 * 64)
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_im2col_t"):
        check(engine.lib.gn_im2col_t(engine._ctx, x.data_ptr(), out.data_ptr(), B, H, W, Cc, k, stride, pad), "gn_im2col_t")
    engine.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL16).all()), f"{what}: the output was written"


# ---- gn_zero_upsample2x / gn_sumpool2x2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_zero_upsample2x(engine, case, monkeypatch):
    x = R.upsample_input(case)
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.zero_upsample2x(engine, x.cuda())
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr()
    assert bits_equal(out, R.zero_upsample_ref(x))  # -0 and the NaN payloads carried, +0 elsewhere
    assert _guard_intact(fake.flats[0], out.numel())


@pytest.mark.parametrize("cancel", [False, True])
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sumpool2x2(engine, case, cancel, monkeypatch):
    x = R.pool_inputs(case, cancel)
    ref, terms = R.sumpool_terms(F64, x)
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.sumpool2x2(engine, x.cuda())
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr()
    note("sumpool", out, ref, ulp16(ref) + M32_SUMPOOL * terms)
    assert_f16_formula(out, ref, terms, M32_SUMPOOL, f"sumpool {case} cancel {cancel}")
    assert _guard_intact(fake.flats[0], out.numel())


@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sumpool_of_zero_upsample_is_the_identity(engine, case):
    x = R.map_inputs(*case)
    assert not bool((x.view(torch.int16) == -0x8000).any())  # no -0: (-0) + 0 is +0
    assert bits_equal(T.sumpool2x2(engine, T.zero_upsample2x(engine, x.cuda())), x)


# ---- gn_geglu_fwd -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEGLU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_geglu_fwd(engine, case, monkeypatch):
    M, Hd, blk = case
    hg = R.geglu_inputs(case)
    ref, terms = R.geglu_fwd_terms(F64, hg, blk)
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.geglu_fwd(engine, hg.cuda(), blk)
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr() and tuple(out.shape) == (M, Hd)
    note("geglu fwd", out, ref, ulp16(ref) + M32_GEGLU * terms)
    assert_f16_formula(out, ref, terms, M32_GEGLU, f"geglu_fwd {case}")  # (asserts every output finite: every finite gate is among them)
    assert _guard_intact(fake.flats[0], out.numel())
