"""-m gpu: the 8-bit blockwise AdamW (csrc/optim8.hip, ``train_ops.adamw8``, ``ControlNetTrainer(use_8bit_adam=True)``) against the
pure-torch restatement of tests/test_adamw8_cpu.py.  bitsandbytes itself is a CUDA library and is not available to pin bit-equality
against; what is held here:

* kernel vs restatement: the kernel runs the restatement's f32 operation sequence (no fma contraction, IEEE divide / sqrt), so its codes
  should equal the f32 restatement's; the bars are what the f32 restatement shows against the f64 one on the same inputs, times 2: the
  share of differing codes and the parameter rel-L2 (CPU, measured: 1 step 0 codes / 3.9e-8, 5 steps 40 of 2 140 180 codes / 2.8e-6),
  and a differing code differs by one index only (measured on an MI355X: 0 codes differ in all four cases, parameters 4.0e-9 / 2.6e-8);
* the quantisation bound |dequant - fp32 moment| <= absmax x the map's largest half-gap (derived, not measured);
* skip / zero_grad, state size (derived from the layout), resume, the cross-kind refusal, InstructPix2Pix + EMA;
* closeness to fp32 AdamW on the tiny trainer: no worse than 2 x what the CPU restatement of the 8-bit step shows against
  torch.optim.AdamW on the fp32 run's recorded gradients (measured on an MI355X, 3 steps, lr 1e-4: parameter rel-L2 4.60e-5 against the
  restatement's 4.42e-5; final-loss gap 3.8e-5 against 4.8e-5; DESIGN.md section 4, "8-bit blockwise AdamW").
Every test needs ``train_ops.adamw8`` or the ``use_8bit_adam`` keyword."""
import time

import pytest
import torch

from genima_amd import configs, optim8, schema, weights
from genima_amd import train_ops as T
from genima_amd.engine import Engine
from genima_amd.host import nchw_to_nhwc
from genima_amd.packing import pack_state_dict
from genima_amd.scheduler import DDPMScheduler
from genima_amd.training import ControlNetTrainer
from test_adamw8_cpu import HYPER, _ragged_case, code_diff, expand_blocks, fresh_state, restate_step
from util import q16, rel_l2

pytestmark = pytest.mark.gpu

FAM = configs.family("tiny")
F32 = torch.float32


class _Dev:
    """The state of one flat buffer on the device + the launch."""

    def __init__(self, E, layout, p):
        self.E = E
        self.table, _, self.n8, _ = optim8.build_block_table(layout)
        nb = self.table.shape[0]
        dev = E.device
        self.tab = self.table.to(dev)
        self.p = p.clone().to(dev)
        self.half = torch.zeros(p.numel(), dtype=torch.float16, device=dev)
        self.mc, self.vc = (torch.zeros(self.n8, dtype=torch.uint8, device=dev) for _ in range(2))
        self.ma, self.va = (torch.zeros(nb, dtype=F32, device=dev) for _ in range(2))
        self.S, self.U = optim8.dynamic_map(True).to(dev), optim8.dynamic_map(False).to(dev)

    def step(self, g, k, clip=None, grad_scale=1.0, zero_grad=True):
        T.adamw8(self.E, self.p, g, self.mc, self.vc, self.ma, self.va, self.tab, self.S, self.U, HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
                 HYPER["eps"], HYPER["wd"], k, clip, grad_scale, half_out=self.half, zero_grad=zero_grad)


@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("clipped", [False, True])
def test_kernel_against_restatement(steps, clipped):
    E = Engine("cuda:0")
    layout, numel, p, grads = _ragged_case()
    d = _Dev(E, layout, p)
    ex = expand_blocks(d.table)
    clip_coef, gscale = (0.37, 1.0 / 1024.0) if clipped else (None, 1.0)
    clip = torch.tensor([clip_coef, 2.7, 0.0], dtype=F32, device=E.device) if clipped else None
    s32, s64 = fresh_state(p, d.table, d.n8, torch.float32), fresh_state(p, d.table, d.n8, torch.float64)
    covered = torch.zeros(numel, dtype=torch.bool)
    covered[ex[0]] = True
    for k in range(steps):
        g = (grads[k] * (1024.0 if clipped else 1.0)).to(E.device)
        d.step(g, k + 1, clip, gscale)
        assert float(g.cpu()[covered].abs().max()) == 0.0 and torch.equal(g.cpu()[~covered], (grads[k] * (1024.0 if clipped else 1.0))[~covered])
        for st, dt in ((s32, torch.float32), (s64, torch.float64)):
            restate_step(st, grads[k] * (1024.0 if clipped else 1.0), ex, k + 1, clip_coef, gscale, dtype=dt, **HYPER)
    torch.cuda.synchronize()
    n = d.n8
    ref_m, _ = code_diff(s32["m_codes"], s64["m_codes"])
    ref_v, _ = code_diff(s32["v_codes"], s64["v_codes"])
    ref_p = float((s32["p"].double() - s64["p"]).norm() / s64["p"].norm())
    dm, wm = code_diff(d.mc.cpu(), s32["m_codes"])
    dv, wv = code_diff(d.vc.cpu(), s32["v_codes"])
    e_p = float((d.p.cpu().double() - s32["p"].double()).norm() / s32["p"].double().norm())
    e_am = float((d.ma.cpu() - s32["m_absmax"]).abs().max() / s32["m_absmax"].max())
    e_av = float((d.va.cpu() - s32["v_absmax"]).abs().max() / s32["v_absmax"].max())
    print(f"steps {steps} clipped {clipped}: kernel vs f32 restatement: {dm} + {dv} of 2 x {n} codes differ (max distance {max(wm, wv)}), parameter "
          f"rel-L2 {e_p:.2e}, absmax rel err {e_am:.1e} / {e_av:.1e}; f32 vs f64 restatement: {ref_m} + {ref_v} codes, parameter rel-L2 {ref_p:.2e}")
    assert (ref_m + ref_v) < 0.01 * 2 * n
    assert (dm + dv) <= 2 * (ref_m + ref_v)
    assert max(wm, wv) <= 1
    assert e_p <= 2 * ref_p
    assert e_am <= 1e-6 and e_av <= 1e-6
    # untouched padding, refreshed f16 copy
    assert torch.equal(d.p.cpu()[~covered], p[~covered])
    assert torch.equal(d.half.cpu()[covered], d.p.cpu().half()[covered])


def test_quantisation_bound():
    """One step from zero state: the stored moments are the fp32 ones rounded to the nearest code of their block, so per element
    |map[code] x absmax - moment| <= absmax x (largest half-gap of the map).  The bound is met with EQUALITY by the block's most
    negative first moment (x = -1 against the map's lowest code -0.99297: a distance of 0.9 / 128, which is also the largest half-gap), so
    the comparison itself is evaluated in f64 with 4 f32 ulps of absmax for the roundings of the f32 moment and of the stored product."""
    E = Engine("cuda:0")
    layout, numel, p, grads = _ragged_case(seed=3)
    d = _Dev(E, layout, p)
    idx, cidx, bid = expand_blocks(d.table)
    st = fresh_state(p, d.table, d.n8)
    mi, vi = restate_step(st, grads[0], (idx, cidx, bid), 1, **HYPER)
    d.step(grads[0].to(E.device), 1)
    S, U = optim8.dynamic_map(True), optim8.dynamic_map(False)
    for name, cmap, codes, absmax, want in (("m", S, d.mc, d.ma, mi), ("v", U, d.vc, d.va, vi)):
        cmap = cmap.double()
        half_gap = float((cmap[1:] - cmap[:-1]).max()) / 2.0
        am = absmax.cpu().double()[bid]
        err = (cmap[codes.cpu()[cidx].long()] * am - want.double()).abs()
        worst = float((err / am).max())
        print(f"{name}: largest half-gap {half_gap:.7f}, worst |dequant - fp32| / absmax {worst:.7f}")
        assert bool((err <= am * (half_gap + 4 * 2.0 ** -23)).all())
        assert worst > 0.1 * half_gap  # (the bound is not vacuous: some element sits in a wide gap)


def test_skip_and_zero_grad():
    E = Engine("cuda:0")
    layout, numel, p, grads = _ragged_case(seed=5)
    d = _Dev(E, layout, p)
    covered = torch.zeros(numel, dtype=torch.bool)
    covered[expand_blocks(d.table)[0]] = True
    d.step(grads[0].to(E.device), 1)
    before = [t.clone() for t in (d.p, d.half, d.mc, d.vc, d.ma, d.va)]
    g = grads[1].clone()
    g[::1000] = float("inf")
    g[7::5000] = float("nan")
    g = g.to(E.device)
    d.step(g, 2, torch.tensor([0.0, float("inf"), 1.0], dtype=F32, device=E.device), 1.0)
    for a, b in zip(before, (d.p, d.half, d.mc, d.vc, d.ma, d.va)):
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.uint8 else a, b.view(torch.uint8) if b.dtype != torch.uint8 else b)
    assert float(g.cpu()[covered].abs().max()) == 0.0
    # zero_grad off: the gradient survives an applied step
    g2 = grads[2].to(E.device)
    d.step(g2, 2, None, 1.0, zero_grad=False)
    assert torch.equal(g2.cpu(), grads[2]) and not torch.equal(d.p, before[0])


# ------------------------------------------------------------------------------------------------------------------ the trainer
def _setup(B=2, seed=0):
    ucfg, ccfg = FAM["unet"], FAM["controlnet"]
    usd = weights.round_to(weights.synth_state_dict(schema.unet_schema(ucfg), 1), torch.float16)
    csd = weights.round_to(weights.synth_state_dict(schema.controlnet_schema(ccfg), 2), torch.float16)
    g = torch.Generator().manual_seed(seed)
    lat = q16(torch.randn(B, 4, 32, 32, generator=g))
    noise = q16(torch.randn(B, 4, 32, 32, generator=g))
    ctx = q16(torch.randn(B, 77, 128, generator=g))
    cond = q16(torch.rand(B, 3, 256, 256, generator=g))
    t = torch.tensor([801, 399][:B])
    sa, s1 = DDPMScheduler().add_noise_coeffs(t)
    dev = lambda x: x.cuda()  # noqa: E731
    args = (dev(nchw_to_nhwc(lat, 8).half()), dev(nchw_to_nhwc(noise, 8).half()), dev(t.float()), dev(sa), dev(s1), dev(ctx.half()),
            dev(nchw_to_nhwc(cond, 8).half()))
    return ucfg, ccfg, pack_state_dict(usd, "cuda"), csd, args


def _counts(layout):
    """(n8, n_blocks, n_small) straight from a layout: parameters of >= 4096 elements are quantised in blocks of 256."""
    n8 = nb = ns = 0
    for _, (off, shape) in layout.items():
        n = 1
        for s in shape:
            n *= s
        if n >= 4096:
            n8, nb = n8 + n, nb + (n + 255) // 256
        else:
            ns += n
    return n8, nb, ns


def test_state_size():
    ucfg, ccfg, unet_W, csd, args = _setup()
    E = Engine("cuda:0")
    a = ControlNetTrainer(E, ucfg, ccfg, unet_W, csd, use_8bit_adam=True)
    n8, nb, ns = _counts(a.cn.layout)
    assert a.optimizer_state_bytes() == 2 * n8 + 8 * nb + 8 * ns
    assert not hasattr(a.cn, "exp_avg") and not hasattr(a.cn, "exp_avg_sq")  # never both forms
    b = ControlNetTrainer(E, ucfg, ccfg, unet_W, csd)
    assert b.optimizer_state_bytes() == 8 * b.cn.numel and not hasattr(b.cn, "m_codes")
    print(f"tiny ControlNet: optimizer state {a.optimizer_state_bytes()} bytes 8-bit vs {b.optimizer_state_bytes()} fp32 "
          f"({a.optimizer_state_bytes() / b.optimizer_state_bytes():.4f})")


def test_close_to_fp32_adamw():
    """N = 3 steps of the tiny trainer on one batch, lr 1e-4, with and without the flag.  Yardstick: on the gradients the fp32 run recorded,
    the CPU restatement of the 8-bit step against torch.optim.AdamW (f64); the final loss of either CPU result is the trainer's forward on
    those parameters.  The 8-bit run's distance from the fp32 run (parameter rel-L2, final loss) must stay within 2 x that."""
    N, lr, S = 3, 1e-4, 4096.0
    ucfg, ccfg, unet_W, csd, args = _setup()
    hyper = dict(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)

    def run(flag, record=None):
        tr = ControlNetTrainer(Engine("cuda:0"), ucfg, ccfg, unet_W, csd, lr=lr, loss_scale=S, use_8bit_adam=flag)
        p0 = tr.cn.master.cpu().clone()
        for _ in range(N):
            tr.forward_backward(*args)
            g = tr.cn.grad.cpu().clone()
            tr.optimizer_step()
            assert tr.update_scale()
            if record is not None:
                record.append((g, float(tr._clip[0].cpu())))
        final = float(tr.forward_backward(*args).cpu())
        tr.cn.zero_grad()
        return tr, p0, final

    rec = []
    t32, p0, l32 = run(False, rec)
    t8, _, l8 = run(True)
    m32, m8 = t32.cn.master.cpu(), t8.cn.master.cpu()

    t0 = time.time()
    w = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([w], lr=lr, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    table, small, n8, _ = optim8.build_block_table(t32.cn.layout)
    ex = expand_blocks(table)
    st = fresh_state(p0, table, n8)
    for k, (g, coef) in enumerate(rec):
        w.grad = g.double() * (coef / S)
        opt.step()
        restate_step(st, g, ex, k + 1, coef, 1.0 / S, **hyper)
    p_adamw = w.detach().float()
    p_8 = p_adamw.clone()  # the small parameters keep fp32 moments: plain AdamW
    p_8[ex[0]] = st["p"][ex[0]]
    cpu_s = time.time() - t0

    def loss_of(pvec):
        t32.cn.master.copy_(pvec)
        t32.cn.sync_half()
        out = float(t32.forward_backward(*args).cpu())
        t32.cn.zero_grad()
        return out
    l_adamw, l_8cpu = loss_of(p_adamw), loss_of(p_8)
    e_gpu, e_ref = rel_l2(m8, m32), rel_l2(p_8, p_adamw)
    e_same = rel_l2(m32, p_adamw)
    d_gpu, d_ref = abs(l8 - l32), abs(l_8cpu - l_adamw)
    print(f"{N} steps, lr {lr}: parameters 8-bit vs fp32 run rel-L2 {e_gpu:.3e}; CPU restatement vs torch AdamW {e_ref:.3e} (fp32 run vs torch AdamW "
          f"{e_same:.1e}); final loss fp32 {l32:.7f} 8-bit {l8:.7f} |d| {d_gpu:.3e}; CPU results: AdamW {l_adamw:.7f} 8-bit {l_8cpu:.7f} |d| {d_ref:.3e}; "
          f"CPU restatement took {cpu_s:.1f} s")
    assert cpu_s < 60
    assert e_gpu <= 2 * e_ref
    assert d_gpu <= 2 * d_ref


def test_resume_is_bit_exact_and_kinds_do_not_mix(tmp_path):
    ucfg, ccfg, unet_W, csd, args = _setup()
    mk = lambda flag: ControlNetTrainer(Engine("cuda:0"), ucfg, ccfg, unet_W, csd, lr=1e-4, loss_scale=4096.0, use_8bit_adam=flag)  # noqa: E731
    a = mk(True)
    for _ in range(2):
        a.step(*args)
    ckpt = a.save_state(str(tmp_path / "q"), 2)
    la = float(a.step(*args).cpu())
    b = mk(True)
    assert b.load_state(ckpt) == 2 and b.opt_step == 2
    for k, t in a.cn.optimizer_state().items():
        assert t.numel() > 0, k
    lb = float(b.step(*args).cpu())
    assert la == lb
    la2, lb2 = float(a.step(*args).cpu()), float(b.step(*args).cpu())  # (the loss after the resumed optimizer step)
    assert la2 == lb2
    assert torch.equal(a.cn.master, b.cn.master)
    for (k, x), y in zip(a.cn.optimizer_state().items(), b.cn.optimizer_state().values()):
        assert torch.equal(x, y), k
    from safetensors import safe_open
    with safe_open(str(tmp_path / "q" / "checkpoint-2" / "optimizer_flat.safetensors"), "pt") as f:
        assert f.metadata()["optimizer"] == "adamw8bit"
        assert set(f.keys()) == {"m_codes", "v_codes", "m_absmax", "v_absmax", "exp_avg_small", "exp_avg_sq_small", "scalars"}
        assert f.get_tensor("m_codes").dtype == torch.uint8
    # the other kind is refused, both ways, by name
    c = mk(False)
    m_before = c.cn.master.clone()
    with pytest.raises(ValueError, match="adamw8bit") as ei:
        c.load_state(ckpt)
    assert "'adamw'" in str(ei.value) and torch.equal(c.cn.master, m_before)
    c.step(*args)
    ckpt32 = c.save_state(str(tmp_path / "f"), 1)
    with pytest.raises(ValueError, match="adamw8bit") as ei:
        mk(True).load_state(ckpt32)
    assert "'adamw'" in str(ei.value)
    assert mk(False).load_state(ckpt32) == 1  # fp32 checkpoints (no marker in the file) load into an fp32 trainer as before


def test_pix2pix_ema_with_8bit_adam():
    from genima_amd.pix2pix import InstructPix2PixTrainer, ema_decay_at, expand_conv_in

    ucfg = configs.family("tiny-pix2pix")["unet"]
    usd = weights.round_to(expand_conv_in(weights.synth_state_dict(schema.unet_schema(dict(ucfg, in_channels=4)), 1), 8), torch.float16)
    g = torch.Generator().manual_seed(0)
    lat, noise = q16(torch.randn(2, 4, 32, 32, generator=g)), q16(torch.randn(2, 4, 32, 32, generator=g))
    ctx, emb = q16(torch.randn(2, 77, 128, generator=g)), q16(torch.randn(2, 4, 32, 32, generator=g))
    t = torch.tensor([801, 399])
    sa, s1 = DDPMScheduler().add_noise_coeffs(t)
    dev = lambda x: x.cuda()  # noqa: E731
    args = (dev(nchw_to_nhwc(lat, 8).half()), dev(nchw_to_nhwc(noise, 8).half()), dev(t.float()), dev(sa), dev(s1), dev(ctx.half()),
            dev(nchw_to_nhwc(emb, 8).half()))
    tr = InstructPix2PixTrainer(Engine("cuda:0"), ucfg, usd, lr=1e-4, loss_scale=4096.0, use_ema=True, use_8bit_adam=True)
    assert tr.cn.use_8bit_adam and tr.cn.m_codes.dtype == torch.uint8
    m0 = tr.cn.master.clone()
    shadow = tr.ema.clone()
    for k in (1, 2):
        loss = float(tr.step(*args).cpu())
        assert loss == loss and tr.opt_step == k
        omd = torch.tensor(1.0 - ema_decay_at(k), dtype=F32)
        want = shadow.cpu() - omd * (shadow.cpu() - tr.cn.master.cpu())  # EMAModel.step on the fp32 master, whatever form the moments take
        assert torch.allclose(tr.ema.cpu(), want, rtol=0, atol=1e-7), k
        shadow = tr.ema.clone()
    assert not torch.equal(tr.cn.master, m0) and int(tr.cn.m_codes.max()) > 0 and float(tr.cn.m_absmax.min()) >= 0
