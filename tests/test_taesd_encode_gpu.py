"""-m gpu: the TAESD encoder on the device -- the fused AutoencoderTinyBlock (gn_tiny_block, csrc/taesd.hip), graphs.emit_taesd_encode /
AutoencoderTiny.encode, and the trainer's ``tiny_vae`` switch (the reference's --tiny_vae, diffusion/train_controlnet_genima.py:1324-1327),
against the fp32 restatement of diffusers' EncoderTiny in test_taesd_encode_cpu.py.

Tolerances: one block keeps two intermediates in f16 (as the three-launch route stores them): rel-L2 <= 1e-3 and max |diff| <= 4 f16 ulps of
the output's largest magnitude; the 15-layer encoder stores 25 f16 intermediates: rel-L2 <= 2e-3."""
import numpy as np
import pytest
import torch

from genima_amd import configs, graphs, packing, schema, validation, weights
from genima_amd.engine import Engine
from genima_amd.host import AutoencoderTiny, CLIPTextModel, ControlNetModel, UNet2DConditionModel, nchw_to_nhwc
from genima_amd.packing import pack_state_dict
from genima_amd.scheduler import DDPMScheduler
from genima_amd.training import ControlNetTrainer
from test_taesd_encode_cpu import encoder_tiny_ref, tiny_block_ref
from util import q16, rel_l2

pytestmark = pytest.mark.gpu

CFG = configs.TAESD
BLOCK = "encoder.layers.3"


def _taesd_sd(seed=7):
    return weights.round_to(weights.synth_state_dict(schema.taesd_schema(CFG), seed), torch.float16)


def _block_inputs(sd, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = q16(torch.randn(B, 64, H, W, generator=g))  # negative values: the first ReLU clips
    ks = (0, 2, 4)
    ws = [packing.pack_conv_weight(sd[f"{BLOCK}.conv.{k}.weight"]).cuda() for k in ks]
    bs = [sd[f"{BLOCK}.conv.{k}.bias"].half().cuda() for k in ks]
    return x, ws, bs


def _ulp16(v: float) -> float:
    return float(np.spacing(np.float16(v)))


@pytest.mark.parametrize("B,H,W", [(b, h, w) for b in (1, 3) for (h, w) in ((16, 16), (17, 23), (64, 64), (256, 256))] + [(1, 512, 512)])
def test_fused_block_vs_fp32_and_three_launch_route(B, H, W):
    sd = _taesd_sd()
    x, ws, bs = _block_inputs(sd, B, H, W, seed=H * 31 + W + B)
    E = Engine("cuda:0")
    assert E.tiny_block_supported(torch.empty(B, H, W, 64))
    x8 = nchw_to_nhwc(x, 64).half().cuda().contiguous()
    out = E.tiny_block(x8, ws, bs)
    Wp = {f"{BLOCK}.conv.{k}.{t}": (ws[i] if t == "weight" else bs[i]) for i, k in enumerate((0, 2, 4)) for t in ("weight", "bias")}
    three = graphs._emit_tiny_block(E, Wp, BLOCK, x8)
    torch.cuda.synchronize()
    got = out.permute(0, 3, 1, 2).float().cpu()
    with torch.no_grad():
        ref = tiny_block_ref(x, sd, BLOCK)
    e = rel_l2(got, ref)
    dmax = float((got - ref).abs().max())
    bar = 4 * _ulp16(float(ref.abs().max()))
    e3 = rel_l2(got, three.permute(0, 3, 1, 2).float().cpu())
    print(f"B {B} {H}x{W}: rel-L2 vs fp32 {e:.2e}, max|d| {dmax:.3e} (bar {bar:.3e}); vs three-launch route {e3:.2e}")
    assert float((ref > 0).float().mean()) < 0.9  # the ReLUs clip
    assert e <= 1e-3 and dmax <= bar
    assert e3 <= 1e-3


def test_encoder_full_width_512(monkeypatch):
    sd = _taesd_sd(11)
    vae = AutoencoderTiny(CFG, sd).to("cuda")
    B, R = 2, 512
    x = q16(torch.rand(B, 3, R, R, generator=torch.Generator().manual_seed(4)) * 2 - 1)
    lat = vae.encode(x).latents
    assert tuple(lat.shape) == (B, 4, R // 8, R // 8) and lat.dtype == torch.float16
    (lat_t,) = vae.encode(x, return_dict=False)
    assert torch.equal(lat, lat_t)
    with torch.no_grad():
        ref = encoder_tiny_ref(x, sd, CFG)
    e = rel_l2(lat.float().cpu(), ref)
    print(f"AutoencoderTiny.encode B {B} {R}^2 vs fp32 EncoderTiny: rel-L2 {e:.2e}")
    assert e <= 2e-3

    # the fused route (GN_TINY_BLOCK=1): one launch per block; recorded and replayed == eager, bit for bit
    monkeypatch.setenv("GN_TINY_BLOCK", "1")
    E = Engine("cuda:0", record=True)
    x8 = nchw_to_nhwc(x.cuda().half(), 8)
    rec = graphs.emit_taesd_encode(E, vae.W, CFG, x8)
    n_fused = sum(1 for m in E.meta if m["kind"] == "tiny_block")
    assert n_fused == sum(CFG["num_encoder_blocks"]) == 10
    E.run()
    eager = graphs.emit_taesd_encode(Engine("cuda:0"), vae.W, CFG, x8)
    torch.cuda.synchronize()
    assert float(eager[..., 4:].abs().max()) == 0.0  # the lat8 convention: channels 4..7 exactly zero
    assert torch.equal(rec, eager)
    e_f = rel_l2(eager[..., :4].permute(0, 3, 1, 2).float().cpu(), ref)
    print(f"fused route vs fp32: rel-L2 {e_f:.2e}")
    assert e_f <= 2e-3
    assert rel_l2(eager[..., :4].permute(0, 3, 1, 2).float().cpu(), lat.float().cpu()) <= 1e-3


def test_encoder_default_route_is_three_launches(monkeypatch):
    """default (GN_TINY_BLOCK unset): every block as three conv launches; the fused route agrees within the block bar."""
    sd = _taesd_sd(12)
    vae = AutoencoderTiny(CFG, sd).to("cuda")
    x8 = nchw_to_nhwc(q16(torch.rand(1, 3, 128, 96, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda().half(), 8)
    monkeypatch.delenv("GN_TINY_BLOCK", raising=False)
    E = Engine("cuda:0", record=True)
    three = graphs.emit_taesd_encode(E, vae.W, CFG, x8)
    assert not any(m["kind"] == "tiny_block" for m in E.meta)
    E.run()
    monkeypatch.setenv("GN_TINY_BLOCK", "1")
    fused = graphs.emit_taesd_encode(Engine("cuda:0"), vae.W, CFG, x8)
    torch.cuda.synchronize()
    assert rel_l2(fused.float().cpu(), three.float().cpu()) <= 2e-3


def _tiny_trainer(vae, tiny_vae, seed=5, accum=1):
    fam = configs.family("tiny")
    synth = lambda sch, s: weights.round_to(weights.synth_state_dict(sch, s), torch.float16)  # noqa: E731
    tr = ControlNetTrainer(Engine("cuda:0"), fam["unet"], fam["controlnet"], pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), "cuda"),
                           synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-4, loss_scale=4096.0, gradient_accumulation_steps=accum)
    text_W = pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), "cuda")
    if tiny_vae:
        tr.attach_frozen(CFG, vae.W, fam["text"], text_W, DDPMScheduler(), seed=seed, tiny_vae=True)
    else:
        tr.attach_frozen(fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"], text_W, DDPMScheduler(),
                         seed=seed)
    return tr


def _batch(B=2, R=256):
    g = torch.Generator().manual_seed(9)
    return dict(pixel_values=q16(torch.rand(B, 3, R, R, generator=g) * 2 - 1), conditioning_pixel_values=q16(torch.rand(B, 3, R, R, generator=g)),
                input_ids=torch.randint(0, 1000, (B, 77), generator=g))


def test_trainer_tiny_vae():
    vae = AutoencoderTiny(CFG, _taesd_sd(13)).to("cuda")
    batch = _batch()
    dev = torch.device("cuda", torch.cuda.current_device())

    tr = _tiny_trainer(vae, True)
    lat8, noise8, t, sa, s1, ctx, cond8, added = tr._front(batch)
    x8 = nchw_to_nhwc(batch["pixel_values"].to(dev, torch.float16), 8)
    ref = graphs.emit_taesd_encode(tr.E, vae.W, CFG, x8)
    assert torch.equal(lat8, ref)  # encode(...).latents: no scaling factor, no posterior sample
    shape = tuple(lat8.shape[:-1]) + (4,)
    first = torch.randn(shape, generator=torch.Generator(dev).manual_seed(5), device=dev, dtype=torch.float32).to(torch.float16)
    assert torch.equal(noise8[..., :4], first)  # the noise is the generator's FIRST draw: nothing drawn for the latents
    assert float(noise8[..., 4:].abs().max()) == 0.0

    # one train step (accumulating: the gradient stays in the flat buffer) against forward_backward on the same latents / noise / timesteps
    tr_a = _tiny_trainer(vae, True, accum=2)
    loss = float(tr_a.train_step(batch).cpu())
    assert np.isfinite(loss)
    tr_b = _tiny_trainer(vae, True, accum=2)
    f = tr_b._front(batch)
    loss_b = float(tr_b.forward_backward(f[0], f[1], f[2].to(dev, torch.float32), f[3].to(dev), f[4].to(dev), f[5], f[6]).cpu())
    torch.cuda.synchronize()
    assert loss == loss_b
    assert torch.equal(tr_a.cn.grad, tr_b.cn.grad)

    # the default path still draws the posterior sample first: its noise is NOT the generator's first draw
    tr_kl = _tiny_trainer(None, False)
    _, noise_kl, *_ = tr_kl._front(batch)
    assert not torch.equal(noise_kl[..., :4], first)
    second = torch.Generator(dev).manual_seed(5)
    torch.randn(shape, generator=second, device=dev, dtype=torch.float32)
    assert torch.equal(noise_kl[..., :4], torch.randn(shape, generator=second, device=dev, dtype=torch.float32).to(torch.float16))


def test_log_validation_with_tiny_vae():
    fam = configs.family("tiny")
    r16 = lambda sd: weights.round_to(sd, torch.float16)  # noqa: E731
    vae = AutoencoderTiny(CFG, _taesd_sd(14))
    text = CLIPTextModel(fam["text"], r16(weights.synth_state_dict(schema.clip_text_schema(fam["text"]), 14)))
    unet = UNet2DConditionModel(fam["unet"], r16(weights.synth_state_dict(schema.unet_schema(fam["unet"]), 11)))
    cn = ControlNetModel(fam["controlnet"], r16(weights.synth_state_dict(schema.controlnet_schema(fam["controlnet"]), 12)))
    pipe = validation.validation_pipeline(vae, text, None, unet, cn, "ddpm")
    R = 128
    from PIL import Image

    rgb = Image.fromarray(weights.counter_bytes(3, "cond", R * R * 3).reshape(R, R, 3))
    gt = Image.fromarray(weights.counter_bytes(4, "gt", R * R * 3).reshape(R, R, 3))
    logs = validation.log_validation(pipe, rgb, gt, "open the box", seed=3)
    out = np.asarray(logs[0]["images"][0])
    assert out.dtype == np.uint8 and out.shape == (R, R, 3)
    assert np.isfinite(logs[0]["mse"])
