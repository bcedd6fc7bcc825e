"""-m gpu: ``ControlNetTrainer.attach_frozen(sphere_loss_weight=)`` on the tiny family (the sizes of tests/test_training_gpu.py): the weighted
step against torch autograd over the CPU oracle, the default path untouched, the empty mask equal to the unweighted step, the front-stream
overlap, the mask carried through the shared augmentations, gradient accumulation, and the refusal under a replayed step.

Bars of the autograd comparison: tests/test_training_gpu.py's own (loss 2e-3 relative, flat gradient rel-L2 <= min(1e-2, 1.5 e_ref + 2e-3),
no dead tensor).  Loss bound of the empty-mask comparison: tests/test_sphere_loss_kernels_gpu.py's (pixels * C + 8) 2^-24."""
import functools

import numpy as np
import pytest
import torch

from genima_amd import augment, configs, schema, weights
from genima_amd import train_ops as T
from genima_amd.engine import Engine
from genima_amd.host import nchw_to_nhwc
from genima_amd.packing import pack_state_dict
from genima_amd.scheduler import DDPMScheduler
from genima_amd.training import ControlNetTrainer
from oracle import sd_torch as O
from oracle import train_torch as OT
from util import q16, rel_l2
import sphere_loss_ref as R

pytestmark = pytest.mark.gpu

FAM = configs.family("tiny")
SEED, LAM, RES, LAT = 5, 4.0, 256, 32


def _synth(sch, s):
    return weights.round_to(weights.synth_state_dict(sch, s), torch.float16)


@functools.lru_cache(maxsize=None)
def _state_dicts():
    return _synth(schema.unet_schema(FAM["unet"]), 1), _synth(schema.controlnet_schema(FAM["controlnet"]), 2)


@functools.lru_cache(maxsize=None)
def _grid_batch(B=2):
    """A byte-grid batch at the tiny family's resolution, its reference mask and the share of marked pixels (asserted real)."""
    target, cond = R.byte_grid_pair(B, RES, RES, seed=11)
    mask = R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30)
    share = R.marked_share(mask)
    assert 0.01 <= share <= 0.5, share
    return target, cond, mask, share


def _batch(B=2):
    target, cond, _, _ = _grid_batch(B)
    g = torch.Generator().manual_seed(9)
    return dict(pixel_values=torch.from_numpy(target), conditioning_pixel_values=torch.from_numpy(cond), input_ids=torch.randint(0, 1000, (B, 77), generator=g))


def _trainer(weight=0.0, threshold=30, augmentations=None, **kw):
    usd, csd = _state_dicts()
    tr = ControlNetTrainer(Engine("cuda:0"), FAM["unet"], FAM["controlnet"], pack_state_dict(usd, "cuda"), csd, lr=1e-4, loss_scale=4096.0, **kw)
    tr.attach_frozen(FAM["vae"], pack_state_dict(_synth(schema.vae_schema(FAM["vae"]), 3), "cuda"), FAM["text"],
                     pack_state_dict(_synth(schema.clip_text_schema(FAM["text"]), 4), "cuda"), DDPMScheduler(), seed=SEED, augmentations=augmentations,
                     sphere_loss_weight=weight, sphere_change_threshold=threshold)
    return tr


def _flat(packed, layout):
    return torch.cat([packed[n].reshape(-1).float().cpu() for n in layout])


def _weighted_oracle(usd, csd, ucfg, ccfg, lat, noise, t, sa, s1, ctx, cond, w, wsum, q=O._id):
    """oracle.train_torch.train_forward_backward's step body with the weighted mean sum(w (pred - target)^2) / (C sum w) as the loss."""
    params = {k: v.detach().clone().requires_grad_(True) for k, v in csd.items()}
    noisy = q(sa.view(-1, 1, 1, 1) * lat + s1.view(-1, 1, 1, 1) * noise)
    down, mid = O.controlnet_forward(params, ccfg, noisy, t, ctx, cond, q=q)
    pred = O.unet_forward(usd, ucfg, noisy, t, ctx, down, mid, q=q)
    loss = (w * (pred.float() - noise.float()) ** 2).sum() / (pred.shape[1] * wsum)
    loss.backward()
    return loss.detach(), {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in params.items()}


def test_weighted_step_against_autograd():
    ucfg, ccfg = FAM["unet"], FAM["controlnet"]
    usd, csd = _state_dicts()
    B = 2
    g = torch.Generator().manual_seed(0)
    lat, noise = q16(torch.randn(B, 4, LAT, LAT, generator=g)), q16(torch.randn(B, 4, LAT, LAT, generator=g))
    ctx, cond = q16(torch.randn(B, 77, 128, generator=g)), q16(torch.rand(B, 3, RES, RES, generator=g))
    t = torch.tensor([801, 399])
    sa, s1 = DDPMScheduler().add_noise_coeffs(t)
    _, _, mask, share = _grid_batch(B)
    w_np, _, wsum = R.loss_weight_pool(mask, LAT, LAT, LAM)  # w from the reference
    assert w_np.max() > 1.0 and w_np.min() == 1.0

    S = 4096.0
    tr = ControlNetTrainer(Engine("cuda:0"), ucfg, ccfg, pack_state_dict(usd, "cuda"), csd, lr=1e-4, loss_scale=S)
    dev = lambda x: x.cuda()  # noqa: E731
    args = (dev(nchw_to_nhwc(lat, 8).half()), dev(nchw_to_nhwc(noise, 8).half()), dev(t.float()), dev(sa), dev(s1), dev(ctx.half()),
            dev(nchw_to_nhwc(cond, 8).half()))
    lw = (torch.from_numpy(w_np).cuda(), torch.tensor([float(wsum)], dtype=torch.float64, device="cuda"))
    loss = float(tr.forward_backward(*args, loss_weight=lw).cpu())
    layout = list(tr.cn.layout)
    g_hip = {n: (tr.cn.G[n].float() / S).cpu() for n in layout}

    w = torch.from_numpy(w_np).view(B, 1, LAT, LAT)
    tf = t.float()
    l32, g32 = _weighted_oracle(usd, csd, ucfg, ccfg, lat, noise, tf, sa, s1, ctx, cond, w, float(wsum))
    l16, g16 = _weighted_oracle(usd, csd, ucfg, ccfg, lat, noise, tf, sa, s1, ctx, cond, w, float(wsum), q=q16)
    _, g_plain, _ = OT.train_forward_backward(usd, csd, ucfg, ccfg, lat, noise, tf, sa, s1, ctx, cond)
    print(f"marked share {share:.4f}; loss hip {loss:.6f}  oracle fp32 {float(l32):.6f}  oracle f16-storage {float(l16):.6f}")
    assert abs(loss - float(l32)) <= 2e-3 * float(l32)
    P32, P16, PP = (pack_state_dict(x, "cpu", dtype=torch.float32) for x in (g32, g16, g_plain))
    f_hip, f32_, f16_, f_plain = _flat(g_hip, layout), _flat(P32, layout), _flat(P16, layout), _flat(PP, layout)
    gnorm = float(f32_.norm())
    e_all, e_ref, e_plain = rel_l2(f_hip, f32_), rel_l2(f16_, f32_), rel_l2(f_plain, f32_)
    bar = min(1e-2, 1.5 * e_ref + 2e-3)
    print(f"flat gradient: |g| = {gnorm:.4e}, rel-L2 vs fp32 oracle {e_all:.2e} (f16-storage oracle {e_ref:.2e}, bar {bar:.2e}); "
          f"the unweighted gradient is {e_plain:.2e} away")
    assert torch.isfinite(f_hip).all()
    assert e_all <= bar
    assert e_plain > bar, "the weighted gradient must differ from the unweighted one by more than the bar, or this test shows nothing"
    dead = [n for n in layout if float(P32[n].abs().max()) > 1e-7 * gnorm and float(g_hip[n].abs().max()) == 0.0]
    assert not dead, dead


def test_default_path_calls_none_of_the_new_ops(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the sphere-loss ops must not run with sphere_loss_weight == 0")
    for name in ("mse_loss_weighted", "change_mask", "loss_weight_pool"):
        monkeypatch.setattr(T, name, boom)
    tr = _trainer(0.0)
    out = tr._front(_batch())
    assert len(out) == 8  # the front's outputs as they were
    loss = float(tr.train_step(_batch()))
    assert loss == loss and "sphere_fraction" not in tr.last


def test_empty_mask_is_the_unweighted_step():
    """A threshold nothing can exceed (2 * 765): weight 1 everywhere, wsum = pixels -- the weight-0 trainer's gradient bit for bit."""
    a, b = _trainer(LAM, threshold=765 * 2, gradient_accumulation_steps=2), _trainer(0.0, gradient_accumulation_steps=2)
    la, lb = float(a.train_step(_batch())), float(b.train_step(_batch()))  # the first micro-batch: the gradient stays in the flat buffer
    assert not a.sync_gradients and not b.sync_gradients
    assert float(a.last["sphere_fraction"]) == 0.0
    pixels, C = 2 * LAT * LAT, 4
    print(f"empty mask: loss {la!r} vs unweighted {lb!r}, bound {(pixels * C + 8) * 2.0 ** -24 * lb:.3e}")
    assert abs(la - lb) <= (pixels * C + 8) * 2.0 ** -24 * lb
    assert float(b.cn.grad.abs().max()) > 0.0 and torch.equal(a.cn.grad, b.cn.grad)


def test_overlapped_front_equals_the_serial_front(monkeypatch):
    """GN_FRONT_SIDE=0 (mask, pooling and encode on the main stream) and the default give the same loss bits with weight 4."""
    _, _, _, share = _grid_batch()

    def run(serial):
        if serial:
            monkeypatch.setenv("GN_FRONT_SIDE", "0")
        else:
            monkeypatch.delenv("GN_FRONT_SIDE", raising=False)
        tr = _trainer(LAM)
        losses = [float(tr.train_step(_batch())) for _ in range(3)]
        return losses, float(tr.last["sphere_fraction"]), tr.cn.master.clone()
    l0, f0, m0 = run(True)
    l1, f1, m1 = run(False)
    print(f"weighted losses {l1}; sphere_fraction {f1:.5f} (reference share {share:.5f})")
    assert l0 == l1 and all(x == x for x in l0) and torch.equal(m0, m1)
    assert f0 == f1 and abs(f1 - share) <= 1e-6
    plain = float(_trainer(0.0).train_step(_batch()))
    assert plain != l1[0]  # same seed and batch: the weight changes the loss


def test_mask_follows_the_shared_augmentations():
    E = Engine("cuda:0")
    augs = "affine,crop"
    target, cond, mask, _ = _grid_batch()
    x8, c8, m8 = torch.from_numpy(target).cuda(), torch.from_numpy(cond).cuda(), torch.from_numpy(mask).cuda()
    g0, g1, g2 = (torch.Generator().manual_seed(SEED) for _ in range(3))
    plain = augment.augment_data(E, augs, dict(pixel_values=x8, conditioning_pixel_values=c8), g0)
    both = augment.augment_data(E, augs, dict(pixel_values=x8, conditioning_pixel_values=c8), g1, extra=dict(sphere_mask=m8))
    assert torch.equal(plain["pixel_values"], both["pixel_values"]) and torch.equal(plain["conditioning_pixel_values"], both["conditioning_pixel_values"])
    assert torch.equal(g0.get_state(), g1.get_state())  # the generator is consumed identically
    draws = augment.draw_augmentations(augment.parse_augmentations(augs), RES, g2)
    want = augment.reflect_pad_crop(E, augment.affine(E, m8, augment.affine_inverse_matrix(*draws["affine"])), *draws["crop"])
    assert torch.equal(both["sphere_mask"], want) and not torch.equal(want, m8)
    assert 0.0 < float((want[..., 0] != 0).float().mean()) < 1.0 and not bool(want[..., 1:].any())
    assert set(plain) == {"pixel_values", "conditioning_pixel_values"}
    with pytest.raises(ValueError):
        augment.augment_data(E, augs, dict(pixel_values=x8, conditioning_pixel_values=c8), g0, extra=dict(sphere_mask=m8[:, :128]))

    tr = _trainer(LAM, augmentations=augs)
    loss = float(tr.train_step(_batch()))
    frac = float(tr.last["sphere_fraction"])
    print(f"weighted step with {augs}: loss {loss!r}, sphere_fraction {frac:.5f}")
    assert np.isfinite(loss) and 0.0 < frac < 1.0


def test_accumulation_applies_one_optimizer_step_per_two_micro_batches():
    tr = _trainer(LAM, gradient_accumulation_steps=2)
    losses, synced = [], []
    for _ in range(4):
        losses.append(float(tr.train_step(_batch())))
        synced.append(tr.sync_gradients)
    assert synced == [False, True, False, True] and tr.opt_step == 2
    assert all(np.isfinite(x) for x in losses)


def test_replayed_step_refuses_the_weighted_loss():
    usd, csd = _state_dicts()
    tr = ControlNetTrainer(Engine("cuda:0"), FAM["unet"], FAM["controlnet"], pack_state_dict(usd, "cuda"), csd, hip_graph=True)
    with pytest.raises(ValueError):
        tr.attach_frozen(None, None, None, None, DDPMScheduler(), sphere_loss_weight=LAM)
    with pytest.raises(ValueError):
        tr.step(*([None] * 7), loss_weight=(None, None))
