"""-m gpu: the ACT ElasticTransform displacement field built on the device (gn_elastic_field, csrc/act_train.hip) against the f64 torch
restatement of tests/elastic_ref.py, evaluated from the same f32 noise and f32 taps.

Bound (derived, not measured): max |device - ref64| <= (alpha / 2) * (2k + 8) * 2^-24 px.  Each output is alpha / 2 times a double convex
combination of values in (-1, 1), evaluated as 2k f32 FMAs plus one f32 store between the passes, the scale multiply and the final
rounding; 4.05e-4 px at k = 81.  The measured maxima are printed; they sit orders of magnitude below the bound."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import elastic_ref as ER

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ALPHA = 80.0
# H, W, sigma, k
CASES = [
    (41, 48, 10.0, 81),     # R = H - 1: the deepest legal reflection, on both borders of every column
    (48, 41, 10.0, 81),     # the same along W
    (19, 37, 2.0, 17),      # W no multiple of the wave / tile width, H below any tile height
    (24, 24, 1.4, 13),      # the even-k rule: int(8 sigma + 1) = 12 -> 13
    (130, 70, 16.0, 129),   # the largest accepted ksize
    (256, 256, 10.0, 81),   # the workload's own shape
]
SEED = 3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _case(H, W, sigma):
    """(noise f32 [2, H, W], taps f32 [k], (scale_x, scale_y), ref f64 [H, W, 2]) -- computed once, shared, never written to."""
    noise = ER.draw_noise(H, W, _gen(SEED))
    taps = ER.gaussian_taps(sigma)
    sx, sy = ER.pixel_scales(H, W, ALPHA)
    return noise, taps, (sx, sy), ER.blur_field(noise, taps, sx, sy)


def _call(E, noise_ptr, disp_ptr, H, W, k, taps, sx, sy):
    ws = E._workspace(max(int(E.lib.gn_elastic_field_workspace_bytes(H, W)), 4))
    return int(E.lib.gn_elastic_field(E._ctx, noise_ptr, disp_ptr, ws.data_ptr(), H, W, k, (C.c_float * len(taps))(*taps), sx, sy))


def _device_field(E, noise, taps, sx, sy):
    _, H, W = noise.shape
    nd = noise.contiguous().cuda()
    disp = torch.full((H, W, 2), float("nan"), dtype=F32, device="cuda")
    rc = _call(E, nd.data_ptr(), disp.data_ptr(), H, W, taps.numel(), taps.tolist(), sx, sy)
    assert rc == 0
    return disp


@pytest.mark.parametrize("H, W, sigma, k", CASES)
def test_field_matches_the_f64_reference(engine, H, W, sigma, k):
    noise, taps, (sx, sy), ref = _case(H, W, sigma)
    assert taps.numel() == k and int(engine.lib.gn_elastic_field_workspace_bytes(H, W)) >= 2 * H * W * 4
    got = _device_field(engine, noise, taps, sx, sy)
    assert got.dtype == F32 and tuple(got.shape) == (H, W, 2)
    again = _device_field(engine, noise, taps, sx, sy)
    got, again = got.cpu(), again.cpu()
    err, bound = float((got.double() - ref).abs().max()), ER.field_bound(ALPHA, k)
    print(f"elastic field {H}x{W} sigma {sigma} (k {k}): max |device - ref64| {err:.3e} px (bound {bound:.3e}), max |field| {float(ref.abs().max()):.3f} px")
    assert err <= bound
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches on one input must give the same bits"


@pytest.mark.parametrize("H, W, sigma, k", CASES)
def test_device_route_matches_the_host_route(engine, H, W, sigma, k):
    from genima_amd.act_training import elastic_displacement, elastic_displacement_device

    host = elastic_displacement(H, W, ALPHA, sigma, generator=_gen(SEED))
    g = _gen(SEED)
    dev = elastic_displacement_device(engine, H, W, ALPHA, sigma, generator=g)
    assert dev.is_cuda and dev.dtype == F32 and tuple(dev.shape) == (H, W, 2) and dev.is_contiguous()
    gh = _gen(SEED)
    ER.draw_noise(H, W, gh)
    assert torch.equal(g.get_state(), gh.get_state()), "the device route must consume the two noise draws and nothing else"
    err = float((dev.cpu().double() - host.double()).abs().max())
    bound = ER.field_bound(ALPHA, k) + 2.0 ** -24 * float(host.abs().max())  # + the host route's own rounding to f32
    print(f"elastic field {H}x{W} sigma {sigma}: max |device route - host route| {err:.3e} px (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("H, W, sigma", [(41, 48, 10.0), (19, 37, 2.0), (70, 130, 2.0)])
def test_constant_plane_stays_constant(engine, H, W, sigma):
    """The taps sum to 1 and reflect padding of a constant is that constant: scale * c everywhere, the borders included -- a wrong reflect
    index reads outside the strip and a tap dropped at an edge lowers the sum."""
    taps = ER.gaussian_taps(sigma)
    sx, sy = ER.pixel_scales(H, W, ALPHA)
    noise = torch.empty(2, H, W, dtype=F32)
    noise[0], noise[1] = 0.75, -0.5
    got = _device_field(engine, noise, taps, sx, sy).cpu().double()
    want = torch.tensor([0.75 * sx, -0.5 * sy], dtype=F64) * float(taps.double().sum())
    err = float((got - want).abs().max())
    print(f"constant planes {H}x{W} sigma {sigma}: max |device - scale * c| {err:.3e} px")
    assert err <= ER.field_bound(ALPHA, taps.numel())


def _folded(taps64, n, R, at):
    """v[i] = sum of the taps t with reflect(i + t - R) == at, i < n: one axis of an impulse's response under reflect padding."""
    src = F.pad(torch.arange(n, dtype=F64)[None, None], (R, R), mode="reflect")[0, 0].long()  # padded position -> source index
    k = taps64.numel()
    return torch.stack([(taps64 * (src[i:i + k] == at)).sum() for i in range(n)])


@pytest.mark.parametrize("H, W, sigma, p0, p1", [
    (19, 37, 2.0, (9, 18), (0, 35)),      # one pixel clear of every border, one inside both halos
    (41, 48, 10.0, (40, 0), (3, 47)),     # R = H - 1: every row folds
    (70, 130, 2.0, (31, 63), (32, 64)),   # either side of a tile seam in both passes
])
def test_single_pixel_gives_the_folded_outer_product(engine, H, W, sigma, p0, p1):
    taps = ER.gaussian_taps(sigma)
    k, t64 = taps.numel(), taps.double()
    sx, sy = ER.pixel_scales(H, W, ALPHA)
    noise = torch.zeros(2, H, W, dtype=F32)
    noise[0][p0], noise[1][p1] = 0.75, -0.75
    got = _device_field(engine, noise, taps, sx, sy).cpu().double()
    want = torch.stack([0.75 * sx * torch.outer(_folded(t64, H, k // 2, p0[0]), _folded(t64, W, k // 2, p0[1])),
                        -0.75 * sy * torch.outer(_folded(t64, H, k // 2, p1[0]), _folded(t64, W, k // 2, p1[1]))], dim=-1)
    err = float((got - want).abs().max())
    print(f"impulses {H}x{W} sigma {sigma}: max |device - folded outer product| {err:.3e} px, peak {float(want.abs().max()):.3f}")
    assert float(want.abs().max()) > 0.05 and err <= ER.field_bound(ALPHA, k)


def test_refused_arguments_launch_nothing(engine):
    """Argument checks only: a non-zero status, and the sentinel-filled output is as it was."""
    H = W = 48
    taps = ER.gaussian_taps(10.0).tolist()  # 81
    noise = torch.zeros(2, 256, 256, dtype=F32, device="cuda")  # sized for the largest shape named below
    disp = torch.full((256, 256, 2), 7.0, dtype=F32, device="cuda")
    big = ER.gaussian_taps(16.0).tolist() + [0.0, 0.0]  # 131 values
    refused = [
        ("H = R", (noise.data_ptr(), disp.data_ptr(), 40, W, 81, taps)),
        ("W = R", (noise.data_ptr(), disp.data_ptr(), H, 40, 81, taps)),
        ("even ksize", (noise.data_ptr(), disp.data_ptr(), H, W, 80, taps)),
        ("ksize = 131", (noise.data_ptr(), disp.data_ptr(), 256, 256, 131, big)),
        ("ksize = 1", (noise.data_ptr(), disp.data_ptr(), H, W, 1, taps)),
        ("noise == disp", (disp.data_ptr(), disp.data_ptr(), H, W, 81, taps)),
        ("null noise", (None, disp.data_ptr(), H, W, 81, taps)),
    ]
    for what, (n_ptr, d_ptr, h, w, k, tp) in refused:
        assert _call(engine, n_ptr, d_ptr, h, w, k, tp, 40.0, 40.0) != 0, what
    ws = engine._workspace(2 * H * W * 4)
    assert int(engine.lib.gn_elastic_field(engine._ctx, noise.data_ptr(), disp.data_ptr(), ws.data_ptr(), H, W, 81, None, 40.0, 40.0)) != 0
    assert int(engine.lib.gn_elastic_field(engine._ctx, noise.data_ptr(), disp.data_ptr(), None, H, W, 81, (C.c_float * 81)(*taps), 40.0, 40.0)) != 0
    torch.cuda.synchronize()
    assert bool((disp == 7.0).all())


def test_act_augment_device_field_against_host_field(engine):
    from genima_amd.act_training import act_augment

    img = torch.randint(0, 256, (1, 2, 64, 64, 3), generator=_gen(8), dtype=torch.uint8).cuda()
    gh, gd = _gen(5), _gen(5)
    host = act_augment(engine, img, gh, p=1.0, noise_std=0.0, field="host")
    dev = act_augment(engine, img, gd, p=1.0, noise_std=0.0, field="device")
    assert dev.shape == host.shape == (1, 2, 64, 64, 8) and dev.dtype == host.dtype == torch.float16
    assert float(dev[..., 3:].abs().max()) == 0.0 and float(host[..., 3:].abs().max()) == 0.0
    delta = ER.field_bound(ALPHA, 81)
    bound = 4 * delta + 2.0 ** -10  # two axes, each weight error enters two taps, |img| <= 1; two f16 roundings near 1.0
    err = float((dev[..., :3].float() - host[..., :3].float()).abs().max())
    print(f"act_augment device field vs host field: max |diff| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert torch.equal(gh.get_state(), gd.get_state()), "both routes must consume the generator identically"
    with pytest.raises(ValueError):
        act_augment(engine, img, _gen(5), p=1.0, noise_std=0.0, field="gpu")


def test_agent_update_with_the_device_field(monkeypatch):
    """``GenimaACT.update`` with ``elastic_field="device"`` in its config, from a RoboBase-shaped replay batch: three updates, finite
    metrics, and the elastic branch that ran took the device route."""
    import numpy as np

    from genima_amd import act_training, configs
    from genima_amd.act import GenimaACT

    calls = {"device": 0, "host": 0}
    dev_fn, host_fn = act_training.elastic_displacement_device, act_training.elastic_displacement

    def _dev(*a, **kw):
        calls["device"] += 1
        return dev_fn(*a, **kw)

    def _host(*a, **kw):
        calls["host"] += 1
        return host_fn(*a, **kw)

    monkeypatch.setattr(act_training, "elastic_displacement_device", _dev)
    monkeypatch.setattr(act_training, "elastic_displacement", _host)
    cfg, ccfg = dict(configs.TINY_ACT_POLICY, data_augmentation=True, elastic_field="device"), configs.TINY_ACT_CLIP_TEXT
    agent = GenimaACT(cfg, None, ccfg, None, device="cuda", seed=4)
    B, S, Tq = 2, cfg["image_size"], cfg["num_queries"]
    g = _gen(8)
    cams = ["left_shoulder", "right_shoulder", "front", "wrist"]
    Vc = ccfg["vocab_size"]
    toks = np.zeros((B, 1, 77), dtype=np.int32)
    toks[:, 0, :5] = [Vc - 2, 3, 4, 5, Vc - 1]
    batch = {f"{c}_rgb": torch.randint(0, 256, (B, 1, 3, S, S), generator=g, dtype=torch.uint8).numpy() for c in cams}
    batch.update({f"{c}_rgb_tp1": batch[f"{c}_rgb"] for c in cams})
    batch.update(low_dim_state=torch.randn(B, 1, cfg["state_dim"], generator=g).numpy(), lang_tokens=toks, reward=np.ones((B,), np.float32),
                 action=torch.rand(B, Tq, cfg["action_dim"], generator=g).numpy())
    m = [agent.update(iter([batch]), i, lr=1e-3, lr_backbone=1e-4) for i in range(3)]
    assert set(m[0]) == {"actor_loss", "actor_l1_loss", "actor_gripper_loss", "actor_kl_loss", "batch_reward"}
    assert all(np.isfinite(list(x.values())).all() for x in m)
    print("elastic branch calls over three updates:", calls)
    assert calls["device"] >= 1 and calls["host"] == 0
