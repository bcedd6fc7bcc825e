"""-m "not gpu": the host side of the drawn random-background replay (``genima_amd.replay`` render mode) -- the background draw against an
independent restatement and its statistics, the per-observation view tables, the texture bank, the command-line flags and the refusals."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import replay_render_ref as RR
from genima_amd import render as R
from genima_amd import replay as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = ("front", "overhead")


def _cpu_engine():
    """The tables of a DeviceReplay go wherever its engine lives; ``sample`` is never called here."""
    return types.SimpleNamespace(device=torch.device("cpu"))


@pytest.mark.parametrize("NB", [3, 7])
@pytest.mark.parametrize("seed", RR.SEEDS)
def test_draw_backgrounds_equals_the_restatement(seed, NB):
    for draw in range(16):
        layer, blend = P.draw_backgrounds(seed, draw, 3, 2, 2, NB, 0.7)
        want_layer, want_blend = RR.draws(seed, draw, 3, 2, 2, NB, 0.7)
        assert layer.dtype == np.int32 and blend.dtype == np.float64 and layer.shape == blend.shape == (3, 4)
        assert np.array_equal(layer, want_layer) and np.array_equal(blend.view(np.int64), want_blend.view(np.int64)), (seed, draw)


@pytest.mark.parametrize("NB", [3, 7])
@pytest.mark.parametrize("seed", RR.SEEDS)
def test_draw_statistics(seed, NB):
    """B = 8, V = 4, fs = 1, 16 draws: n = 512 slots.  A layer count is binomial(n, 1 / NB); the blend is uniform on [alpha, 1), so its mean
    has sigma = 0.3 / sqrt(12 n).  Both within 4 sigma (measured when the formula was chosen: 2.1 and 0.9)."""
    alpha, n = 0.7, 512
    got = [P.draw_backgrounds(seed, d, 8, 4, 1, NB, alpha) for d in range(16)]
    layer, blend = np.concatenate([g[0].ravel() for g in got]), np.concatenate([g[1].ravel() for g in got])
    assert layer.size == n and layer.min() >= 0 and layer.max() < NB
    p = 1.0 / NB
    counts = np.bincount(layer, minlength=NB)
    z = (counts - n * p) / np.sqrt(n * p * (1 - p))
    zm = (blend.mean() - (alpha + 1.0) / 2) / (0.3 / np.sqrt(12 * n))
    print("seed", hex(seed), "NB", NB, "counts", counts.tolist(), "max |z|", float(np.abs(z).max()), "mean z", float(zm), "min", blend.min(), "max", blend.max())
    assert np.abs(z).max() <= 4.0 and abs(zm) <= 4.0
    assert (blend >= alpha).all() and (blend < 1.0).all()


@pytest.mark.parametrize("seed", RR.SEEDS)
def test_draws_differ_from_batch_to_batch_and_use_every_layer(seed):
    l0, _ = P.draw_backgrounds(seed, 0, 3, 2, 2, 3, 0.7)
    l1, _ = P.draw_backgrounds(seed, 1, 3, 2, 2, 3, 0.7)
    assert not np.array_equal(l0, l1)
    assert set(np.concatenate([l0.ravel(), l1.ravel()]).tolist()) == {0, 1, 2}


def test_view_tables_equal_pack_step_per_observation():
    cfg, eps = RR.episodes((9,), 96, CAMS)
    rp = P.DeviceReplay(eps, CAMS, engine=_cpu_engine(), action_sequence=4, batch_size=2,
                        render=P.RenderTargets(cfg, RR.bank(3, 96), seed=5))
    traj = eps[0][1]
    assert (rp.N, rp.N_obs, rp.V, rp.H, rp.W, rp.NB, rp.samples, rp.draw) == (8, 9, 2, 96, 96, 3, 4, 0)
    assert rp.render.alpha_blend == cfg.alpha_blend == 0.7
    for ts in range(9):
        want = R.pack_views(R.pack_step(traj, cfg, ts, CAMS))
        for k in ("cams", "spheres", "tex_index", "count"):
            assert rp.host_views[k].dtype == want[k].dtype
            assert np.array_equal(rp.host_views[k][ts * 2: ts * 2 + 2], want[k]), (ts, k)
            assert np.array_equal(getattr(rp, k).numpy()[ts * 2: ts * 2 + 2], want[k]), (ts, k)
    # horizon 4 over 9 steps: 4 spheres in front, the gripper alone from overhead; the windows of the last two steps are empty
    assert rp.host_views["count"].reshape(9, 2).tolist() == [[4, 1]] * 7 + [[0, 0]] * 2
    assert rp.device_bytes == sum(rp.host_views[k].nbytes for k in rp.host_views) + 3 * 96 * 96 * 3 + rp.host_atlas.nbytes
    assert rp.host_frames is None and rp.frame_ptr is None and rp.chunks == []
    with pytest.raises(ValueError, match="render mode"):
        rp.host_batch([0])
    with pytest.raises(ValueError, match="capacity_bytes"):
        P.DeviceReplay(eps, CAMS, engine=_cpu_engine(), render=P.RenderTargets(cfg, RR.bank(3, 96)), capacity_bytes=rp.device_bytes - 1)


def test_texture_bank_order_and_shape(tmp_path):
    from PIL import Image

    rng = np.random.RandomState(0)
    files = {"tex10.png": (40, 30), "tex2.png": (96, 96), "tex1.jpg": (17, 64)}  # natural order: tex1, tex2, tex10
    imgs = {}
    for name, (w, h) in files.items():
        imgs[name] = Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        imgs[name].save(str(tmp_path / name))
    Image.fromarray(rng.randint(0, 256, (8, 8)).astype(np.uint8), mode="L").save(str(tmp_path / "tex3.png"))  # a grey file: converted after the resize
    bank = P.load_texture_bank(str(tmp_path), 48, 96)
    assert bank.dtype == np.uint8 and bank.shape == (4, 48, 96, 3) and bank.flags.c_contiguous
    for layer, name in enumerate(("tex1.jpg", "tex2.png", "tex3.png", "tex10.png")):
        want = np.asarray(Image.open(str(tmp_path / name)).resize((96, 48)).convert("RGB"), dtype=np.uint8)
        assert np.array_equal(bank[layer], want), name
    arr = RR.bank(2, 8)
    assert np.array_equal(P.load_texture_bank(arr, 8, 8), arr)
    for bad in (arr.astype(np.float32), arr[0], RR.bank(2, 9), arr[:0]):
        with pytest.raises(ValueError):
            P.load_texture_bank(bad, 8, 8)
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(ValueError, match="no texture files"):
        P.load_texture_bank(str(tmp_path / "empty"), 8, 8)


def test_render_mode_refusals(tmp_path):
    cfg, eps = RR.episodes((6,), 96, CAMS)
    rt = P.RenderTargets(cfg, RR.bank(3, 96))
    ep_dir = str(tmp_path / "episode0")
    os.makedirs(ep_dir)
    P.save_demo(os.path.join(ep_dir, "demo.npz"), eps[0][0])
    with pytest.raises(ValueError, match=r"traj\.npz.*episode0"):  # the error names the episode
        P.DeviceReplay([ep_dir], CAMS, engine=_cpu_engine(), render=rt)
    R.save_traj(os.path.join(ep_dir, "traj.npz"), eps[0][1])
    with open(os.path.join(ep_dir, "description.txt"), "w") as f:
        f.write("open box\n")
    rp = P.DeviceReplay([ep_dir], CAMS, engine=_cpu_engine(), render=rt)  # no camera directory exists, none is read
    assert rp.descriptions == ["open box"] and rp.N == 5
    with pytest.raises(ValueError, match="image_size"):
        P.DeviceReplay(eps, CAMS, engine=_cpu_engine(), render=rt, image_size=64)
    assert P.DeviceReplay(eps, CAMS, engine=_cpu_engine(), render=rt, image_size=96).H == 96
    with pytest.raises(ValueError, match="cameras"):
        P.DeviceReplay(eps, ("front", "nowhere"), engine=_cpu_engine(), render=rt)
    with pytest.raises(ValueError, match="observations"):
        P.DeviceReplay([(P.synthetic_demo(7, size=2, cameras=CAMS[:1])[0], eps[0][1])], CAMS, engine=_cpu_engine(), render=rt)
    with pytest.raises(ValueError, match="alpha_blend"):
        P.RenderTargets(cfg, RR.bank(3, 96), alpha_blend=1.5)
    with pytest.raises(ValueError, match="render mode"):
        rp.host_batch([0])


def test_train_act_flags_parse():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_act
    finally:
        sys.path.pop(0)
    a = train_act.parse(["--dataset_root", "/data"])
    assert (a.rnd_bg_textures, a.sphere_textures, a.alpha_blend, a.render_seed) == (None, "./sphere_textures/", 0.7, 0)
    a = train_act.parse(["--dataset_root", "/data", "--rnd_bg_textures", "/tex", "--sphere_textures", "/sph", "--alpha_blend", "0.5", "--render_seed", "9"])
    assert (a.rnd_bg_textures, a.sphere_textures, a.alpha_blend, a.render_seed) == ("/tex", "/sph", 0.5, 9)
    assert "rnd_bg" in train_act.__doc__ and "rlbench_rgb_rendered" not in train_act.__doc__
