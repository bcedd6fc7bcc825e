"""-m gpu: ``gn_render_spheres`` (csrc/render.hip) against the float64 restatement of tests/render_reference.py through the ABI, its
composites against numpy on the kernel's own render, the f16 tiled output against ``gn_image_u8_to_f16``, and the host surface
(``JointMarker``, ``render_episode``, ``DataLoader(render_targets=...)``) against the batched path.

Comparison rule: every pixel agrees to <= 1 LSB per channel and ``occupied`` / the white key agree exactly, except pixels where some
sample's ray passes within a relative 1e-4 of a silhouette (|dist^2 - r^2| <= 1e-4 r^2) or of a texel-centre boundary, where f32 and
f64 may legitimately fall on different sides; those may be at most 1 % of a view's occupied pixels.  A float32 numpy run of the same
restatement on these exact scenes (seeds 11 / samples 4 and 12 / samples 1) stays inside both bars: largest difference 1 LSB, no
``occupied`` mismatch, excluded share at most 0.30 % (samples 4) and 0.06 % (samples 1) of the occupied pixels of a view."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import render_reference as ref
from genima_amd import data as D
from genima_amd import render as R
from genima_amd.pipeline import HashTokenizer

pytestmark = pytest.mark.gpu
TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_textures")
H = W = 256


@pytest.fixture(scope="module")
def atlas():
    return R.load_atlas(TEXTURES)


@pytest.mark.parametrize("seed,samples", [(11, 4), (12, 1)])
def test_kernel_matches_the_f64_reference(engine, atlas, seed, samples):
    sc = ref.scene(seed)
    assert set(sc["tex_index"][np.arange(4)[None] < sc["count"][:, None]].tolist()) == {0, 1, 2, 3, 4}  # all five golden textures
    white = torch.full((8, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    out = R.render_views(engine, sc, atlas, H, W, samples, bg=white, want=("full", "occupied"))
    got, occ = out["full"].cpu().numpy(), out["occupied"].cpu().numpy().astype(bool)
    for b in range(8):
        want, excluded = ref.render(sc["cams"][b], sc["spheres"][b], sc["tex_index"][b], sc["count"][b], atlas, H, W, samples)
        want_occ = np.any(want != 255, -1)
        keep = ~excluded
        share = (excluded & want_occ).sum() / want_occ.sum()
        diff = np.abs(got[b].astype(int) - want.astype(int)).max(-1)
        print(f"seed {seed} samples {samples} view {b}: occupied {want_occ.sum()}, excluded share {100 * share:.3f} %, "
              f"max diff {diff[keep].max()} LSB, pixels off by one {(diff[keep] > 0).sum()}")
        assert want_occ.sum() > 500
        assert share <= 0.01
        assert diff[keep].max() <= 1
        assert np.array_equal(occ[b][keep], want_occ[keep])
        assert np.array_equal(np.all(got[b] == 255, -1)[keep], ~want_occ[keep])


def test_composites_equal_numpy_on_the_kernels_own_render(engine, atlas):
    sc = ref.scene(11)
    # view 0, its largest sphere: forced to pure white (factor 1, an all-white atlas layer): keyed out like background -- the reference's quirk
    atlas6 = np.concatenate([atlas, np.full((1,) + atlas.shape[1:], 255, np.uint8)])
    sc["spheres"][0, 1, 13:] = 1.0
    sc["tex_index"][0, 1] = 5
    rng = np.random.RandomState(3)
    bg, bg2 = (rng.randint(0, 256, (8, H, W, 3), dtype=np.uint8) for _ in range(2))
    bg2[1] = 255  # a white texture too
    blend = rng.uniform(0.7, 1.0, 8)
    blend[2], blend[3] = 1.0, 0.7
    white = torch.full((8, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    raw = R.render_views(engine, sc, atlas6, H, W, 4, bg=white, want=("full",))["full"].cpu().numpy()
    grey = sc["spheres"].copy()
    grey[..., 13:] = 0.5
    plain = R.render_views(engine, {**sc, "spheres": grey}, atlas6, H, W, 4, bg=white, want=("occupied",))["occupied"].cpu().numpy()
    out = R.render_views(engine, sc, atlas6, H, W, 4, bg=torch.from_numpy(bg).cuda(), bg2=torch.from_numpy(bg2).cuda(), blend=blend,
                         want=("full", "rnd", "occupied"))
    for b in range(8):
        full, rnd, occ = ref.composite(raw[b], bg[b], bg2[b], blend[b])
        assert np.array_equal(out["full"][b].cpu().numpy(), full)
        assert np.array_equal(out["rnd"][b].cpu().numpy(), rnd)
        assert np.array_equal(out["occupied"][b].cpu().numpy().astype(bool), occ)
    assert plain[0].sum() > out["occupied"][0].sum() + 500  # the white sphere covers pixels and is not "occupied"


def test_f16_tiled_output_is_image_u8_to_f16_of_the_tiled_bytes(engine, atlas):
    sc = ref.scene(11)
    rng = np.random.RandomState(5)
    bg, bg2 = (torch.from_numpy(rng.randint(0, 256, (8, H, W, 3), dtype=np.uint8)).cuda() for _ in range(2))
    blend = rng.uniform(0.7, 1.0, 8)
    out = R.render_views(engine, sc, atlas, H, W, 4, bg=bg, bg2=bg2, blend=blend, want=("full", "rnd", "full_f16", "rnd_f16"),
                         full_scale=(2.0, -1.0), rnd_scale=(1.0, 0.0))

    def tiled(x):  # [8, H, W, 3] -> [2, 2H, 2W, 3], view 4 i + t at tile row t // 2, column t % 2
        return x.view(2, 2, 2, H, W, 3).permute(0, 1, 3, 2, 4, 5).reshape(2, 2 * H, 2 * W, 3).contiguous()

    assert np.array_equal(tiled(out["full"])[1].cpu().numpy(), R._tile([out["full"][4 + t].cpu().numpy() for t in range(4)]))
    for k, (mul, add) in (("full", (2.0, -1.0)), ("rnd", (1.0, 0.0))):
        want = engine.image_u8_to_f16(tiled(out[k]), 8, mul, add)
        assert torch.equal(out[k + "_f16"].view(torch.int16), want.view(torch.int16)), k
    # the tiled background form and an explicit tile_index give the same bytes
    perm = np.array([5, 4, 7, 6, 1, 0, 3, 2], np.int32)
    again = R.render_views(engine, sc, atlas, H, W, 4, bg=tiled(bg)[:, :, :, :], bg_tiled=True, n_tiled=2, want=("full_f16",))
    assert torch.equal(again["full_f16"].view(torch.int16), out["full_f16"].view(torch.int16))
    moved = R.render_views(engine, sc, atlas, H, W, 4, bg=bg, tile_index=perm, n_tiled=2, want=("full_f16",))["full_f16"]
    want = engine.image_u8_to_f16(tiled(out["full"][torch.from_numpy(np.argsort(perm)).cuda()]), 8, 2.0, -1.0)
    assert torch.equal(moved.view(torch.int16), want.view(torch.int16))


def test_bad_arguments_are_refused_without_launching(engine, atlas):
    sc = ref.scene(11)
    white = torch.full((8, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    from genima_amd._lib import GenimaHipError
    for kw in (dict(samples=2), dict(want=("rnd",)), dict(want=("full",), bg=None)):
        args = dict(samples=4, bg=white, want=("full",))
        args.update(kw)
        with pytest.raises(GenimaHipError):
            R.render_views(engine, sc, atlas, H, W, args.pop("samples"), **args)


def _episode(L=9, seed=7):
    return R.synthetic_episode(L, seed, TEXTURES)


def test_joint_marker_returns_the_batched_image(engine):
    cfg, traj, frames = _episode()
    jm = R.JointMarker(W, H, cfg.camera_scales, sphere_radius=cfg.sphere_radius, znear=cfg.znear, zfar=cfg.zfar, texture_dir=TEXTURES, engine=engine)
    mats, opens, colors = R.step_spheres(traj, cfg, 0, "wrist")
    ext = np.array(traj["extrinsics"][0][0])
    img = jm.render_action(traj["intrinsics"][0][0], ext, mats, opens, camera_scale=3.0, sphere_colors=colors)
    assert np.array_equal(ext, traj["extrinsics"][0][0])  # the caller's matrix is not flipped in place
    assert img.shape == (H, W, 3) and img.dtype == np.uint8 and np.any(img != 255)
    white = torch.full((5, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    batch = R.render_views(engine, R.pack_views(R.pack_step(traj, cfg, 0)), jm.atlas, H, W, 4, bg=white)["full"].cpu().numpy()
    assert np.array_equal(img, batch[0])
    one = R.render_views(engine, R.pack_views(R.pack_step(traj, cfg, 0, ["wrist"])), jm.atlas, H, W, 4, bg=white[:1])["full"].cpu().numpy()
    assert one.shape == (1, H, W, 3) and np.array_equal(img, one[0])  # the batched path at B = 1


@pytest.mark.parametrize("cache", [None, "device"])
def test_loader_render_targets_equals_the_png_tree(engine, tmp_path, cache):
    cfg, traj, frames = _episode()
    base = os.path.join(str(tmp_path), "open_box", "variation0")
    ep = os.path.join(base, "episodes", "episode0")
    os.makedirs(ep)
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    R.render_episode(traj, frames, ep, cfg, engine=engine)
    L = len(traj["gripper_open"])
    assert sorted(os.listdir(os.path.join(ep, "tiled_rgb_rendered")), key=lambda s: int(s[:-4])) == [f"{i}.png" for i in range(L - 1)]
    first = np.asarray(Image.open(os.path.join(ep, "tiled_rgb_rendered", "0.png")))
    assert first.shape == (512, 512, 3) and np.any(first != np.asarray(Image.open(os.path.join(ep, "tiled_rgb", "0.png"))))  # spheres were drawn
    assert np.array_equal(first[:256, 256:], np.asarray(Image.open(os.path.join(ep, "front_rgb", "0.png"))))  # tile 1 = the second camera
    ds = D.RLBenchDataset(str(tmp_path), tasks="open_box", num_demos=1, image_type="tiled_rgb_rendered", conditioning_image_type="tiled_rgb")
    assert len(ds) == L - 2
    tok = HashTokenizer(1024)
    files = D.DataLoader(ds, 3, tok, 512, seed=1)
    drawn = D.DataLoader(ds, 3, tok, 512, seed=1, cache=cache, render_targets=R.TrajectorySource(cfg))
    for epoch in range(2):
        n = 0
        for a, b in zip(files, drawn):
            assert "pixel_values_u8" not in b and "render_views" in b
            a, b = D.to_device(engine, a), D.to_device(engine, b)
            assert set(a) == set(b) == {"pixel_values", "conditioning_pixel_values", "input_ids"}
            for k in ("pixel_values", "conditioning_pixel_values"):
                assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k
            assert torch.equal(a["input_ids"], b["input_ids"])
            n += a["pixel_values"].shape[0]
        assert n == L - 2
    if cache:
        assert drawn.cache.decodes == L - 2  # only the conditioning frames, once


def test_render_episode_writes_the_random_context_tree(engine, tmp_path):
    cfg, traj, frames = _episode(L=4)
    tex_dir = os.path.join(str(tmp_path), "textures")
    os.makedirs(tex_dir)
    rng = np.random.RandomState(2)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (64, 48, 3), dtype=np.uint8)).save(os.path.join(tex_dir, f"t{i}.png"))
    cfg.textures_path = tex_dir
    out, rnd = os.path.join(str(tmp_path), "full"), os.path.join(str(tmp_path), "rnd")
    np.random.seed(9)
    R.render_episode(traj, frames, out, cfg, rnd_out_dir=rnd, engine=engine)
    # the reference's draws, in its order: per ts, per camera, choice then uniform
    np.random.seed(9)
    files = [os.path.join(tex_dir, f) for f in os.listdir(tex_dir)]
    white = torch.full((5, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    atlas = R.load_atlas(TEXTURES)
    for ts in range(3):
        raw = R.render_views(engine, R.pack_views(R.pack_step(traj, cfg, ts)), atlas, H, W, 4, bg=white)["full"].cpu().numpy()
        for c, cam in enumerate(cfg.cameras):
            tex = np.array(Image.open(np.random.choice(files)).resize((W, H)))
            blend = np.random.uniform(cfg.alpha_blend, 1.0)
            full, rn, _ = ref.composite(raw[c], frames[cam][ts], tex, blend)
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, f"{cam}_rgb", f"{ts}.png"))), full)
            assert np.array_equal(np.asarray(Image.open(os.path.join(rnd, f"{cam}_rgb", f"{ts}.png"))), rn)


def test_train_step_takes_a_render_targets_batch_and_reproduces_the_png_losses(engine, tmp_path):
    """A fine-tune fed by ``DataLoader(render_targets=...)`` (host batches and device-cache batches) against one fed from the PNG tree
    ``render_episode`` wrote: the batches are bit-identical, so the loss sequences must be too."""
    from genima_amd import configs, schema, weights
    from genima_amd.packing import pack_state_dict
    from genima_amd.scheduler import DDPMScheduler
    from genima_amd.training import ControlNetTrainer

    cfg, traj, frames = _episode(L=6)
    base = os.path.join(str(tmp_path), "open_box", "variation0")
    ep = os.path.join(base, "episodes", "episode0")
    os.makedirs(ep)
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    R.render_episode(traj, frames, ep, cfg, engine=engine)
    ds = D.RLBenchDataset(str(tmp_path), tasks="open_box", num_demos=1, image_type="tiled_rgb_rendered", conditioning_image_type="tiled_rgb")
    fam = configs.family("tiny")
    tok = HashTokenizer(fam["text"]["vocab_size"])

    def run(**kw):
        synth = lambda sch, s: weights.synth_state_dict(sch, s)  # noqa: E731
        tr = ControlNetTrainer(engine, fam["unet"], fam["controlnet"], pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), "cuda"),
                               synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-4)
        tr.attach_frozen(fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"],
                         pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), "cuda"), DDPMScheduler(), seed=5,
                         augmentations="crop,colorjitter")
        loader = D.DataLoader(ds, 2, tok, 512, shuffle=True, seed=0, **kw)
        return [float(tr.train_step(batch)) for _ in range(2) for batch in loader]

    want = run()
    assert len(want) == 4 and all(np.isfinite(want)) and len(set(want)) > 1
    assert run(render_targets=R.TrajectorySource(cfg)) == want
    assert run(render_targets=R.TrajectorySource(cfg), cache="device") == want
