"""-m gpu: the drawn random-background replay -- ``gn_replay_render`` against ``gn_render_spheres`` on the gathered views and the drawn
textures (bit for bit: that kernel is itself pinned to the f64 reference in tests/test_render_gpu.py), its conversion against
``gn_image_u8_to_f16``, its low-dimensional outputs against ``gn_replay_gather``, the draws against the numpy restatement, the refusals, one
training step and the training loop with its resumed draw counter.  Every comparison is exact.

Shapes: 96 x 96 frames (the 64-pixel block column is partial), V = 2 cameras x frame stack 2, two episodes of 6 and 9 steps, B = 3 = [the
first transition of episode 1 (its stack repeats the episode's first observation), the same again, the last transition of episode 0 (its own
observation has an empty window: texture only)], 4 spheres / 1 sphere / none in a view, 3 textures."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import replay_render_ref as RR
from genima_amd import configs
from genima_amd import render as R
from genima_amd import replay as P
from genima_amd._lib import GenimaHipError
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu

SIZE, V, FS, LENGTHS, T, NB = 96, 2, 2, (6, 9), 4, 3
CAMS = ("front", "overhead")  # three listed joints + the gripper, the gripper alone
IDX = [5, 5, 4]
B = len(IDX)
SEED = 0x9ABC00001234


@pytest.fixture(scope="module")
def scene():
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    return cfg, eps, RR.bank(NB, SIZE)


def _replay(engine, scene, samples=4, seed=SEED):
    cfg, eps, bank = scene
    return P.DeviceReplay(eps, CAMS, engine=engine, frame_stack=FS, action_sequence=T, batch_size=2, tokenizer=RR.tokens,
                          render=P.RenderTargets(dataclasses.replace(cfg, samples=samples), bank, seed=seed))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b, keys):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("samples", [4, 1])
def test_images_equal_gn_render_spheres_on_the_drawn_textures(engine, scene, samples):
    rp = _replay(engine, scene, samples)
    got = rp.sample(IDX, want_u8=True, want_draws=True, draw=3)
    assert tuple(got["images"].shape) == (B, V * FS, SIZE, SIZE, 8) and got["images"].dtype == torch.float16
    assert tuple(got["images_u8"].shape) == (B, V * FS, SIZE, SIZE, 3) and got["images_u8"].dtype == torch.uint8
    layer, blend = RR.draws(SEED, 3, B, V, FS, NB, 0.7)
    assert got["bg_layer"].dtype == torch.int32 and np.array_equal(got["bg_layer"].cpu().numpy(), layer)
    assert got["blend"].dtype == torch.float64 and np.array_equal(got["blend"].cpu().numpy().view(np.int64), blend.view(np.int64))
    # the views in slot order, by the gather's rule
    h = rp.host
    rows = [max(h["obs_index"][n] - (FS - 1) + k, h["first_obs"][n]) * V + v for n in IDX for v in range(V) for k in range(FS)]
    assert rows[:4] == [6 * V, 6 * V, 6 * V + 1, 6 * V + 1] and rows[8:] == [3 * V, 4 * V, 3 * V + 1, 4 * V + 1]  # the clamp at observation 6, episode 1's first; observations 3, 4 of episode 0
    views = {k: rp.host_views[k][rows] for k in rp.host_views}
    assert set(views["count"].tolist()) == {0, 1, 4}
    bg2 = rp.bank[torch.from_numpy(layer.ravel().astype(np.int64)).cuda()].contiguous()
    ref = R.render_views(engine, views, rp.atlas, SIZE, SIZE, samples, bg2=bg2, blend=blend.ravel(), want=("rnd", "occupied"))
    assert torch.equal(got["images_u8"].view(B * V * FS, SIZE, SIZE, 3), ref["rnd"])
    conv = engine.image_u8_to_f16(ref["rnd"], 8, 1.0, 0.0)
    assert torch.equal(_bits(conv.view_as(got["images"])), _bits(got["images"]))
    assert not bool(got["images"][..., 3:].any())
    occupied = ref["occupied"].sum((1, 2)).tolist()
    print("samples", samples, "count", views["count"].tolist(), "occupied", occupied, "layer", layer.ravel().tolist())
    for c, occ in zip(views["count"].tolist(), occupied):
        assert occ >= 50 if c > 0 else occ == 0  # a blank render cannot pass
    # where nothing is drawn the frame is the texture itself
    assert torch.equal(got["images_u8"][2, 1], rp.bank[int(layer[2, 1])]) and views["count"][9] == 0
    assert "images_u8" not in rp.sample(IDX) and "bg_layer" not in rp.sample(IDX)


def test_low_dim_outputs_equal_the_gathers(engine, scene):
    _, eps, _ = scene
    rp = _replay(engine, scene)
    dummy = [(demo, {c: np.zeros((len(demo["gripper_open"]), 4, 4, 3), np.uint8) for c in CAMS}, desc) for demo, _, desc in eps]
    rg = P.DeviceReplay(dummy, CAMS, engine=engine, frame_stack=FS, action_sequence=T, batch_size=2, tokenizer=RR.tokens)
    assert rp.N == rg.N == 13
    for idx in (IDX, [0, 12, 7, 4]):
        a, b = rp.sample(idx), rg.sample(idx)
        assert tuple(a["lang_tokens"].shape) == (len(idx), 1, 77) and a["reward"].tolist() == [1.0] * len(idx)
        _same(a, b, ("low_dim_state", "action", "lang_tokens"))
    assert not torch.equal(a["action"][0], a["action"][1]) and not torch.equal(a["lang_tokens"][0], a["lang_tokens"][1])
    with pytest.raises(ValueError, match="render mode"):
        rg.sample(IDX, want_draws=True)


def test_draws_are_a_function_of_seed_draw_and_slot(engine, scene):
    rp = _replay(engine, scene)
    keys = ("images", "images_u8", "bg_layer", "blend", "low_dim_state", "action")
    a = rp.sample(IDX, want_u8=True, want_draws=True, draw=0)
    assert rp.draw == 0  # an explicit draw leaves the counter alone
    _same(a, rp.sample(IDX, want_u8=True, want_draws=True, draw=0), keys)
    b = rp.sample(IDX, want_u8=True, want_draws=True, draw=1)
    assert not torch.equal(a["bg_layer"], b["bg_layer"]) and not torch.equal(a["images_u8"], b["images_u8"])
    # the counter: starts at 0, one step per sample
    _same(a, rp.sample(IDX, want_u8=True, want_draws=True), keys)
    _same(b, rp.sample(IDX, want_u8=True, want_draws=True), keys)
    assert rp.draw == 2
    # another seed, other draws
    c = _replay(engine, scene, seed=1).sample(IDX, want_draws=True, draw=0)
    assert np.array_equal(c["bg_layer"].cpu().numpy(), RR.draws(1, 0, B, V, FS, NB, 0.7)[0]) and not torch.equal(c["blend"], a["blend"])
    # a device index outside [0, N) is clamped into it
    dev = torch.tensor([rp.N + 3, -2, 4], dtype=torch.int32, device="cuda")
    _same(rp.sample(dev, want_u8=True, want_draws=True, draw=7), rp.sample([rp.N - 1, 0, 4], want_u8=True, want_draws=True, draw=7), keys)
    for bad in ([rp.N], [-1], []):  # host-made indices are checked before the upload
        with pytest.raises(GenimaHipError):
            rp.sample(bad)


def test_refused_arguments_launch_nothing(engine, scene):
    rp = _replay(engine, scene)
    shapes = (((B, V * FS, SIZE, SIZE, 8), torch.float16, 7.0), ((B, V * FS, SIZE, SIZE, 3), torch.uint8, 201), ((B, FS, rp.S), torch.float32, -5.0),
              ((B, T, rp.A), torch.float32, -5.0), ((B, 77), torch.int32, -3), ((B, V * FS), torch.int32, -3), ((B, V * FS), torch.float64, -5.0))
    out = tuple(torch.full(s, v, dtype=dt, device="cuda") for s, dt, v in shapes)
    tables = (rp.cams, rp.spheres, rp.tex_index, rp.count, rp.atlas, rp.bank, rp.qpos, rp.action, rp.obs_index, rp.first_obs, rp.last_tr)
    kw = dict(samples=4, seed=SEED, draw=0, alpha_blend=0.7, lang_tokens=rp.lang_tokens, episode=rp.episode, out=out)

    def call(tables=tables, **over):
        engine.replay_render(*tables, IDX, V, FS, T, **dict(kw, **over))

    nine = (rp.cams, torch.zeros((rp.N_obs * V, 9, 16), device="cuda"), torch.zeros((rp.N_obs * V, 9), dtype=torch.int32, device="cuda")) + tables[3:]
    flat = torch.full((B * V * FS * SIZE * SIZE * 8 + 8,), 7.0, dtype=torch.float16, device="cuda")
    off = (flat[4: flat.numel() - 4].view(shapes[0][0]),) + out[1:]  # images 8 bytes off the 16-byte grid
    assert off[0].data_ptr() % 16 == 8
    for over in (dict(samples=2), dict(samples=0), dict(alpha_blend=1.5), dict(alpha_blend=-0.1), dict(alpha_blend=float("nan")), dict(tables=nine),
                 dict(out=off)):
        with pytest.raises(GenimaHipError, match="gn_replay_render"):
            call(**over)
    torch.cuda.synchronize()
    for o, (_, _, v) in zip(out, shapes):
        assert bool((o == v).all())
    assert bool((flat == 7.0).all())
    call()  # ... and the same outputs are written by a call that is accepted
    _same(dict(zip("abcdefg", out)), dict(zip("abcdefg", engine.replay_render(*tables, IDX, V, FS, T, **dict(kw, out=None, want_u8=True, want_draws=True)))), "abcdefg")
    for o, (_, _, v) in zip(out, shapes):
        assert not bool((o == v).all())


def test_record_mode_refuses_replay_render():
    E = Engine("cuda:0", record=True)
    z = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError, match="eager"):
        E.replay_render(z, z, z, z, z, z, z, z, z, z, z, z, 1, 1, 4)


# ---------------------------------------------------------------------------------------------------------------------------- training
def _agent(seed=4):
    from genima_amd.act import GenimaACT

    cfg, ccfg = dict(configs.TINY_ACT_POLICY, data_augmentation=True), configs.TINY_ACT_CLIP_TEXT
    return GenimaACT(cfg, None, ccfg, None, device="cuda", seed=seed), cfg, ccfg


def _tiny_replay(engine, lengths, **kw):
    pcfg = configs.TINY_ACT_POLICY
    cfg, eps = RR.episodes(lengths, pcfg["image_size"], P.DEFAULT_CAMERAS)
    return P.DeviceReplay(eps, P.DEFAULT_CAMERAS, engine=engine, action_sequence=pcfg["num_queries"], batch_size=2, tokenizer=RR.tokens,
                          render=P.RenderTargets(cfg, RR.bank(NB, pcfg["image_size"]), seed=3), **kw)


def test_update_device_trains_on_a_drawn_batch(engine):
    rp = _tiny_replay(engine, (4, 5))
    agent, _, _ = _agent()
    for i, ix in enumerate(([0, 3], [6, 2])):
        m = agent.update_device(rp.sample(ix), i, lr=1e-3, lr_backbone=1e-4)
        print(i, m)
        assert set(m) == {"actor_loss", "actor_l1_loss", "actor_gripper_loss", "actor_kl_loss", "batch_reward"}
        assert np.isfinite(list(m.values())).all()
    assert rp.draw == 2


def test_training_loop_counts_and_resumes_the_draw(tmp_path, engine):
    from genima_amd.act import GenimaACT
    from genima_amd.act_train_loop import ControllerTrainLoop

    rp = _tiny_replay(engine, (4, 4), generator=torch.Generator().manual_seed(1))
    agent, cfg, ccfg = _agent()
    loop = ControllerTrainLoop(agent, rp, str(tmp_path / "run"), num_train_epochs=2, checkpoint_every=1)
    last = loop.train()
    assert np.isfinite(list(last.values())).all()
    d = os.path.join(str(tmp_path / "run"), "snapshots", "genima_controller")
    assert sorted(os.listdir(d)) == ["0.pt", "action_stats.json", "latest.pt", "proprio_stats.json"]
    assert loop._num_iters == 6 and rp.draw == 6
    rp2 = _tiny_replay(engine, (4, 4))
    assert rp2.draw == 0
    again = ControllerTrainLoop(GenimaACT(cfg, None, ccfg, agent._clip_sd, device="cuda", seed=5), rp2, str(tmp_path / "run"), num_train_epochs=2,
                                checkpoint_every=1)
    assert again._epoch == 2 and again._num_iters == 6 and rp2.draw == 6
