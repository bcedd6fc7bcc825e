"""-m gpu: the per-sphere table of ``OpenLoopEval`` end to end on the tiny families, the diffusion-only mode and ``diffusion_validator``.

The world is tests/test_openloop_gpu.py's: 64 x 64 views, V = 4, two episodes of 6 and 9 observations = 13 transitions, batch 3 -- five
batches, the last one holds transition 12 and two repeats of it.  With a horizon of 4 transitions 4 and 12 (the last of each episode) draw no
sphere.  A camera with listed joints draws 4 spheres, so S = 4."""
import json
import os
import types

import numpy as np
import pytest
import torch

import openloop_ref as OR
import replay_render_ref as RR
import sphere_metrics_ref as SR
from genima_amd import configs
from genima_amd import render as R
from genima_amd import replay as P
from genima_amd.act import GenimaACT
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import OpenLoopEval, diffusion_validator

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED, S = 64, (6, 9), 3, 2, 4
N = sum(L - 1 for L in LENGTHS)


def _episodes():
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    return cfg, [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=SIZE, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]


def _stats():
    demos = [P.synthetic_demo(L, seed=90 + i)[0] for i, L in enumerate((7, 8))]
    return P.action_stats(demos), P.proprio_stats(demos)


def _evaluator(w, controller, engine, stats):
    return OpenLoopEval(w.dagent, controller, w.eps, CAMS, render_cfg=w.cfg, stats=stats, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine)


@pytest.fixture(scope="module")
def world(engine):
    cfg, eps = _episodes()
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=2 * SIZE, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    w = types.SimpleNamespace(cfg=cfg, eps=eps, dagent=SDControlNetAgent(ns),
                              controller=GenimaACT(dict(configs.TINY_ACT_POLICY), None, configs.TINY_ACT_CLIP_TEXT, None, device="cuda", seed=4))
    w.ev = _evaluator(w, w.controller, engine, _stats())
    w.res = w.ev.run()
    return w


def test_sphere_table_rows_and_windows(world):
    res = world.res
    assert res.spheres.shape == (N, 4, S, 17) == (13, 4, 4, 17) and res.spheres.dtype == np.int64
    assert res.windows.shape == (N, 4, S, 4) and res.windows.dtype == np.int32
    # the windows are those of the host-side view tables of each transition's own step
    for n in (0, 3, 7, 12):
        views = R.pack_views(R.pack_step(world.eps[res.episode[n]][2], world.cfg, int(res.step[n]), CAMS))
        assert np.array_equal(res.windows[n], R.sphere_windows(views["cams"], views["spheres"], views["count"], SIZE, SIZE)), n
    w = res.windows
    assert (res.spheres[..., 0] == (w[..., 2] - w[..., 0]) * (w[..., 3] - w[..., 1])).all()  # column 0 is the window's area, in every row
    assert (res.spheres[..., 5] > 0).any() and (res.spheres[..., 1] > 0).any()
    sp = res.summary()["image"]["spheres"]
    assert sp["score"] is not None and np.isfinite(sp["score"]) and sum(sp["n_drawn"].values()) == sp["overall"]["n_drawn"] > 0


def test_steps_with_an_empty_horizon_window_have_no_ground_truth_mass(world):
    res = world.res
    empty = [n for n in range(N) if R.window_step(int(res.step[n]), LENGTHS[res.episode[n]], world.cfg.action_horizon) is None]
    assert empty == [4, 12]
    for n in range(N):
        if n in empty:
            assert (res.spheres[n, :, :, 5:9] == 0).all() and (res.windows[n] == 0).all() and (res.spheres[n] == 0).all(), n
            assert not res.sphere_drawn()[n].any() and np.isnan(res.sphere_shift()[n]).all()
        else:
            assert (res.spheres[n, :, :, 5] > 0).any(), n


def test_two_batches_recomputed_outside_the_evaluator(world):
    ev, res = world.ev, world.res
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    checked = []
    with torch.inference_mode():
        for k in range(5):
            idx = ev.batch_indices(k * BATCH)
            batch = ev.targets(idx)
            out = ev.generate(batch, idx, gen)  # every batch advances the one generator
            if k not in (1, 4):
                continue
            n_valid = min(BATCH, N - k * BATCH)  # batch 1: transitions 3, 4, 5; batch 4 is padded [12, 12, 12] and scores its first row only
            views = OR.untile(out.cpu().numpy())
            full = batch["full"].cpu().numpy().reshape(BATCH, 4, SIZE, SIZE, 3)
            frames = batch["images_u8"].cpu().numpy().reshape(BATCH, 4, SIZE, SIZE, 3)
            occ = batch["occupied"].cpu().numpy().reshape(BATCH, 4, SIZE, SIZE)
            want = SR.sphere_metrics(views, full, frames, occ, res.windows[idx], ev.change_threshold)
            for pos in range(n_valid):
                assert np.array_equal(res.spheres[idx[pos]], want[pos]), (k, pos)
                checked.append(int(idx[pos]))
            assert np.array_equal(res.image[idx[:n_valid]], OR.image_metrics(views, full, occ)[:n_valid])
    assert checked == [3, 4, 5, 12]


def test_a_second_evaluator_and_the_diffusion_only_mode_give_the_same_bits(world, engine):
    res = world.res
    again = _evaluator(world, world.controller, engine, _stats()).run()
    assert np.array_equal(again.image, res.image) and np.array_equal(again.spheres, res.spheres)
    assert set(again.actions) == {"generated", "oracle"}
    for name in ("generated", "oracle"):
        for unit in ("norm", "rad"):
            assert np.array_equal(again.actions[name][unit].view(np.int32), res.actions[name][unit].view(np.int32)), (name, unit)
    alone = _evaluator(world, None, None, None)  # no controller, no statistics; the device and the engine come from the pipeline
    assert alone.E.device == world.ev.E.device and alone.T == 20 and alone.joint_std is None
    only = alone.run()
    assert only.actions == {} and len(only) == N
    assert np.array_equal(only.image, res.image) and np.array_equal(only.spheres, res.spheres) and np.array_equal(only.windows, res.windows)
    s = only.summary()
    assert "generated" not in s and "oracle" not in s and s["image"]["spheres"] == res.summary()["image"]["spheres"]
    with pytest.raises(ValueError, match="nothing to score"):
        _evaluator(types.SimpleNamespace(dagent=None, eps=world.eps, cfg=world.cfg), None, engine, None)


def test_diffusion_validator_writes_one_line_per_call(world, engine, tmp_path):
    made = []

    def make_pipe():
        made.append(1)
        return world.dagent.pipe

    validate = diffusion_validator(make_pipe, world.eps, CAMS, render_cfg=world.cfg, out_dir=str(tmp_path), tokenizer=RR.tokens, batch_size=BATCH, seed=SEED,
                                   engine=engine)
    first, second = validate(500), validate(1000)
    lines = [json.loads(l) for l in open(os.path.join(str(tmp_path), "validation.jsonl"))]
    assert lines == [first, second] and len(made) == 2 and [l["step"] for l in lines] == [500, 1000]
    assert set(first) == {"step", "select", "found_rate", "shift_px", "mass_ratio", "spread_ratio", "colour_l1", "sphere_rmse", "background_rmse", "wrapped_mse", "n"}
    score = world.res.summary()["image"]["spheres"]["score"]
    assert first["select"] == score == second["select"] and first["n"] == N  # the same weights, the same seed: the evaluator's score
    assert first["wrapped_mse"] == world.res.summary()["image"]["wrapped_mse"]
