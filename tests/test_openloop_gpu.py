"""-m gpu: ``OpenLoopEval`` end to end on the tiny families -- the tables' rows and order, repeatability, two transitions recomputed outside
the evaluator (the same pipeline call with the same generator state, ``act_tiled``, the numpy scores of tests/openloop_ref.py), the oracle row
against ``controller.act`` on the rendered target, the empty-window steps, one transition against ``harness.control_step`` bit for bit, the
refusals and ``controller_validator``.

Shapes: 64 x 64 views (the tiny ACT config's; the tiny pipeline then runs its native 128 x 128 canvas), V = 4, two episodes of 6 and 9
observations = 5 + 8 = 13 transitions, batch 3: five batches, the last one holds one transition and two repeats of it.  With a horizon of 4 the
observations L - 2 and L - 1 of a trajectory have an empty window (``render.window_step``); L - 1 starts no transition, so the last transition
of each episode is the one that draws no sphere.  ``control_step`` tiles 256 x 256 views only, so that comparison runs a second evaluator on
one 3-observation episode at 256 x 256, batch 1."""
import types

import numpy as np
import pytest
import torch

import openloop_ref as OR
import replay_render_ref as RR
from genima_amd import configs, harness
from genima_amd import render as R
from genima_amd import replay as P
from genima_amd.act import GenimaACT
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import OpenLoopEval, controller_validator

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED = 64, (6, 9), 3, 2
N = sum(L - 1 for L in LENGTHS)


def _episodes(lengths, size):
    cfg, eps = RR.episodes(lengths, size, CAMS)
    return cfg, [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=size, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]


def _stats():
    demos = [P.synthetic_demo(L, seed=90 + i)[0] for i, L in enumerate((7, 8))]  # the "training" set: other demos than the scored ones
    return P.action_stats(demos), P.proprio_stats(demos)


def _agents(resolution):
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=resolution, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    return SDControlNetAgent(ns), GenimaACT(dict(configs.TINY_ACT_POLICY), None, configs.TINY_ACT_CLIP_TEXT, None, device="cuda", seed=4)


@pytest.fixture(scope="module")
def world(engine):
    cfg, eps = _episodes(LENGTHS, SIZE)
    dagent, controller = _agents(2 * SIZE)
    ev = OpenLoopEval(dagent, controller, eps, CAMS, render_cfg=cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine)
    return types.SimpleNamespace(cfg=cfg, eps=eps, dagent=dagent, controller=controller, ev=ev, res=ev.run())


def test_tables_hold_every_transition_once_in_order(world):
    res = world.res
    assert len(res) == N == 13 and res.image.shape == (N, 4, 5) and res.image.dtype == np.int64
    assert res.episode.tolist() == [0] * 5 + [1] * 8 and res.step.tolist() == list(range(5)) + list(range(8))
    for name in ("generated", "oracle"):
        for unit in ("norm", "rad"):
            t = res.actions[name][unit]
            assert t.shape == (N, 20, 2) and t.dtype == np.float32 and np.isfinite(t).all() and set(np.unique(t[..., 1])) <= {0.0, 1.0}
    assert (res.image[..., 1] + res.image[..., 3] == SIZE * SIZE).all()  # every pixel of every view counted once, in every row
    assert (res.image[..., 4] > 0).all()  # no row left at its zero
    s = res.summary()
    assert s["n"] == N and np.isfinite(s["generated"]["joint_l1_norm"]) and set(s["per_task"]) == {"open box 0", "open box 1"}


def test_a_second_run_gives_the_same_bits(world):
    again = world.ev.run()
    assert np.array_equal(again.image, world.res.image)
    for name in ("generated", "oracle"):
        for unit in ("norm", "rad"):
            assert np.array_equal(again.actions[name][unit].view(np.int32), world.res.actions[name][unit].view(np.int32)), (name, unit)


def _check_actions(tabs, n, a_hat16, actions, std):
    for unit, scale in (("norm", None), ("rad", std)):
        total, flag, bound = OR.action_metrics(a_hat16, actions, scale)
        got = tabs[unit][n].astype(np.float64)
        err = np.abs(got[:, 0] - total[0])
        print(f"transition {n} {unit}: max error {err.max():.3e}, max error / bound {(err / bound[0]).max():.3f}")
        assert np.array_equal(got[:, 1], flag[0]) and (err <= bound[0]).all()


def test_two_transitions_recomputed_outside_the_evaluator(world):
    ev, res, dagent, controller = world.ev, world.res, world.dagent, world.controller
    std = np.asarray(ev.replay.action_stats["std"], np.float64)[:7].astype(np.float32)
    chosen = {4: (1, 1), 12: (4, 0)}  # transition -> (batch, position); batch 4 is the padded one: [12, 12, 12]
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    with torch.inference_mode():
        for k in range(5):
            idx = np.minimum(np.arange(k * BATCH, (k + 1) * BATCH), N - 1)
            batch = ev.targets(idx)
            frames = batch["images_u8"].cpu().numpy()  # [B, 4, H, W, 3]
            tiled = np.zeros((BATCH, 2 * SIZE, 2 * SIZE, 3), np.uint8)
            for v in range(4):
                tiled[:, (v // 2) * SIZE:(v // 2 + 1) * SIZE, (v % 2) * SIZE:(v % 2 + 1) * SIZE] = frames[:, v]
            assert np.array_equal(batch["tiled"].cpu().numpy(), tiled)
            prompts = [harness.make_prompt(world.eps[res.episode[n]][3]) for n in idx]
            out = dagent.pipe(prompt=prompts, image=torch.from_numpy(tiled), num_inference_steps=5, guidance_scale=0.0, generator=gen, output_type="pt").images
            for n, (kb, pos) in chosen.items():
                if kb != k:
                    continue
                a_hat = controller.act_tiled(out, batch["low_dim_state"], batch["lang_tokens"])[pos: pos + 1].cpu().numpy()
                want = OR.image_metrics(OR.untile(out.cpu().numpy())[pos: pos + 1], batch["full"].cpu().numpy().reshape(BATCH, 4, SIZE, SIZE, 3)[pos: pos + 1],
                                        batch["occupied"].cpu().numpy().reshape(BATCH, 4, SIZE, SIZE)[pos: pos + 1])
                assert np.array_equal(res.image[n], want[0]), n
                assert a_hat.dtype == np.float16
                _check_actions(res.actions["generated"], n, a_hat, batch["action"][pos: pos + 1].cpu().numpy(), std)


def test_oracle_row_is_the_controller_on_the_rendered_target(world):
    ev, res, controller = world.ev, world.res, world.controller
    std = np.asarray(ev.replay.action_stats["std"], np.float64)[:7].astype(np.float32)
    with torch.inference_mode():
        idx = np.arange(3, 6)  # transitions 3, 4 (episode 0; 4 draws no sphere) and 5 (episode 1's first)
        batch = ev.targets(idx)
        full = batch["full"].view(BATCH, 4, SIZE, SIZE, 3)
        # gn_render_spheres' `full` over these frames, drawn here from the host-side view tables of the same steps
        views = R.pack_views([v for n in idx for v in R.pack_step(world.eps[res.episode[n]][2], world.cfg, int(res.step[n]), CAMS)])
        ref = R.render_views(ev.E, views, ev.atlas, SIZE, SIZE, world.cfg.samples, bg=batch["images_u8"].view(BATCH * 4, SIZE, SIZE, 3), want=("full",))
        assert torch.equal(ref["full"], batch["full"])
        obs = {f"{cam}_rgb": full[:, v].permute(0, 3, 1, 2).unsqueeze(1).contiguous() for v, cam in enumerate(CAMS)}
        obs["low_dim_state"], obs["lang_tokens"] = batch["low_dim_state"], batch["lang_tokens"]
        chunk = controller.act(obs).cpu().numpy()
    assert np.array_equal(chunk.astype(np.float16).astype(np.float32), chunk)  # act returns the f16 chunk, widened
    actions = batch["action"].cpu().numpy()
    for pos, n in enumerate(idx):
        _check_actions(res.actions["oracle"], int(n), chunk[pos: pos + 1].astype(np.float16), actions[pos: pos + 1], std)
    assert not np.array_equal(res.actions["oracle"]["norm"], res.actions["generated"]["norm"])  # the two rows see different images


def test_steps_with_an_empty_window_draw_no_sphere(world):
    res = world.res
    empty = [R.window_step(int(res.step[n]), LENGTHS[res.episode[n]], world.cfg.action_horizon) is None for n in range(N)]
    assert [n for n in range(N) if empty[n]] == [4, 12]  # observation L - 2 of each episode; L - 1 starts no transition
    for n in range(N):
        if empty[n]:
            assert (res.image[n, :, 1] == 0).all() and (res.image[n, :, 0] == 0).all(), n
        else:
            assert (res.image[n, :, 1] > 0).any(), n
    assert np.isnan(res.sphere_rmse()[4]).all() and world.res.summary()["image"]["sphere_missing"]["front"] >= 2


def test_one_transition_equals_control_step_bit_for_bit(engine):
    size = 256
    cfg, eps = _episodes((3,), size)
    dagent, controller = _agents(2 * size)
    ev = OpenLoopEval(dagent, controller, eps, CAMS, render_cfg=cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=1, seed=SEED, engine=engine)
    with torch.inference_mode():
        batch = ev.targets(np.array([0]))
        gen = ev.generate(batch, np.array([0]), torch.Generator(device="cuda").manual_seed(SEED))
        a_hat = controller.act_tiled(gen, batch["low_dim_state"], batch["lang_tokens"]).float().cpu().numpy()
    demo, frames, _, desc = eps[0]
    obs = {f"{cam}_rgb": np.ascontiguousarray(frames[cam][0].transpose(2, 0, 1))[None] for cam in CAMS}
    obs["low_dim_state"] = batch["low_dim_state"][0].cpu().numpy()
    obs["lang_tokens"] = RR.tokens([desc]).reshape(1, 1, 77)
    actions, _, tiled_in, tiled_out = harness.control_step(dagent, controller, obs, desc, CAMS, 1, [torch.Generator(device="cuda").manual_seed(SEED)], 5, 0.0, "cuda")
    assert np.array_equal(np.asarray(tiled_in[0]), batch["tiled"][0].cpu().numpy())
    assert np.array_equal(np.asarray(tiled_out[0]), gen[0].cpu().numpy())
    assert np.array_equal(actions.view(np.int32), a_hat[0].view(np.int32))
    # ... and the evaluator's own row 0 scores exactly that image
    res = ev.run()
    want = OR.image_metrics(OR.untile(gen.cpu().numpy()), batch["full"].cpu().numpy().reshape(1, 4, size, size, 3), batch["occupied"].cpu().numpy().reshape(1, 4, size, size))
    assert len(res) == 2 and np.array_equal(res.image[0], want[0])


def test_refusals(world):
    world.controller.set_execution(5)
    try:
        with pytest.raises(ValueError, match="execution mode"):
            OpenLoopEval(world.dagent, world.controller, world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens)
    finally:
        world.controller.set_execution()
    stacked = types.SimpleNamespace(execution=None, config={"frame_stack": 2})
    with pytest.raises(NotImplementedError, match="frame_stack"):
        OpenLoopEval(world.dagent, stacked, world.eps, CAMS, render_cfg=world.cfg, stats=_stats())
    with pytest.raises(ValueError, match="TRAINING"):
        OpenLoopEval(world.dagent, world.controller, world.eps, CAMS, render_cfg=world.cfg, stats=None)


def test_controller_validator_scores_without_touching_weights(world, engine):
    controller = GenimaACT(dict(configs.TINY_ACT_POLICY, data_augmentation=False), None, configs.TINY_ACT_CLIP_TEXT, None, device="cuda", seed=4)
    validate = controller_validator(world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, engine=engine)
    before = {k: v.clone() for k, v in controller.state_dict().items()}
    first = validate(controller, 1)
    assert np.isfinite(first["select"]) and first["select"] == first["joint_l1_norm"] > 0 and 0.0 <= first["gripper_acc"] <= 1.0 and first["n"] == N
    # the controller alone on the rendered targets: the evaluator's oracle row (the same weights: seed 4)
    assert first["select"] == world.res.summary()["oracle"]["joint_l1_norm"]
    after = controller.state_dict()
    assert set(before) <= set(after) and all(torch.equal(after[k], before[k]) for k in before)  # (the text tower's keys appear once it has run)
    assert validate(controller, 2) == first
    # inside a training run the validator reads the weights the last update left
    rp = world.ev.replay
    controller.update_device(rp.sample([0, 1, 2]))
    trained = {k: v.clone() for k, v in controller.state_dict().items()}
    second = validate(controller, 3)
    assert np.isfinite(second["select"]) and second["select"] != first["select"]
    after = controller.state_dict()
    assert all(torch.equal(after[k], trained[k]) for k in trained)
