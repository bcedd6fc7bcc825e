"""-m gpu: ``OpenLoopEval(..., executions=...)`` end to end on the tiny families, laid out as tests/test_openloop_gpu.py is: 64 x 64 views, two
episodes of 6 and 9 observations = 5 + 8 = 13 transitions, batch 3 (the last batch padded).  A run with executions leaves every table of a
run without them bit for bit as it was; the replayed modes agree with the whole-chunk scores where they must; then the real path -- the
controller itself with ``set_execution(5, True, 0.01)`` on the rendered targets -- against the replay of the table, and
``controller_validator(..., execution=...)``."""
import types

import numpy as np
import pytest
import torch

import openloop_exec_ref as XR
import replay_render_ref as RR
from genima_amd import configs
from genima_amd import replay as P
from genima_amd.act import GenimaACT
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import OpenLoopEval, controller_validator

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED = 64, (6, 9), 3, 2
N = sum(L - 1 for L in LENGTHS)
EXECUTIONS = [(1, False, 0.01), (20, False, 0.01), (5, True, 0.01), (7, True, 0.1)]
REL_BOUND = 1e-5  # tests/test_ensemble_gpu.py derives it for this arithmetic


def _episodes(lengths, size):
    cfg, eps = RR.episodes(lengths, size, CAMS)
    return cfg, [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=size, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]


def _stats():
    demos = [P.synthetic_demo(L, seed=90 + i)[0] for i, L in enumerate((7, 8))]
    return P.action_stats(demos), P.proprio_stats(demos)


@pytest.fixture(scope="module")
def world(engine):
    cfg, eps = _episodes(LENGTHS, SIZE)
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=2 * SIZE, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    dagent = SDControlNetAgent(ns)
    controller = GenimaACT(dict(configs.TINY_ACT_POLICY), None, configs.TINY_ACT_CLIP_TEXT, None, device="cuda", seed=4)
    kw = dict(render_cfg=cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine)
    plain = OpenLoopEval(dagent, controller, eps, CAMS, **kw).run()
    ev = OpenLoopEval(dagent, controller, eps, CAMS, executions=EXECUTIONS, **kw)
    return types.SimpleNamespace(cfg=cfg, eps=eps, dagent=dagent, controller=controller, ev=ev, res=ev.run(), plain=plain)


def test_executions_leave_the_other_tables_as_they_were(world):
    res, plain = world.res, world.plain
    assert plain.executions is None and plain.chunks is None and plain.execution_summary() is None
    assert np.array_equal(res.image, plain.image) and np.array_equal(res.spheres, plain.spheres) and np.array_equal(res.windows, plain.windows)
    assert set(res.actions) == set(plain.actions) == {"generated", "oracle"}
    for kind in ("generated", "oracle"):
        for unit in ("norm", "rad"):
            assert np.array_equal(res.actions[kind][unit].view(np.int32), plain.actions[kind][unit].view(np.int32)), (kind, unit)
    assert res.summary() == plain.summary()
    assert world.controller.execution is None, "the controller passed in still has no mode set"


def test_result_carries_the_replayed_modes(world):
    res = world.res
    T, A = 20, int(world.controller.config["action_dim"])
    assert [(x["h"], x["temporal_agg"], x["m"], x["K"]) for x in res.executions] == [(1, False, 0.01, 1), (20, False, 0.01, 1), (5, True, 0.01, 4), (7, True, 0.1, 3)]
    assert set(res.chunks) == {"generated", "oracle"}
    first = XR.first_transitions([L - 1 for L in LENGTHS])
    for kind in ("generated", "oracle"):
        chunks = res.chunks[kind]
        assert chunks.shape == (N, T, A) and chunks.dtype == np.float16 and np.isfinite(chunks).all() and np.abs(chunks).max() > 0
        scale = float(np.abs(chunks.astype(np.float64)).max())
        for x in res.executions:
            tabs = x[kind]
            assert tabs["actions"].shape == (N, A) and tabs["actions"].dtype == np.float32 and tabs["n_calls"].dtype == np.int32
            want, calls = XR.exec_actions(chunks, first, A, x["h"], x["temporal_agg"], x["m"])
            assert np.abs(tabs["actions"].astype(np.float64) - want).max() <= REL_BOUND * scale and np.array_equal(tabs["n_calls"], calls)
            for unit in ("norm", "rad"):
                assert tabs["scores"][unit].shape == (N, 4) and tabs["scores"][unit].dtype == np.float32 and np.isfinite(tabs["scores"][unit]).all()
    assert not np.array_equal(res.chunks["generated"], res.chunks["oracle"])
    # h = 1 without temporal_agg executes position 0 of every chunk: the whole-chunk tables' first position, bit for bit
    for kind in ("generated", "oracle"):
        one = res.executions[0][kind]
        assert np.array_equal(one["actions"], res.chunks[kind][:, 0, :].astype(np.float32))
        for unit in ("norm", "rad"):
            assert np.array_equal(one["scores"][unit][:, 0].view(np.int32), res.actions[kind][unit][:, 0, 0].view(np.int32)), (kind, unit)
            assert np.array_equal(one["scores"][unit][:, 1], res.actions[kind][unit][:, 0, 1]), (kind, unit)
        # h = 20 = T, longer than either episode: every step executes its offset in the episode's first chunk
        whole = res.executions[1][kind]
        assert np.array_equal(whole["actions"], np.stack([res.chunks[kind][first[n], n - first[n]] for n in range(N)]).astype(np.float32))
        # the demo's own jump does not depend on the mode
        assert np.array_equal(whole["scores"]["norm"][:, 3], one["scores"]["norm"][:, 3]) and (whole["scores"]["norm"][np.unique(first), 2:] == 0).all()
    s = res.execution_summary()
    assert len(s) == 4 and s[2]["calls_per_step"] == 0.2 and set(s[2]["per_task"]) == {"open box 0", "open box 1"}
    assert s[0]["oracle"]["joint_l1_norm"] == pytest.approx(res.summary()["oracle"]["per_t"]["joint_l1_norm"][0], rel=1e-12)
    assert s[2]["oracle"]["by_position"]["n"] == [3, 3, 3, 2, 2] and s[2]["generated"]["jump_boundary_norm"] > 0


def test_a_second_run_gives_the_same_bits(world):
    again = world.ev.run()
    for a, b in zip(again.executions, world.res.executions):
        for kind in ("generated", "oracle"):
            assert np.array_equal(a[kind]["actions"].view(np.int32), b[kind]["actions"].view(np.int32)) and np.array_equal(a[kind]["n_calls"], b[kind]["n_calls"])
            for unit in ("norm", "rad"):
                assert np.array_equal(a[kind]["scores"][unit].view(np.int32), b[kind]["scores"][unit].view(np.int32))
    for kind in ("generated", "oracle"):
        assert np.array_equal(again.chunks[kind].view(np.int16), world.res.chunks[kind].view(np.int16))


def test_bad_settings_are_refused(world):
    from genima_amd._lib import GenimaHipError

    kw = dict(render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens)
    for bad in ([(0, True, 0.01)], [(21, False, 0.01)], [(5, True, -1.0)], [(5, True, float("nan"))]):
        with pytest.raises(GenimaHipError):
            OpenLoopEval(world.dagent, world.controller, world.eps, CAMS, executions=bad, **kw)
    with pytest.raises(ValueError, match="executions"):
        OpenLoopEval(world.dagent, None, world.eps, CAMS, render_cfg=world.cfg, stats=None, executions=[(5, True, 0.01)])


def test_the_controller_under_the_mode_against_the_replayed_table(world, engine):
    """One episode of 12 observations (11 transitions), batch 1, the controller alone on the rendered targets.  The table's chunks come from
    the program without an execution mode, the real ones from the program that ends in the ensemble op: the two may pick different GEMM
    plans, so the chunks may differ by d, measured here; a convex combination cannot move further than its inputs, so the executed actions
    differ by at most d + 1e-5 max|chunk|."""
    h, agg, m = 5, True, 0.01
    cfg, eps = _episodes((12,), SIZE)
    controller = world.controller
    ev = OpenLoopEval(None, controller, eps, CAMS, render_cfg=cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=1, engine=engine, executions=[(h, agg, m)])
    res = ev.run()
    n, A = len(res), ev.A
    assert n == 11 and set(res.chunks) == {"oracle"}
    table, replayed = res.chunks["oracle"].astype(np.float32), res.executions[0]["oracle"]["actions"]
    controller.set_execution(h, agg, m)
    try:
        real, d = np.zeros((n, A), np.float32), 0.0
        with torch.inference_mode():
            for t in range(0, n, h):
                batch = ev.targets(np.array([t]))
                io = controller._run(batch["full"].view(1, ev.V, SIZE, SIZE, 3), batch["low_dim_state"].flatten(1), batch.get("lang_tokens"), step=t)
                assert io.exec is not None
                k = min(h, n - t)
                real[t: t + k] = io.ens_out[0, :k].cpu().numpy()
                d = max(d, float(np.abs(io.a_hat[0, :, :A].float().cpu().numpy() - table[t]).max()))
    finally:
        controller.set_execution()
    scale = float(np.abs(table).max())
    diff = float(np.abs(real - replayed).max())
    print(f"real path: d = max |a_hat_real - a_hat_table| = {d:.3e}, max |exec_real - exec_table| = {diff:.3e}, max|chunk| = {scale:.3e}")
    assert diff <= d + REL_BOUND * scale
    assert not np.array_equal(replayed[5:], table[5:, 0]), "from the second call on two chunks are averaged (else this test proves nothing)"
    assert res.executions[0]["oracle"]["n_calls"].tolist() == [1] * 5 + [2] * 5 + [3]


def test_controller_validator_selects_by_the_executed_error(world, engine):
    validate = controller_validator(world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, engine=engine,
                                    execution=(5, True, 0.01))
    got = validate(world.controller, 1)
    want = world.res.execution_summary()[2]["oracle"]  # the oracle row does not depend on the diffusion agent
    assert np.isfinite(got["select"]) and got["select"] == got["exec_joint_l1_norm"] == want["joint_l1_norm"] > 0
    assert got["exec_joint_l1_rad"] == want["joint_l1_rad"] and got["exec_gripper_acc"] == want["gripper_acc"] and got["exec_calls_per_step"] == 0.2
    assert got["exec_jump_boundary_norm"] == want["jump_boundary_norm"] and got["exec_jump_inside_norm"] == want["jump_inside_norm"]
    assert got["joint_l1_norm"] == world.res.summary()["oracle"]["joint_l1_norm"] and got["n"] == N
    plain = controller_validator(world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, engine=engine)(world.controller, 1)
    assert set(plain) == {"select", "joint_l1_norm", "joint_l1_rad", "gripper_acc", "n"} and plain["select"] == plain["joint_l1_norm"]
    assert world.controller.execution is None
