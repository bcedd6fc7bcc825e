"""-m gpu: ``OpenLoopEval(seeds=R, executions=[...], combine=("mean", "medoid"))`` end to end on the tiny families.

The tiny world of tests/test_openloop_seeds_gpu.py: 64 x 64 views, V = 4, two episodes of 6 and 9 observations = 13 transitions, batch 3, seed 2,
``seeds=3, executions=[(5, True)]``.  The new row kinds ``seed_mean`` / ``seed_medoid`` are held to the float64 restatement
(tests/ensemble_samples_ref.py ``replay_table``) applied to the seed run's chunk table that was read back, their scores to
tests/openloop_exec_ref.py on the executed actions; ``generated`` and every other table, bit for bit, to a run without ``combine``."""
import types

import numpy as np
import pytest

import ensemble_samples_ref as SR
import openloop_exec_ref as XR
import replay_render_ref as RR
from genima_amd import configs
from genima_amd import replay as P
from genima_amd.act import GenimaACT
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import OpenLoopEval

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED, R = 64, (6, 9), 3, 2, 3
N = sum(L - 1 for L in LENGTHS)
H, AGG, M = 5, True, 0.01
REL_BOUND = 1e-5  # tests/test_ensemble_samples_gpu.py's: |out - ref| <= 1e-5 * max|chunk|


def _stats():
    demos = [P.synthetic_demo(L, seed=90 + i)[0] for i, L in enumerate((7, 8))]
    return P.action_stats(demos), P.proprio_stats(demos)


@pytest.fixture(scope="module")
def world(engine):
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    eps = [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=SIZE, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=2 * SIZE, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    w = types.SimpleNamespace(cfg=cfg, eps=eps, dagent=SDControlNetAgent(ns),
                              controller=GenimaACT(dict(configs.TINY_ACT_POLICY), None, configs.TINY_ACT_CLIP_TEXT, None, device="cuda", seed=4))
    w.evaluator = lambda **kw: OpenLoopEval(w.dagent, w.controller, eps, CAMS, render_cfg=cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, seed=SEED,
                                            engine=engine, seeds=R, executions=[(H, AGG)], **kw)
    w.ev = w.evaluator(combine=("mean", "medoid"))
    w.res = w.ev.run()
    w.plain = w.evaluator().run()
    return w


def replay_with_picks(chunks, first, picks):
    """The f64 replay of execution (H, AGG, M) over the chunk each transition's pick names: tests/openloop_exec_ref.py on that one table."""
    table = np.stack([chunks[picks[n], n] for n in range(chunks.shape[1])])
    return XR.exec_actions(table, first, table.shape[2], H, AGG, M)[0]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_new_row_kinds_equal_the_restatement(world):
    res = world.res
    ex = res.executions[0]
    assert {"generated", "oracle", "seed_mean", "seed_medoid"} <= set(ex)
    chunks = res.seed_tables["chunks"].astype(np.float64)  # [R, N, T, A]
    first = world.ev.first_tr_host
    demo = world.ev.replay.action.cpu().numpy()
    std = np.asarray(world.ev.replay.action_stats["std"], np.float64)[:7].astype(np.float32)
    for rule in SR.RULES:
        got = ex["seed_" + rule]
        assert got["actions"].shape == (N, 8) and got["actions"].dtype == np.float32 and got["picks"].dtype == np.int32
        if rule == "mean":
            want, _ = SR.replay_table(chunks, first, H, AGG, M, rule)
            assert (got["picks"] == -1).all()
        else:
            # the run's own chunks are not built to keep a margin, so a pick is held to what f32 can tell apart: its f64 D lies within 1e-3 of the
            # smallest (R * T * A f32 additions move a D by ~5e-5 of it), and it IS the f64 pick wherever the runner-up is further away than that
            for n in range(N):
                D = SR.medoid_distances(chunks[:, n])
                assert D[got["picks"][n]] <= D.min() * (1 + 1e-3), (n, D, got["picks"][n])
                group, margin = SR.medoid_margin(chunks[:, n])
                if margin >= 1e-3:
                    assert got["picks"][n] == group[0], (n, D)
            want = replay_with_picks(chunks, first, got["picks"])
        err = np.abs(got["actions"].astype(np.float64) - want).max() / np.abs(chunks).max()
        print(f"seed_{rule}: |executed - restatement| / max|chunk| = {err:.3e} (bound {REL_BOUND:.0e})")
        assert err <= REL_BOUND
        assert np.array_equal(got["n_calls"], ex["generated"]["n_calls"])
        for unit, scale in (("norm", None), ("rad", std)):
            exact, bound = XR.exec_metrics(got["actions"], demo, first, scale)
            assert (np.abs(got["scores"][unit].astype(np.float64) - exact) <= bound).all(), (rule, unit)
    assert not _same(ex["seed_mean"]["actions"], ex["generated"]["actions"]), "the mean of three seeds is not seed 0's chunk"


def test_the_summary_carries_the_row_kinds(world):
    s = world.res.execution_summary()[0]
    base = world.plain.execution_summary()[0]
    new = {"seed_mean", "seed_medoid"}
    assert set(s) - set(base) == new and all(set(t) - set(base["per_task"][name]) == new for name, t in s.get("per_task", {}).items())
    without = {k: v for k, v in s.items() if k not in new}
    if "per_task" in s:
        without["per_task"] = {name: {k: v for k, v in t.items() if k not in new} for name, t in s["per_task"].items()}
    assert without == base, "beside the new row kinds the summary is the one of a run without combine"
    keys = set(s["generated"])
    assert set(s["seed_mean"]) == keys and set(s["seed_medoid"]) == keys | {"pick_histogram", "pick_is_seed0_rate"}
    hist = s["seed_medoid"]["pick_histogram"]
    picks = world.res.executions[0]["seed_medoid"]["picks"]
    assert len(hist) == R and sum(hist) == N and hist == np.bincount(picks, minlength=R).tolist()
    assert s["seed_medoid"]["pick_is_seed0_rate"] == pytest.approx(hist[0] / N, rel=1e-12)
    assert all(np.isfinite(s[k]["joint_l1_norm"]) and 0.0 <= s[k]["gripper_acc"] <= 1.0 for k in ("seed_mean", "seed_medoid"))


def test_everything_else_is_the_run_without_combine(world):
    res, plain = world.res, world.plain
    assert _same(res.image, plain.image) and _same(res.spheres, plain.spheres)
    for k in ("image", "spheres", "chunks", "demo"):
        assert _same(res.seed_tables[k], plain.seed_tables[k]), k
    for unit in ("norm", "rad"):
        assert _same(res.seed_tables["generated"][unit], plain.seed_tables["generated"][unit]) and _same(res.seed_actions[unit], plain.seed_actions[unit])
        for name in ("generated", "oracle"):
            assert _same(res.actions[name][unit], plain.actions[name][unit])
    assert _same(res.seed_spheres, plain.seed_spheres) and all(_same(res.chunks[k], plain.chunks[k]) for k in plain.chunks)
    for kind in ("generated", "oracle"):
        a, b = res.executions[0][kind], plain.executions[0][kind]
        assert set(a) == set(b) and _same(a["actions"], b["actions"]) and _same(a["n_calls"], b["n_calls"])
        assert all(_same(a["scores"][u], b["scores"][u]) for u in ("norm", "rad"))
    assert set(plain.executions[0]) == {"h", "temporal_agg", "m", "K", "generated", "oracle"}
    assert res.summary() == plain.summary() and res.seed_summary() == plain.seed_summary()


def test_refusals(world):
    with pytest.raises(ValueError, match="needs seeds=R and executions"):
        OpenLoopEval(world.dagent, world.controller, world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH,
                     executions=[(H, AGG)], combine=("mean",))
    with pytest.raises(ValueError, match="distinct rules"):
        world.evaluator(combine=("median",))
