"""-m gpu: ``OpenLoopEval(seeds=R)`` end to end on the tiny families.

The tiny world of tests/test_openloop_gpu.py, rebuilt here: 64 x 64 views, V = 4, two episodes of 6 and 9 observations = 13 transitions, batch 3
(five batches, the last one padded), seed 2, ``seeds=3`` -- with ``executions``, ``triangulate`` and ``orientation`` on as well, so that what
they report beside a seed axis is compared too.  Slice r of every seed table is held, bit for bit, to a run without ``seeds`` and with
``seed = 2 + r`` (those runs keep their chunks through ``executions``); everything outside the seed block to the run without the option; the
two reductions to the restatements of tests/seed_spread_ref.py applied to the seed tables that were read back."""
import json
import os
import types

import numpy as np
import pytest
import torch

import replay_render_ref as RR
import seed_spread_ref as SS
from genima_amd import configs
from genima_amd import replay as P
from genima_amd.act import GenimaACT
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import VALIDATOR_SCALARS, OpenLoopEval, diffusion_validator

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED, R = 64, (6, 9), 3, 2, 3
N = sum(L - 1 for L in LENGTHS)
OPTIONS = dict(executions=[(5, True)], triangulate=True, orientation=5)


def _stats():
    demos = [P.synthetic_demo(L, seed=90 + i)[0] for i, L in enumerate((7, 8))]  # the "training" set: other demos than the scored ones
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

    def evaluator(controller=w.controller, seed=SEED, **kw):
        return OpenLoopEval(w.dagent, controller, eps, CAMS, render_cfg=cfg, stats=_stats() if controller is not None else None, tokenizer=RR.tokens,
                            batch_size=BATCH, seed=seed, engine=engine, **kw)

    w.evaluator = evaluator
    w.ev = evaluator(seeds=R, **OPTIONS)
    w.res = w.ev.run()
    w.plain = [evaluator(seed=SEED + r, **(OPTIONS if r == 0 else dict(executions=[(5, True)]))).run() for r in range(R)]  # one run per seed
    return w


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_every_seed_slice_is_the_run_with_that_seed(world):
    res, st = world.res, world.res.seed_tables
    assert res.seeds == [2, 3, 4] and set(st) == {"image", "spheres", "generated", "chunks", "demo"}
    S = res.windows.shape[2]
    assert st["image"].shape == (R, N, 4, 5) and st["image"].dtype == np.int64 and st["spheres"].shape == (R, N, 4, S, 17) and st["spheres"].dtype == np.int64
    assert st["chunks"].shape == (R, N, 20, 8) and st["chunks"].dtype == np.float16 and st["demo"].shape == (N, 20, 8) and st["demo"].dtype == np.float32
    for r, plain in enumerate(world.plain):
        assert _same(st["image"][r], plain.image), r  # every row, the padded last batch's one among them
        assert _same(st["spheres"][r], plain.spheres), r
        for unit in ("norm", "rad"):
            assert st["generated"][unit].shape == (R, N, 20, 2) and _same(st["generated"][unit][r], plain.actions["generated"][unit]), (r, unit)
        assert _same(st["chunks"][r], plain.chunks["generated"]), r
    assert not _same(st["image"][0], st["image"][1]) and not _same(st["chunks"][1], st["chunks"][2]), "the seeds draw different noise"
    assert (st["spheres"][:, ..., 5:9] == st["spheres"][:1, ..., 5:9]).all() and (st["spheres"][..., 0] == st["spheres"][:1, ..., 0]).all()
    # the demo table: the normalised chunk of every transition, as the replay samples it
    rp = world.ev.replay
    for start in range(0, N, BATCH):
        idx = world.ev.batch_indices(start)
        n_valid = min(BATCH, N - start)
        assert np.array_equal(st["demo"][start: start + n_valid], rp.sample(idx)["action"][:n_valid].cpu().numpy())


def test_the_result_outside_the_seed_block_is_the_run_without_seeds(world):
    res, plain = world.res, world.plain[0]
    bare = world.evaluator().run()  # no option at all
    for other in (plain, bare):
        assert _same(res.image, other.image) and _same(res.spheres, other.spheres) and set(res.actions) == set(other.actions) == {"generated", "oracle"}
        assert list(res.actions) == list(other.actions)
        for name in ("generated", "oracle"):
            for unit in ("norm", "rad"):
                assert _same(res.actions[name][unit], other.actions[name][unit]), (name, unit)
        assert res.summary() == other.summary()
    assert bare.seeds is None and bare.seed_tables is None and bare.seed_summary() is None and bare.chunks is None
    # the options that read the first seed's tables report what they report without a seed axis
    assert _same(res.points, plain.points) and _same(res.orientation, plain.orientation)
    assert list(res.chunks) == list(plain.chunks) and all(_same(res.chunks[k], plain.chunks[k]) for k in plain.chunks)
    for kind in ("generated", "oracle"):
        a, b = res.executions[0][kind], plain.executions[0][kind]
        assert _same(a["actions"], b["actions"]) and _same(a["n_calls"], b["n_calls"]) and all(_same(a["scores"][u], b["scores"][u]) for u in ("norm", "rad"))
    assert res.execution_summary() == plain.execution_summary() and res.triangulation_summary() == plain.triangulation_summary()
    assert res.orientation_summary() == plain.orientation_summary()
    # slice 0 IS the existing table
    assert np.shares_memory(res.image, res.seed_tables["image"]) and np.shares_memory(res.spheres, res.seed_tables["spheres"])


def test_the_reductions_equal_the_restatements_on_the_read_back_tables(world):
    res, st = world.res, world.res.seed_tables
    want, bound = SS.seed_spheres(st["spheres"], world.ev.seed_min_ratio)
    got = res.seed_spheres
    assert got.shape == want.shape == (N, 4, res.windows.shape[2], 8) and got.dtype == np.float64
    assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(np.isnan(got), np.isnan(want))
    k = want[..., 0]
    assert (k >= 2).any() and (k == 0).any() and (got[4, ..., 0] == 0).all() and (got[12, ..., 0] == 0).all(), "the steps that draw no sphere find none"
    some = k > 0
    err = np.abs(got[some] - want[some])[:, 1:]
    print(f"seed_spheres on the run's tables: max |out - restatement| = {err.max():.3e}, max error / bound = "
          f"{(err / np.maximum(bound[some][:, 1:], 1e-300)).max():.3e}, bits equal: {_same(got[some], want[some])}")
    assert (err <= bound[some][:, 1:]).all()
    std = np.asarray(world.ev.replay.action_stats["std"], np.float64)[:7].astype(np.float32)
    for unit, scale in (("norm", None), ("rad", std)):
        got = res.seed_actions[unit]
        exact, bound = SS.seed_actions(st["chunks"], st["demo"], scale, dtype=np.float64)
        walk, _ = SS.seed_actions(st["chunks"], st["demo"], scale)
        assert got.shape == (N, 20, 4) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - exact)
        print(f"seed_actions {unit}: max error / bound = {(err[..., [0, 2, 3]] / bound[..., [0, 2, 3]]).max():.3f}, bits equal the f32 walk: {_same(got, walk)}")
        assert (err <= bound).all() and np.array_equal(got[..., 1], walk[..., 1])
        # column 3 is the seed-order f32 mean of the action kernel's own per-seed sums: the tables beside it
        total = np.zeros((N, 20), np.float32)
        for r in range(R):
            total = (total + st["generated"][unit][r][..., 0]).astype(np.float32)
        assert _same(got[..., 3], (total * np.float32(1.0 / R)).astype(np.float32)), unit


def test_seed_summary_and_json(world, tmp_path):
    res = world.res
    s = res.seed_summary()
    assert s["seeds"] == [2, 3, 4] and set(s["scores"]) == set(VALIDATOR_SCALARS) | {"joint_l1_norm", "joint_l1_rad", "gripper_acc"}
    for r, plain in enumerate(world.plain):
        sm = plain.summary()
        assert s["scores"]["select"]["values"][r] == sm["image"]["spheres"]["score"], r
        assert s["scores"]["wrapped_mse"]["values"][r] == sm["image"]["wrapped_mse"] and s["scores"]["joint_l1_rad"]["values"][r] == sm["generated"]["joint_l1_rad"]
    e = s["scores"]["select"]
    assert e["std"] == pytest.approx(np.std(e["values"], ddof=1), rel=1e-12) and e["std"] > 0 and e["min"] <= e["mean"] <= e["max"]
    o = s["spheres"]["overall"]
    want = SS.sphere_block(res.seed_spheres, R)
    assert o["n"] == want["n"] > 0 and all(o[k] == pytest.approx(want[k], rel=1e-12) for k in want)
    assert 0.0 <= o["variance_share"] <= 1.0 + 1e-12 and o["rms_shift_px"] <= o["worst_px"] and set(s["spheres"]["per_camera"]) == set(CAMS)
    for unit in ("norm", "rad"):
        a, want = s["actions"][unit], SS.action_block(res.seed_actions[unit], 7)
        assert all(a[k] == pytest.approx(want[k], rel=1e-12) for k in want)
        assert a["seed_mean"] <= a["mean_of_seeds"] and 0.0 <= a["gain"] <= 1.0 and a["spread"] > 0
        # the mean over the seeds of each seed's own score, two ways
        assert a["mean_of_seeds"] == pytest.approx(s["scores"][f"joint_l1_{unit}"]["mean"], rel=1e-5)
    js = res.to_json(str(tmp_path / "s.json"))
    assert js["seeds"] == s and {"executions", "spheres_3d", "orientation"} <= set(js)
    assert {k: v for k, v in js.items() if k not in ("seeds", "executions", "spheres_3d", "orientation")} == res.summary()
    with open(tmp_path / "s.json") as f:
        assert json.load(f) == json.loads(json.dumps(js))


def test_a_second_run_gives_the_same_bits(world):
    again, res = world.ev.run(), world.res
    for k in ("image", "spheres", "chunks", "demo"):
        assert _same(again.seed_tables[k], res.seed_tables[k]), k
    for unit in ("norm", "rad"):
        assert _same(again.seed_tables["generated"][unit], res.seed_tables["generated"][unit]) and _same(again.seed_actions[unit], res.seed_actions[unit])
    assert _same(again.seed_spheres, res.seed_spheres) and again.seed_summary() == res.seed_summary()


def test_the_diffusion_only_mode_has_no_action_block(world):
    only = world.evaluator(controller=None, seeds=R).run()
    st = world.res.seed_tables
    assert only.actions == {} and only.seed_actions is None and set(only.seed_tables) == {"image", "spheres"} and only.seeds == [2, 3, 4]
    assert _same(only.seed_tables["image"], st["image"]) and _same(only.seed_tables["spheres"], st["spheres"])
    assert _same(only.seed_spheres, world.res.seed_spheres)
    s = only.seed_summary()
    assert "actions" not in s and set(s["scores"]) == set(VALIDATOR_SCALARS) and s["spheres"] == world.res.seed_summary()["spheres"]
    assert s["scores"]["select"] == world.res.seed_summary()["scores"]["select"]


def test_refusals(world):
    for bad in (0, 1, 65, 2.5):
        with pytest.raises(ValueError, match="OpenLoopEval: seeds is None or the number of generator seeds"):
            world.evaluator(seeds=bad)
    with pytest.raises(ValueError, match="without a diffusion agent nothing is generated"):
        OpenLoopEval(None, world.controller, world.eps, CAMS, render_cfg=world.cfg, stats=_stats(), tokenizer=RR.tokens, batch_size=BATCH, seeds=3)


def test_diffusion_validator_with_seeds(world, engine, tmp_path):
    kw = dict(render_cfg=world.cfg, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine)
    without = diffusion_validator(lambda: world.dagent.pipe, world.eps, CAMS, **kw)(500)
    line = diffusion_validator(lambda: world.dagent.pipe, world.eps, CAMS, out_dir=str(tmp_path), seeds=2, **kw)(500)
    assert set(line) - set(without) == {"select_mean", "select_std", "variance_share"} and {k: line[k] for k in without} == without
    assert line["select"] == world.res.summary()["image"]["spheres"]["score"]
    values = world.res.seed_summary()["scores"]["select"]["values"][:2]
    assert line["select_mean"] == pytest.approx(np.mean(values), rel=1e-12) and line["select_std"] == pytest.approx(np.std(values, ddof=1), rel=1e-12)
    assert line["select_std"] > 0 and 0.0 <= line["variance_share"] <= 1.0 + 1e-12
    with open(os.path.join(str(tmp_path), "validation.jsonl")) as f:
        assert [json.loads(l) for l in f] == [line]
