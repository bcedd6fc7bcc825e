"""-m "not gpu": the host side of the open-loop scores over several seeds -- the identities the two reductions satisfy (on the numpy
restatements of tests/seed_spread_ref.py, which the GPU tests hold the kernels to), ``OpenLoopResult.seed_summary`` on hand-built tables,
``summary()`` untouched by the seed axis, the ABI names, the option's refusals before any device work, ``diffusion_validator``'s line on a stub
evaluator and the command line's ``--seeds``."""
import ctypes
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest

import seed_spread_ref as SS
from genima_amd import _lib, build, openloop
from genima_amd.openloop import OpenLoopEval, OpenLoopResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_openloop_seed_spheres", "gn_openloop_seed_actions")


def _sphere_tables(R, N, V, S, seed):
    """Random sphere tables [R, N, V, S, 17] whose ground-truth columns agree across the seeds; some generated masses are 0 or small."""
    rng = np.random.default_rng(seed)
    t = np.zeros((R, N, V, S, 17), np.int64)
    gt_m = rng.integers(0, 5000, (N, V, S)) * (rng.random((N, V, S)) > 0.15)
    t[:, ..., 5] = gt_m
    t[:, ..., 6], t[:, ..., 7] = (gt_m * rng.uniform(0, 60, (N, V, S))).astype(np.int64), (gt_m * rng.uniform(0, 60, (N, V, S))).astype(np.int64)
    gen_m = (gt_m[None] * rng.uniform(0.0, 1.6, (R, N, V, S))).astype(np.int64) * (rng.random((R, N, V, S)) > 0.1)
    t[..., 1] = gen_m
    t[..., 2], t[..., 3] = (gen_m * rng.uniform(0, 60, (R, N, V, S))).astype(np.int64), (gen_m * rng.uniform(0, 60, (R, N, V, S))).astype(np.int64)
    return t


def _chunks(R, N, T, A, ld, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2, 2, (R, N, T, ld)).astype(np.float16)
    c[..., A:] = np.inf  # pad columns: never read
    demo = rng.uniform(-2, 2, (N, T, A)).astype(np.float32)
    demo[..., A - 1] = rng.random((N, T)) > 0.5
    return c, demo


@pytest.mark.parametrize("R", [2, 5, 64])
def test_squared_shift_is_squared_bias_plus_spread(R):
    """[4] = [1]^2 + [2]^2 + [3]: the mean squared distance from the truth is the squared distance of the mean plus the variance."""
    out, bound = SS.seed_spheres(_sphere_tables(R, 7, 4, 3, seed=R), 0.5)
    k = out[..., 0]
    some = k > 0
    assert some.any() and (k == 0).any() and ((k > 0) & (k < R)).any()
    assert np.isnan(out[~some][:, 1:]).all() and np.isfinite(out[some]).all()
    lhs, rhs = out[some][:, 4], out[some][:, 1] ** 2 + out[some][:, 2] ** 2 + out[some][:, 3]
    # each of [4], [3] and [1]^2 + [2]^2 lies within (R + 8) 2^-53 M of its exact value (seed_spread_ref's squared-deviation count: M is
    # 4 / k sum_r (|c_r| + |m| + |ct|)^2, the bound of columns 3 and 4), and the exact values satisfy the identity: three such terms
    tol = 3.0 * bound[some][:, 4]
    print(f"R={R}: max |[4] - ([1]^2 + [2]^2 + [3])| / bound = {(np.abs(lhs - rhs) / tol).max():.3e}")
    assert (np.abs(lhs - rhs) <= tol).all()
    assert (out[some][:, 7] >= out[some][:, 4] * (1 - 1e-15)).all(), "the largest squared shift is at least the mean one"
    one = out[k == 1]
    assert (len(one) or R == 64) and (one[:, 3] == 0).all() and (one[:, 6] == 0).all(), "one found seed: it is its own mean"


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("R", [2, 3, 16])
def test_seed_mean_error_lies_between_the_triangle_bounds(R, scaled):
    """[0] <= [3] (the error of the mean is at most the mean of the errors, by convexity) and [0] >= [3] - [2] (the triangle inequality
    |a_r - d| <= |a_r - mean| + |mean - d|, averaged over the seeds)."""
    A = 8
    chunks, demo = _chunks(R, 5, 20, A, 16, seed=10 + R)
    scale = np.linspace(0.25, 3.0, A - 1).astype(np.float32) if scaled else None
    out, bound = SS.seed_actions(chunks, demo, scale)
    o = out.astype(np.float64)
    # every column lies within its (R + A + 8) 2^-24 M of the exact rule (seed_spread_ref: R + A + 3 roundings for columns 0 and 3, the
    # deviation count with its factor 2 for column 2), and the exact values satisfy both inequalities: the slack is the sum of the bounds
    upper = o[..., 3] + bound[..., 0] + bound[..., 3] - o[..., 0]
    lower = o[..., 0] - (o[..., 3] - o[..., 2]) + bound[..., 0] + bound[..., 2] + bound[..., 3]
    print(f"R={R} scaled={scaled}: min slack of [0] <= [3]: {upper.min():.3e}; of [0] >= [3] - [2]: {lower.min():.3e}; "
          f"largest bound {bound.max():.3e}")
    assert (upper >= 0).all() and (lower >= 0).all()
    assert (o[..., 2] > 0).all() and set(np.unique(o[..., 1])) <= {0.0, 1.0}
    # the f32 walk against the f64 rule: inside the bound it is asserted with on the device
    exact, _ = SS.seed_actions(chunks, demo, scale, dtype=np.float64)
    err = np.abs(o - exact)
    print(f"   f32 order against the f64 rule: max error / bound = {(err[..., [0, 2, 3]] / bound[..., [0, 2, 3]]).max():.3f}")
    assert (err <= bound).all()


def test_one_seed_has_no_spread():
    chunks, demo = _chunks(1, 5, 20, 8, 8, seed=3)
    scale = np.linspace(0.5, 2.0, 7).astype(np.float32)
    for s in (None, scale):
        out, _ = SS.seed_actions(chunks, demo, s)
        assert np.array_equal(out[..., 0].view(np.int32), out[..., 3].view(np.int32)) and (out[..., 2] == 0).all()
        assert np.array_equal(out[..., 3].view(np.int32), SS.action_l1(chunks[0], demo, s).view(np.int32))
    t = _sphere_tables(1, 7, 4, 3, seed=4)
    out, _ = SS.seed_spheres(t, 0.5)
    found = out[..., 0] == 1
    assert found.any() and (out[found][:, 3] == 0).all() and (out[found][:, 6] == 0).all()
    assert np.array_equal(out[found][:, 4], out[found][:, 1] ** 2 + out[found][:, 2] ** 2) and np.array_equal(out[found][:, 7], out[found][:, 4])


def test_found_rule_is_the_triangulation_rule_with_its_boundary():
    t = np.zeros((3, 1, 2, 1, 17), np.int64)
    t[:, 0, 0, 0, 5:8] = [10, 50, 40]
    t[0, 0, 0, 0, 1:4] = [5, 10, 20]  # exactly min_ratio * gt_m: found
    t[1, 0, 0, 0, 1:4] = [4, 40, 40]  # below: not found
    t[2, 0, 0, 0, 1:4] = [20, 160, 80]
    out, _ = SS.seed_spheres(t, 0.5)
    assert out[0, 0, 0].tolist() == [2.0, 0.0, 0.0, 9.0, 9.0, 1.25, 0.5625, 9.0]  # centroids (2, 4) and (8, 4) about the truth (5, 4)
    assert out[0, 1, 0, 0] == 0 and np.isnan(out[0, 1, 0, 1:]).all()  # gt_m = 0: hidden
    assert SS.seed_spheres(t, 0.0)[0][0, 0, 0, 0] == 3 and SS.seed_spheres(t, 0.51)[0][0, 0, 0, 0] == 1


# ---- OpenLoopResult.seed_summary on hand-built tables -----------------------------------------------------------------------------------------
def _hand():
    """R = 2 (seeds 7, 8), one transition, cameras front / wrist, S = 2, T = 2, A = 3 (two joints).
    front 0: truth (5, 4); the seeds land at (8, 4) and (2, 4) with mass ratios 1 and 0.5 -> no bias, spread 9.
    front 1: truth (2, 2); both seeds land at (5, 2) -> bias (3, 0), no spread.
    wrist 0: the second seed's mass ratio is 0.125: one found seed.  wrist 1: hidden."""
    sph = np.zeros((2, 1, 2, 2, 17), np.int64)
    sph[:, 0, 0, 0, 5:9], sph[:, 0, 0, 1, 5:9], sph[:, 0, 1, 0, 5:9] = [10, 50, 40, 500], [4, 8, 8, 40], [8, 16, 24, 200]
    sph[0, 0, 0, 0, 1:5], sph[1, 0, 0, 0, 1:5] = [10, 80, 40, 900], [5, 10, 20, 150]
    sph[0, 0, 0, 1, 1:5] = sph[1, 0, 0, 1, 1:5] = [4, 20, 8, 150]
    sph[0, 0, 1, 0, 1:5], sph[1, 0, 1, 0, 1:5] = [8, 16, 24, 200], [1, 2, 3, 20]
    sph[..., 0], sph[..., 9] = 100, 4
    sph[0, ..., 10], sph[1, ..., 10] = 48, 12
    win = np.zeros((1, 2, 2, 4), np.int32)
    win[0, :, :] = [0, 0, 6, 8]
    image = np.zeros((2, 1, 2, 5), np.int64)
    image[0, 0], image[1, 0] = [[48, 4, 36, 12, 48], [0, 0, 432, 16, 96]], [[192, 4, 144, 12, 24], [12, 1, 15, 15, 48]]
    chunks = np.array([[[[1, 2, 1], [0, 0, 2]]], [[[3, 2, -3], [2, 4, 2]]]], np.float16)  # [R, N, T, A]
    demo = np.array([[[2, 0, 1], [1, 1, 0]]], np.float32)
    scale = np.array([0.5, 2.0], np.float32)
    gen = {u: np.stack([np.stack([SS.action_l1(chunks[r], demo, s), ((chunks[r, ..., 2] > 0) == (demo[..., 2] > 0.5)).astype(np.float32)], axis=-1)
                        for r in range(2)]) for u, s in (("norm", None), ("rad", scale))}
    tables = {"image": image, "spheres": sph, "generated": gen, "chunks": chunks, "demo": demo}
    res = OpenLoopResult(image[0], {"generated": {u: t[0] for u, t in gen.items()}, "oracle": {u: t[1] for u, t in gen.items()}}, [0], [0], [0], ["a"],
                         ["front", "wrist"], 2, 4, 4, spheres=sph[0], windows=win, seeds=[7, 8], seed_tables=tables,
                         seed_spheres=SS.seed_spheres(sph, 0.5)[0], seed_actions={u: SS.seed_actions(chunks, demo, s)[0] for u, s in (("norm", None), ("rad", scale))})
    return res, tables, win


def test_seed_summary_on_hand_built_tables(tmp_path):
    res, tables, win = _hand()
    s = res.seed_summary()
    assert s["seeds"] == [7, 8]
    o = s["spheres"]["overall"]
    assert o == {"n": 2, "found_all_rate": 1.0, "bias_px": 1.5, "spread_px": np.sqrt(4.5), "rms_shift_px": 3.0, "variance_share": 0.5,
                 "mass_ratio_std": np.sqrt(0.0625 / 2), "worst_px": 3.0}
    assert s["spheres"]["per_camera"]["front"] == o and s["spheres"]["per_camera"]["wrist"]["n"] == 0
    assert s["spheres"]["per_camera"]["wrist"]["variance_share"] is None
    for name, sel in (("overall", None), ("front", np.arange(2)[None, :, None] == np.zeros((1, 2, 2), int))):
        want = SS.sphere_block(res.seed_spheres, 2, sel)
        got = o if name == "overall" else s["spheres"]["per_camera"][name]
        assert got.keys() == want.keys() and all(got[k] == pytest.approx(want[k], rel=1e-14) for k in got)
    # t = 0: the seeds' chunks (1, 2 | 1) and (3, 2 | -3) average to (2, 2 | -1) against the demo's (2, 0 | 1): seed-mean error 2, each seed's 3,
    # deviation 1, and the mean logit closes a gripper the demo opens.  t = 1: (0, 0 | 2), (2, 4 | 2) -> (1, 2 | 2) against (1, 1 | 0): 1; 2 and 4; 3
    assert res.seed_actions["norm"][0].tolist() == [[2.0, 0.0, 1.0, 3.0], [1.0, 0.0, 3.0, 3.0]]
    a = s["actions"]["norm"]
    assert a == {"mean_of_seeds": 1.5, "seed_mean": 0.75, "gain": 0.5, "spread": 1.0, "gripper_acc_seed_mean": 0.0}
    for unit in ("norm", "rad"):
        want = SS.action_block(res.seed_actions[unit], 2)
        assert all(s["actions"][unit][k] == pytest.approx(want[k], rel=1e-14) for k in want)
    assert s["actions"]["rad"]["seed_mean"] == (0.5 * 0 + 2.0 * 2 + 0.5 * 0 + 2.0 * 1) / 2 / 2
    # the scores: the existing summary code on each seed's tables
    sc = s["scores"]
    assert set(sc) == set(openloop.VALIDATOR_SCALARS) | {"joint_l1_norm", "joint_l1_rad", "gripper_acc"}
    for r in range(2):
        alone = OpenLoopResult(tables["image"][r], {"generated": {u: t[r] for u, t in tables["generated"].items()}}, [0], [0], [0], ["a"], ["front", "wrist"], 2, 4, 4,
                               spheres=tables["spheres"][r], windows=win)
        sm = alone.summary()
        sp = sm["image"]["spheres"]
        assert sc["select"]["values"][r] == sp["score"] and sc["found_rate"]["values"][r] == sp["overall"]["found_rate"]
        assert sc["shift_px"]["values"][r] == sp["overall"]["shift_px"] and sc["wrapped_mse"]["values"][r] == sm["image"]["wrapped_mse"]
        assert sc["joint_l1_norm"]["values"][r] == sm["generated"]["joint_l1_norm"] and sc["gripper_acc"]["values"][r] == sm["generated"]["gripper_acc"]
    # seed 0: shifts 3, 3, 0 -> 2; seed 1: 3, 3 and the unfound wrist sphere is still a centroid, (2, 3) against (2, 3) -> 0
    assert sc["select"]["values"] == [2.0, 2.0] and sc["found_rate"]["values"] == [1.0, 2 / 3]
    assert sc["sphere_rmse"]["values"] == [2.0, (4.0 + 2.0) / 2]
    # to_json: a key of its own beside the summary
    js = res.to_json(str(tmp_path / "s.json"))
    assert js["seeds"] == s and {k: v for k, v in js.items() if k != "seeds"} == res.summary()
    with open(tmp_path / "s.json") as f:
        assert json.load(f) == json.loads(json.dumps(js))


def test_first_value_is_the_summarys_own_number_exactly():
    res, _, _ = _hand()
    s, sm = res.seed_summary(), res.summary()
    scal = res.validator_scalars()
    assert scal["select"] == sm["image"]["spheres"]["score"] and scal["wrapped_mse"] == sm["image"]["wrapped_mse"]
    for k in openloop.VALIDATOR_SCALARS:
        assert s["scores"][k]["values"][0] == scal[k], k
    for k in ("joint_l1_norm", "joint_l1_rad", "gripper_acc"):
        assert s["scores"][k]["values"][0] == sm["generated"][k], k
    assert res.seed_summary(found_mass=0.6)["scores"]["found_rate"]["values"] == [1.0, 1 / 3]  # the second seed's 0.5 and 0.125 fall below
    assert s["scores"]["found_rate"]["values"][0] == sm["image"]["spheres"]["overall"]["found_rate"]


def test_std_is_the_sample_standard_deviation():
    e = openloop._across([1.0, 2.0, 4.0])
    assert e["values"] == [1.0, 2.0, 4.0] and e["mean"] == 7 / 3 and e["min"] == 1.0 and e["max"] == 4.0
    assert e["std"] == pytest.approx(np.sqrt(((1 - 7 / 3) ** 2 + (2 - 7 / 3) ** 2 + (4 - 7 / 3) ** 2) / 2), rel=1e-15)  # ddof = 1: / (R - 1)
    assert e["std"] == pytest.approx(np.std([1.0, 2.0, 4.0], ddof=1), rel=1e-15) and e["std"] != pytest.approx(np.std([1.0, 2.0, 4.0]), rel=1e-3)
    want = SS.across([1.0, 2.0, 4.0])
    assert all(e[k] == pytest.approx(want[k], rel=1e-15) for k in ("mean", "std", "min", "max"))
    assert openloop._across([3.0, 5.0])["std"] == pytest.approx(np.sqrt(2.0))
    none = openloop._across([None, 2.0])  # a score that one seed does not have
    assert none == {"values": [None, 2.0], "mean": 2.0, "std": None, "min": 2.0, "max": 2.0}
    assert openloop._across([None, None])["mean"] is None


def test_result_without_seeds_has_no_new_key(tmp_path):
    res, _, win = _hand()
    plain = OpenLoopResult(res.image, res.actions, [0], [0], [0], ["a"], ["front", "wrist"], 2, 4, 4, spheres=res.spheres, windows=win)
    assert plain.seeds is None and plain.seed_tables is None and plain.seed_spheres is None and plain.seed_actions is None
    assert plain.seed_summary() is None
    js = plain.to_json(str(tmp_path / "p.json"))
    assert "seeds" not in js and js == plain.summary() and plain.summary() == res.summary()
    with pytest.raises(ValueError, match="seed_tables"):
        OpenLoopResult(res.image, res.actions, [0], [0], [0], ["a"], ["front", "wrist"], 2, 4, 4, spheres=res.spheres, windows=win, seeds=[1, 2])


# ---- the ABI, the option, the validator and the command line ------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/genima_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound by genima_amd/_lib.py"
        assert hasattr(lib, n), f"libgenima_hip.so does not export {n}"
    assert _lib.ABI_VERSION == 101 and len(_lib.DESC_CLASSES) == 11  # exports were appended, no struct changed or added
    # column 3 is openloop.hip's joint sum per seed, bit for bit: the two files are compiled under the same flags
    assert "openloop_seeds.hip" in build.SOURCES and build.EXTRA_FLAGS["openloop_seeds.hip"] == build.EXTRA_FLAGS["openloop.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(build.CSRC, "openloop_seeds.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "hipMemset" not in code and "fma" not in code and not re.search(r"\b(sqrt|exp|rsqrt|pow)[a-z0-9_]*\s*\(", code)


def test_library_refuses_without_a_context():
    lib = _lib.load()
    mem = ctypes.create_string_buffer(4096)
    buf = ctypes.c_void_p((ctypes.addressof(mem) + 63) // 64 * 64)
    assert lib.gn_openloop_seed_spheres(None, buf, buf, 0.5, 2, 1, 4, 2) != 0
    assert b"gn_openloop_seed_spheres" in lib.gn_last_error()
    assert lib.gn_openloop_seed_actions(None, buf, 8, buf, None, buf, 0.5, 2, 1, 5, 3) != 0
    assert b"gn_openloop_seed_actions" in lib.gn_last_error()


def _check(seeds, agent=True, seed_min_ratio=0.5):
    """``_check_options`` alone, on stubs: it runs before any device work."""
    ev = OpenLoopEval.__new__(OpenLoopEval)
    stub = types.SimpleNamespace(pipe=types.SimpleNamespace(device="cpu")) if agent else None
    controller = None if agent else types.SimpleNamespace(execution=None, config={"num_queries": 20}, device="cpu")
    ev._check_options(stub, controller, ("a", "b", "c", "d"), None if agent else ("s", "p"), "engine", 30, None, None, False, 0.5, 1e-6, None, seeds, seed_min_ratio)
    return ev


def test_the_option_is_checked_before_any_device_work():
    assert _check(None).seeds is None and _check(2).seeds == 2 and _check(64).seeds == 64 and _check(np.int64(3)).seeds == 3
    assert _check(None, agent=False).seeds is None
    for bad in (0, 1, 65, 2.5, -3, True, "4"):
        with pytest.raises(ValueError, match=r"OpenLoopEval: seeds is None or the number of generator seeds R, an integer in \[2, 64\]"):
            _check(bad)
    with pytest.raises(ValueError, match="OpenLoopEval: seeds repeats the generation.*without a diffusion agent nothing is generated"):
        _check(3, agent=False)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="seed_min_ratio"):
            _check(3, seed_min_ratio=bad)


def test_diffusion_validator_line_with_seeds_on_a_stub_evaluator(tmp_path, monkeypatch):
    res, _, win = _hand()
    plain = OpenLoopResult(res.image, {}, [0], [0], [0], ["a"], ["front", "wrist"], 2, 4, 4, spheres=res.spheres, windows=win)
    built = []

    class StubEval:
        def __init__(self, agent, controller, episodes, cameras, **kw):
            built.append(kw)

        def run(self):
            return res if "seeds" in built[-1] else plain

    monkeypatch.setattr(openloop, "OpenLoopEval", StubEval)
    kw = dict(render_cfg="cfg", tokenizer="tok", batch_size=3, num_inference_steps=2, seed=7, engine="E")
    without = openloop.diffusion_validator(object, ["ep0"], ("front", "wrist"), out_dir=str(tmp_path / "a"), **kw)(100)
    with_seeds = openloop.diffusion_validator(object, ["ep0"], ("front", "wrist"), out_dir=str(tmp_path / "b"), seeds=2, seed_min_ratio=0.25, **kw)(100)
    assert built[0] == dict(kw, stats=None), "without the option the evaluator is called as it was before the option existed"
    assert built[1] == dict(kw, stats=None, seeds=2, seed_min_ratio=0.25)
    assert set(with_seeds) - set(without) == {"select_mean", "select_std", "variance_share"}
    assert {k: with_seeds[k] for k in without} == without, "select and the other fields stay the first seed's"
    assert with_seeds["select_mean"] == 2.0 and with_seeds["select_std"] == 0.0 and with_seeds["variance_share"] == 0.5
    line = json.loads(open(tmp_path / "b" / "validation.jsonl").read())
    assert line == with_seeds and "select_std" not in json.loads(open(tmp_path / "a" / "validation.jsonl").read())


def test_eval_openloop_takes_seeds(capsys):
    spec = importlib.util.spec_from_file_location("eval_openloop", os.path.join(ROOT, "tools", "eval_openloop.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--dataset_root", "d", "--sd_ckpt", "s", "--no_controller"]
    assert tool.parse(base).seeds is None and tool.parse(base + ["--seeds", "4"]).seeds == 4 and tool.parse(base + ["--seeds", "4"]).seed_min_ratio == 0.5
    for bad in ("1", "65", "2.5", "x"):
        with pytest.raises(SystemExit):
            tool.parse(base + ["--seeds", bad])
    capsys.readouterr()
