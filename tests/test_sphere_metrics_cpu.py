"""Host side of the per-sphere open-loop scores: ``render.sphere_windows`` on hand-built cameras (every number below is worked out by hand
from the projection include/genima_hip.h states; radii and offsets are binary fractions, so the f32 tables hold them exactly), the derived
accessors and ``summary()["image"]["spheres"]`` of ``OpenLoopResult`` on a hand-written table, the unchanged summary without a sphere table,
and ``diffusion_validator``'s line on a stub evaluator."""
import json
import os

import numpy as np
import pytest

import sphere_metrics_ref as SR
from genima_amd import openloop
from genima_amd import render as R
from genima_amd.openloop import OpenLoopResult


def _cam(f=100.0, c=32.0, pose=None, znear=0.125, zfar=3.0):
    cam = np.zeros(18, np.float32)
    cam[:4] = (f, f, c, c)
    cam[4:16] = (np.eye(3, 4) if pose is None else np.asarray(pose, np.float64)).reshape(-1)
    cam[16:] = (znear, zfar)
    return cam


def _spheres(centres, radii):
    sph = np.zeros((len(centres), 16), np.float32)
    for i, (c, r) in enumerate(zip(centres, radii)):
        sph[i, :12] = np.eye(3, 4).reshape(-1)
        sph[i, [3, 7, 11]] = c
        sph[i, 12] = r
    return sph


def test_windows_of_a_hand_built_camera():
    # the camera at the origin looks along -z, y up; fx = fy = 100, centre (32, 32), 64 x 64; radius 1/16 at depth 1 -> r_px = 6.25, h = 12.5
    centres = [(0, 0, -1),             # on the optical axis: u = v = 32 -> floor(19.5) .. ceil(44.5)
               (-0.3125, 0.3125, -1),  # u = 32 - 31.25 = 0.75, v = 32 - 31.25 = 0.75 (y up -> towards row 0): clipped at the top-left corner
               (0, 0, 1),              # behind the camera: z = -1
               (0, 0, -4),             # beyond zfar = 3
               (0, 0, -1),             # radius 1 / 128: scale r_px = 1.5625 < min_half -> h = 3
               (2, 0, -1),             # u = 232: the clipped window is empty
               (0, 0, -1)]             # s >= count
    radii = [0.0625, 0.0625, 0.0625, 0.0625, 1 / 128, 0.0625, 0.0625]
    win = R.sphere_windows(_cam(), _spheres(centres, radii), np.int32(6), 64, 64)
    assert win.dtype == np.int32 and win.shape == (7, 4)
    assert win.tolist() == [[19, 19, 45, 45], [0, 0, 14, 14], [0, 0, 0, 0], [0, 0, 0, 0], [29, 29, 35, 35], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert R.sphere_windows(_cam(), _spheres(centres, radii), np.int32(0), 64, 64).tolist() == [[0, 0, 0, 0]] * 7
    # scale and min_half are arguments: scale 1 -> h = 6.25; min_half 8 then decides
    assert R.sphere_windows(_cam(), _spheres(centres[:1], radii[:1]), np.int32(1), 64, 64, scale=1.0).tolist() == [[25, 25, 39, 39]]
    assert R.sphere_windows(_cam(), _spheres(centres[:1], radii[:1]), np.int32(1), 64, 64, scale=1.0, min_half=8.0).tolist() == [[24, 24, 40, 40]]
    # the cap: radius 1 at depth 1 -> scale r_px = 200 -> h = 127 around (256, 256): 254 pixels a side, inside the kernel's 256
    big = R.sphere_windows(_cam(c=256.0), _spheres([(0, 0, -1)], [1.0]), np.int32(1), 512, 512)
    assert big.tolist() == [[129, 129, 383, 383]]
    # H and W are separate: the same sphere in a 40-row, 64-column image is clipped at the bottom only
    assert R.sphere_windows(_cam(), _spheres(centres[:1], radii[:1]), np.int32(1), 40, 64).tolist() == [[19, 19, 45, 40]]


def test_windows_follow_the_camera_pose_and_batch_shape():
    # R = diag(1, -1, -1) (the camera looks along world +z, y down), t = (0.5, 0, 0): c - t = (0.125, 0.125, 1) -> p = (0.125, -0.125, -1), z = 1
    pose = np.array([[1, 0, 0, 0.5], [0, -1, 0, 0], [0, 0, -1, 0]], np.float64)
    centres, radii = [(0.625, 0.125, 1.0)], [0.0625]
    # u = 32 + 12.5 = 44.5, v = 32 + 12.5 = 44.5, h = 12.5: floor(32) .. ceil(57)
    assert R.sphere_windows(_cam(pose=pose), _spheres(centres, radii), np.int32(1), 64, 64).tolist() == [[32, 32, 57, 57]]
    # leading dimensions [N, V] pass through; count is per view
    cams = np.stack([_cam(), _cam(pose=pose)])[None].repeat(2, axis=0)
    sph = np.stack([_spheres([(0, 0, -1)], [0.0625]), _spheres(centres, radii)])[None].repeat(2, axis=0)
    win = R.sphere_windows(cams, sph, np.array([[1, 1], [1, 0]], np.int32), 64, 64)
    assert win.shape == (2, 2, 1, 4) and win[:, :, 0].tolist() == [[[19, 19, 45, 45], [32, 32, 57, 57]], [[19, 19, 45, 45], [0, 0, 0, 0]]]


def _table():
    """1 transition, cameras front / wrist, S = 3.  front: A (found, shifted by (3, -4), spread doubled), B (no generated mass), C (undrawn,
    with spurious generated mass); wrist: D (gen == gt, no occupied pixel), two empty windows."""
    sph = np.zeros((1, 2, 3, 17), np.int64)
    win = np.zeros((1, 2, 3, 4), np.int32)
    #             area  gen: m  mx  my  mr2   gt: m  mx   my   mr2  n_occ se  gen rgb       gt rgb
    sph[0, 0, 0] = [100, 10, 50, 40, 450, 20, 40, 160, 1380, 4, 77, 40, 80, 120, 44, 72, 120]
    sph[0, 0, 1] = [48, 0, 0, 0, 0, 5, 10, 15, 100, 2, 9, 20, 20, 20, 30, 10, 20]
    sph[0, 0, 2] = [36, 7, 7, 7, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    sph[0, 1, 0] = [64, 8, 16, 24, 200, 8, 16, 24, 200, 0, 0, 0, 0, 0, 0, 0, 0]
    win[0, 0] = [[0, 0, 10, 10], [2, 3, 8, 11], [10, 10, 16, 16]]
    win[0, 1, 0] = [4, 4, 12, 12]
    return sph, win


def _result(spheres=None, windows=None):
    image = np.zeros((1, 2, 5), np.int64)
    image[0, 0], image[0, 1] = [3 * 4 * 4, 4, 3 * 12 * 1, 12, 48], [0, 0, 3 * 16 * 9, 16, 96]
    return OpenLoopResult(image, {}, [0], [0], [0], ["a"], ["front", "wrist"], 2, 4, 4, spheres=spheres, windows=windows)


def test_accessors_on_a_hand_written_table():
    sph, win = _table()
    res = _result(sph, win)
    nan = np.nan
    shift, mass, spread, colour = res.sphere_shift(), res.sphere_mass_ratio(), res.sphere_spread_ratio(), res.sphere_colour_l1()
    for a in (shift, mass, spread, colour):
        assert a.shape == (1, 2, 3) and a.dtype == np.float64
    # A: centroids (5, 4) and (2, 8) -> 5 px; spreads sqrt(45 - 25 - 16) = 2 and sqrt(69 - 4 - 64) = 1; colour (4 + 8 + 0) / 3 / 4
    # B: no generated mass -> NaN shift and spread ratio, mass ratio 0; colour (10 + 10 + 0) / 3 / 2.  C: undrawn -> NaN everywhere
    np.testing.assert_array_equal(shift[0], [[5.0, nan, nan], [0.0, nan, nan]])
    np.testing.assert_array_equal(mass[0], [[0.5, 0.0, nan], [1.0, nan, nan]])
    np.testing.assert_array_equal(spread[0], [[2.0, nan, nan], [1.0, nan, nan]])
    np.testing.assert_array_equal(colour[0], [[1.0, 10.0 / 3.0, nan], [nan, nan, nan]])
    assert res.sphere_drawn()[0].tolist() == [[True, True, False], [True, False, False]]
    # the restatement derives the same values
    d = SR.derived(sph)
    for name, got in (("shift", shift), ("mass_ratio", mass), ("spread_ratio", spread), ("colour_l1", colour)):
        np.testing.assert_array_equal(d[name], got)


def test_summary_block_counts_a_missing_sphere_and_skips_an_undrawn_one(tmp_path):
    sph, win = _table()
    res = _result(sph, win)
    s = res.summary()
    sp = s["image"]["spheres"]
    assert sp["n_drawn"] == {"front": 2, "wrist": 1}  # C is excluded although the generated image changed its window
    assert sp["found_rate"] == {"front": 0.5, "wrist": 1.0}  # A's ratio 0.5 meets the default found_mass, B's 0 does not
    assert sp["shift_px"] == {"front": 5.0, "wrist": 0.0} and sp["mass_ratio"] == {"front": 0.25, "wrist": 1.0}
    assert sp["spread_ratio"] == {"front": 2.0, "wrist": 1.0} and sp["colour_l1"] == {"front": (1.0 + 10.0 / 3.0) / 2, "wrist": None}
    # score: A's 5 px, B's penalty -- half the diagonal of its 6 x 8 window = 5 --, D's 0
    assert sp["score"] == (5.0 + 5.0 + 0.0) / 3
    assert sp["overall"] == {"n_drawn": 3, "found_rate": 2 / 3, "shift_px": 2.5, "mass_ratio": 0.5, "spread_ratio": 1.5, "colour_l1": (1.0 + 10.0 / 3.0) / 2}
    assert res.summary(found_mass=0.6)["image"]["spheres"]["found_rate"] == {"front": 0.0, "wrist": 1.0}
    assert json.loads(json.dumps(res.to_json(str(tmp_path / "s.json")))) == json.load(open(tmp_path / "s.json"))
    # nothing drawn at all: counts 0, every mean None
    none = _result(np.zeros_like(sph), win).summary()["image"]["spheres"]
    assert none["score"] is None and none["n_drawn"] == {"front": 0, "wrist": 0} and none["found_rate"] == {"front": None, "wrist": None}
    with pytest.raises(ValueError, match="windows"):
        _result(sph, None)


def test_result_without_a_sphere_table_summarises_as_before():
    res = _result()
    s = res.summary()
    assert res.spheres is None and res.windows is None
    assert s == {"n": 1, "image": {"sphere_rmse": {"front": 2.0, "wrist": None}, "sphere_missing": {"front": 0, "wrist": 1},
                                   "background_rmse": {"front": 1.0, "wrist": 3.0}, "wrapped_mse": (48 + 96) / (2 * 4 * 4 * 3)},
                 "cameras": ["front", "wrist"], "tasks": ["a"]}
    # ... and with one, only the new block is added
    sph, win = _table()
    with_block = _result(sph, win).summary()
    block = with_block["image"].pop("spheres")
    assert with_block == s and set(block) == {"n_drawn", "found_rate", "shift_px", "mass_ratio", "spread_ratio", "colour_l1", "overall", "score"}


def test_diffusion_validator_line_on_a_stub_evaluator(tmp_path, monkeypatch):
    sph, win = _table()
    built, pipes = [], []

    class StubEval:
        def __init__(self, agent, controller, episodes, cameras, **kw):
            built.append((agent, controller, episodes, tuple(cameras), kw))
            self.agent = agent

        def run(self):
            return _result(sph, win)

    def make_pipe():
        pipes.append(object())
        return pipes[-1]

    monkeypatch.setattr(openloop, "OpenLoopEval", StubEval)
    out = str(tmp_path / "val")
    validate = openloop.diffusion_validator(make_pipe, ["ep0"], ("front", "wrist"), render_cfg="cfg", out_dir=out, tokenizer="tok", batch_size=3,
                                            num_inference_steps=2, seed=9, engine="E")
    first, second = validate(100), validate(200)
    want = {"step": 100, "select": 10.0 / 3.0, "found_rate": 2 / 3, "shift_px": 2.5, "mass_ratio": 0.5, "spread_ratio": 1.5,
            "colour_l1": (1.0 + 10.0 / 3.0) / 2, "sphere_rmse": 2.0, "background_rmse": 2.0, "wrapped_mse": (48 + 96) / (2 * 4 * 4 * 3), "n": 1}
    assert first == want and second == dict(want, step=200)
    lines = [json.loads(l) for l in open(os.path.join(out, "validation.jsonl"))]
    assert lines == [first, second]
    # the evaluator is built once, diffusion-only, without statistics; every call wraps a fresh pipeline
    assert len(built) == 1 and len(pipes) == 2
    agent, controller, episodes, cameras, kw = built[0]
    assert controller is None and episodes == ["ep0"] and cameras == ("front", "wrist") and agent.pipe is pipes[0]
    assert kw == dict(render_cfg="cfg", stats=None, tokenizer="tok", batch_size=3, num_inference_steps=2, seed=9, engine="E")
    # without out_dir nothing is written
    assert openloop.diffusion_validator(make_pipe, ["ep0"], ("front", "wrist"), render_cfg="cfg")(7)["step"] == 7
    assert sorted(os.listdir(tmp_path)) == ["val"]
