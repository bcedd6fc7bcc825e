"""-m "not gpu": the orientation read-out of the open-loop evaluation (``gn_openloop_orientation``, ``OpenLoopEval(orientation=)``) without
a device: the candidate rotations' known answers, the recovery of a planted rotation from f64 renders through the numpy restatement of the
kernel's sums (tests/orientation_ref.py), ``orientation_summary`` on a hand-made table, and the entry point's declaration, binding and flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import orientation_ref as OF
import render_reference as ref
from genima_amd import _lib, build
from genima_amd import render as R
from genima_amd.openloop import ORIENTATION_COLUMNS, OpenLoopResult, orientation_candidates, parse_orientation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTURES = os.path.join(ROOT, "tests", "golden", "sphere_textures")


def test_candidates_known_answers():
    ang, rot = orientation_candidates()
    assert ang.dtype == np.float64 and rot.dtype == np.float32 and ang.shape == (37,) and rot.shape == (37, 9) and rot.flags.c_contiguous
    assert np.array_equal(ang, np.arange(-90.0, 91.0, 5.0)) and ang[18] == 0.0
    assert np.array_equal(rot[18].view(np.uint32), np.eye(3, dtype=np.float32).reshape(9).view(np.uint32))  # the exact identity, no -0
    # +-90 degrees about z: x -> +-y
    z90 = np.float32(np.cos(np.pi / 2))
    assert np.array_equal(rot[36], np.array([z90, -1, 0, 1, z90, 0, 0, 0, 1], np.float32))
    assert np.array_equal(rot[0], np.array([z90, 1, 0, -1, z90, 0, 0, 0, 1], np.float32))
    for r in rot.astype(np.float64).reshape(-1, 3, 3):
        assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-7 and abs(np.linalg.det(r) - 1.0) <= 1e-7
    # another axis and span: a third of a turn about (1, 1, 1) cycles the axes
    ang, rot = orientation_candidates(3, 240.0, axis=(2, 2, 2))
    assert np.array_equal(ang, [-120.0, 0.0, 120.0])
    assert np.abs(rot[2].reshape(3, 3).astype(np.float64) - np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]])).max() <= 1e-7
    assert np.abs(rot[0].reshape(3, 3).astype(np.float64) - np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]])).max() <= 1e-7
    ang, rot = orientation_candidates(1, 0.0)
    assert np.array_equal(ang, [0.0]) and np.array_equal(rot, np.eye(3, dtype=np.float32).reshape(1, 9))
    for bad in (dict(K=4), dict(K=0), dict(K=65), dict(K=5, span_deg=0.0), dict(K=5, span_deg=400.0), dict(axis=(0, 0, 0)), dict(axis=(1, 0))):
        with pytest.raises(ValueError):
            orientation_candidates(**bad)
    assert parse_orientation("37") == {"K": 37} and parse_orientation("25, 60") == {"K": 25, "span_deg": 60.0}
    for bad in ("", "a", "5,b", "5,6,7"):
        with pytest.raises(ValueError):
            parse_orientation(bad)


def test_compose_is_the_stated_f64_sum_and_the_identity_changes_nothing():
    sph = ref.scene(4, B=2, H=32, W=32)["spheres"]
    _, rot = orientation_candidates(5, 40.0)
    assert np.array_equal(OF.compose(sph[0], 1, rot[2]), sph[0])  # the identity row: the ground-truth pose, exactly
    got = OF.compose(sph[1], 2, rot[4])
    Rs = sph[1, 2, :12].reshape(3, 4)[:, :3].astype(np.float64)
    want = (Rs @ rot[4].reshape(3, 3).astype(np.float64)).astype(np.float32)  # products of f32 values are exact in f64: only the sum's order could differ
    assert np.abs(got[2, :12].reshape(3, 4)[:, :3].astype(np.float64) - want).max() <= 2 ** -23
    keep = np.ones((4, 16), bool)
    keep[2, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = False
    assert np.array_equal(got[keep], sph[1][keep])  # every other sphere, the centre, the radius and the factor stay


def _window_costs(views, atlas, b, s, win, rot, planted):
    """Window s of view b, drawn by tests/render_reference.py in f64 with 4 samples.  Only the window is drawn: a camera whose principal
    point is moved by the window's corner casts the same rays through the same pixels (pixel + offset - cx is exact in f64 either way).
    -> None for a window with fewer than 100 occupied pixels, else per planted rotation the int64 [K, 4] sums of the candidates against a
    ``gen`` that is the view with sphere s turned by it."""
    x0, y0, wd, ht = win
    cam = views["cams"][b].astype(np.float64)
    cam[2] -= x0
    cam[3] -= y0

    def draw(table):
        return ref.render(cam, table, views["tex_index"][b], views["count"][b], atlas, ht, wd, 4)[0]

    gt = draw(views["spheres"][b])
    occ = (gt != 255).any(axis=-1)
    if occ.sum() < 100:
        return None
    S = views["spheres"].shape[1]
    cand = np.zeros((1, S, len(rot), ht, wd, 3), np.uint8)
    cand[0, s] = np.stack([draw(OF.compose(views["spheres"][b], s, r)) for r in rot])
    local = np.zeros((1, S, 4), np.int32)
    local[0, s] = (0, 0, wd, ht)
    return [OF.orientation_sums(cand, draw(OF.compose(views["spheres"][b], s, p))[None], gt[None], occ[None], local)[0, s] for p in planted]


def test_a_planted_rotation_is_recovered_on_the_grid():
    """128 x 128, seeds 1 - 3, 4 samples: rotate one sphere by 7 and by -13 degrees about its z and search a 5 degree grid over +-30.  Every
    window with at least 100 occupied pixels whose own sphere is visible (a non-flat ground-truth curve) returns the nearest grid angle; the
    windows whose sphere is hidden behind a neighbour have an identically zero ground-truth curve and are reported unreadable."""
    H = W = 128
    atlas = R.load_atlas(TEXTURES)
    ang, rot = orientation_candidates(13, 60.0)
    assert np.array_equal(ang, np.arange(-30.0, 31.0, 5.0))
    plant = {7.0: 5.0, -13.0: -15.0}
    planted = [orientation_candidates(3, 2.0 * abs(a))[1][2 if a > 0 else 0] for a in plant]
    n_windows = n_readable = n_flat = 0
    for seed in (1, 2, 3):
        views = ref.scene(seed, B=8, H=H, W=W)
        wins = R.sphere_windows(views["cams"], views["spheres"], views["count"], H, W)
        for b in range(8):
            for s in range(int(views["count"][b])):
                tabs = _window_costs(views, atlas, b, s, OF.clamp_window(wins[b, s], H, W), rot, planted)
                for tab, nearest in zip(tabs or (), plant.values()):
                    n_windows += 1
                    assert (tab[:, 1] == tab[0, 1]).all() and (tab[:, 3] == tab[0, 3]).all() and tab[0, 1] == tab[0, 3] >= 100
                    assert tab[6, 2] == 0  # the identity candidate is the ground truth
                    if tab[:, 2].max() == tab[:, 2].min():  # flat: the window's own sphere is not visible
                        n_flat += 1
                        assert (tab[:, 2] == 0).all(), (seed, b, s)
                        continue
                    n_readable += 1
                    assert ang[int(np.argmin(tab[:, 0] / tab[:, 1]))] == nearest, (seed, b, s, nearest, tab[:, 0].tolist())
                    assert ang[int(np.argmin(tab[:, 2] / tab[:, 3]))] == 0.0
    print(f"windows {n_windows}, readable {n_readable}, flat {n_flat}")
    assert (n_windows, n_readable, n_flat) == (102, 98, 4)  # the count the feature was proposed on


def _hand_made():
    """One transition, cameras a and b, three slots, five candidates at 10 degree steps."""
    ang = np.array([-20.0, -10.0, 0.0, 10.0, 20.0])
    sph = np.zeros((1, 2, 3, 17), np.int64)
    ori = np.zeros((1, 2, 3, 5, 4), np.int64)
    gt_curve = np.array([300, 100, 0, 100, 300])

    def put(v, s, gen_m, gt_m, se_gen, n, se_gt):
        sph[0, v, s, 1], sph[0, v, s, 5] = gen_m, gt_m
        ori[0, v, s, :, 0], ori[0, v, s, :, 1], ori[0, v, s, :, 2], ori[0, v, s, :, 3] = se_gen, n, se_gt, n

    put(0, 0, 10, 10, [400, 300, 200, 100, 200], 100, gt_curve)    # scored: the minimum at +10
    put(0, 1, 1, 10, [5, 4, 3, 4, 5], 100, gt_curve)               # drawn, not found: counts as half the span
    put(0, 2, 10, 10, [9, 8, 7, 8, 9], 100, 0)                     # found, but its ground-truth curve is flat: unreadable
    put(1, 0, 10, 10, [100, 200, 300, 400, 500], 100, gt_curve)    # scored: the minimum at the first candidate, an edge
    put(1, 1, 10, 10, [50, 40, 30, 40, 50], 10, gt_curve)          # found and readable, but 10 pixels: left out
    put(1, 2, 10, 0, [1, 2, 3, 4, 5], 100, gt_curve)               # not drawn
    return OpenLoopResult(None, {}, [0], [0], [0], ["t"], ["a", "b"], 7, 64, 64, spheres=sph, windows=np.zeros((1, 2, 3, 4), np.int32),
                          orientation=ori, orientation_angles=ang)


def test_orientation_summary_on_a_hand_made_table():
    res = _hand_made()
    sc = res.orientation_scores()
    assert sc["scored"].tolist() == [[[True, False, False], [True, False, False]]]
    assert sc["readable"].tolist() == [[[True, True, False], [True, True, True]]]
    assert sc["err_deg"][0, 0, 0] == 10.0 and sc["err_deg"][0, 1, 0] == 20.0 and np.isnan(sc["err_deg"][0, 0, 1])
    assert sc["at_edge"][0, 0, 0] == 0.0 and sc["at_edge"][0, 1, 0] == 1.0
    assert sc["contrast"][0, 0, 0] == 1.0 - 1.0 / 2.4 and sc["contrast"][0, 1, 0] == 1.0 - 1.0 / 3.0
    assert sc["floor_deg"][0, 0, 0] == 0.0 and np.isnan(sc["floor_deg"][0, 0, 2]) and np.isnan(sc["floor_deg"][0, 1, 2])
    s = res.orientation_summary()
    o = s["overall"]
    assert o["n_scored"] == 2 and o["n_unreadable"] == 1 and o["err_deg"] == 15.0 and o["err_median_deg"] == 15.0 and o["within_step"] == 0.5
    assert o["at_edge"] == 0.5 and o["floor_deg"] == 0.0 and o["contrast"] == ((1.0 - 1.0 / 2.4) + (1.0 - 1.0 / 3.0)) / 2.0
    assert s["n_scored"] == {"a": 1, "b": 1} and s["n_unreadable"] == {"a": 1, "b": 0} and s["err_deg"] == {"a": 10.0, "b": 20.0}
    assert s["within_step"] == {"a": 1.0, "b": 0.0} and s["at_edge"] == {"a": 0.0, "b": 1.0}
    assert s["score_deg"] == (10.0 + 20.0 + 20.0) / 3.0  # the +10 sphere, the unfound one at half the 40 degree span, the edge one
    assert s["angles_deg"] == [-20.0, -10.0, 0.0, 10.0, 20.0] and "per_task" not in s
    # a lower pixel bar scores the small sphere too: its minimum is at 0
    assert res.orientation_summary(min_pixels=10)["overall"]["n_scored"] == 3 and res.orientation_summary(min_pixels=10)["err_deg"]["b"] == 10.0
    # a lower mass bar finds the faint sphere: its minimum is at 0, and nothing counts as half the span any more
    assert res.orientation_summary(found_mass=0.1)["score_deg"] == (10.0 + 0.0 + 20.0) / 3.0
    assert ORIENTATION_COLUMNS == ("se_gen", "n_gen", "se_gt", "n_gt")
    none = OpenLoopResult(None, {}, [0], [0], [0], ["t"], ["a", "b"], 7, 64, 64)
    assert none.orientation is None and none.orientation_summary() is None
    with pytest.raises(ValueError, match="orientation comes with"):
        OpenLoopResult(None, {}, [0], [0], [0], ["t"], ["a", "b"], 7, 64, 64, orientation=res.orientation, orientation_angles=res.orientation_angles)


def test_the_evaluator_refuses_the_option_without_a_diffusion_agent_or_with_a_bad_value():
    import types

    from genima_amd.openloop import OpenLoopEval

    controller = types.SimpleNamespace(execution=None, config={"frame_stack": 1, "num_queries": 20}, device="cuda")
    with pytest.raises(ValueError, match="orientation reads the generated spheres"):
        OpenLoopEval(None, controller, [], render_cfg=None, stats=({}, {}), orientation=7)
    for bad in (True, "7", 7.0, dict(K=7, steps=3), 8, dict(K=7, span_deg=-1.0)):
        with pytest.raises(ValueError):
            OpenLoopEval(None, controller, [], render_cfg=None, stats=({}, {}), orientation=bad)


def test_entry_point_is_declared_bound_and_built_without_contraction():
    header = open(os.path.join(ROOT, "include", "genima_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int32_t\s+gn_openloop_orientation\s*\(([^;]*)\)\s*;", decl)
    assert m, "include/genima_hip.h does not declare gn_openloop_orientation"
    args = [a.strip() for a in m.group(1).split(",")]
    res, bound = _lib.SIGNATURES["gn_openloop_orientation"]
    assert res is ctypes.c_int32 and len(args) == len(bound) == 28
    for a, t in zip(args, bound):  # pointers first, then the int32 sizes: the binding's types follow the declaration's
        assert ("*" in a) == (t is ctypes.c_void_p) and (t is ctypes.c_void_p or (a.startswith("int32_t ") and t is ctypes.c_int32)), a
    assert "openloop_orient.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["openloop_orient.hip"]
    assert build.EXTRA_FLAGS["openloop_orient.hip"] == build.EXTRA_FLAGS["render.hip"]
    assert os.path.exists(os.path.join(build.CSRC, "openloop_orient.hip"))
    build.build(verbose=False)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "gn_openloop_orientation")
