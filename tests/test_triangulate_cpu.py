"""-m "not gpu": the triangulation rule of ``gn_openloop_triangulate`` on the CPU -- tests/triangulate_ref.py on exact projections through
``render.synthetic_episode``'s cameras, the group tables (``openloop.sphere_groups`` against the reference's own construction), degenerate
inputs, the FLOOR of the method on the rendered synthetic episode, ``OpenLoopResult.triangulation_summary`` on hand-built tables and the
``OpenLoopEval`` argument checks that need no device.

The floor scene: ``render.synthetic_episode(L=9, seed=7, action_horizon=4)`` at 256 x 256 with every camera scale set to 1 (why: see the
floor test), the four tiled cameras, steps 0, 3 and 6, drawn by tests/render_reference.py over the episode's random frames, summed by
tests/sphere_metrics_ref.py with threshold 30."""
import json
import types

import numpy as np
import pytest

import render_reference as RF
import replay_render_ref as RR
import sphere_metrics_ref as SR
import triangulate_ref as TR
from genima_amd import render as R
from genima_amd.openloop import POINT_COLUMNS, OpenLoopEval, OpenLoopResult, sphere_groups
from genima_amd.replay import DEFAULT_CAMERAS as CAMS

SPLIT_JOINTS = {"wrist": [1, 3], "front": [3, 5], "right_shoulder": [5], "left_shoulder": [], "overhead": []}  # joint 1 is drawn in one view only


def _tables(cfg, traj, steps):
    views = [R.pack_views(R.pack_step(traj, cfg, ts, CAMS)) for ts in steps]
    tab = {k: np.stack([v[k] for v in views]) for k in ("cams", "spheres", "tex_index", "count")}
    win = R.sphere_windows(tab["cams"], tab["spheres"], tab["count"], cfg.image_height, cfg.image_width)
    return tab, win


def _episode(joints=None):
    cfg, traj, frames = R.synthetic_episode(9, seed=7, texture_dir=RR.GOLDEN_SPHERES, action_horizon=4)
    if joints is not None:
        cfg.joints = joints
    return cfg, traj, frames


def _exact_observations(tab, win):
    N, V, S = win.shape[:3]
    return [[[TR.observe(tab["cams"][n, v], tab["spheres"][n, v, s, [3, 7, 11]]) if s < tab["count"][n, v] and win[n, v, s].any() else None
              for s in range(S)] for v in range(V)] for n in range(N)]


@pytest.mark.parametrize("joints", [None, SPLIT_JOINTS], ids=["default", "per_camera_joints"])
def test_exact_projections_are_recovered(joints):
    cfg, traj, _ = _episode(joints)
    tab, win = _tables(cfg, traj, range(9))
    slot, centre = TR.group_tables(tab["spheres"], tab["count"], win)
    mine = sphere_groups(tab["spheres"], tab["count"], win)
    assert np.array_equal(mine[0], slot) and np.array_equal(mine[1], centre) and mine[0].dtype == np.int32 and mine[1].dtype == np.float64
    assert slot.shape == (9, 4, 4) and (slot[7:] == -1).all()  # the gripper and three joints; the last two steps draw nothing
    # every slot the table names holds the group's own centre, and every drawn sphere with a window is named once
    for n, g, v in zip(*np.nonzero(slot >= 0)):
        assert np.array_equal(tab["spheres"][n, v, slot[n, g, v], [3, 7, 11]].astype(np.float64), centre[n, g])
    assert (slot >= 0).sum() == sum(win[n, v, s].any() for n in range(9) for v in range(4) for s in range(tab["count"][n, v]))
    if joints is not None:  # left_shoulder draws the gripper alone; wrist slot 2 and front slot 1 are the same joint
        assert (tab["count"][:7] == [1, 2, 3, 3]).all()
        assert (slot[:7, 0] >= 0).sum(axis=-1).min() >= 2 and ((slot[:7, 1:] >= 0).sum(axis=-1) <= 2).all()
    sph, w = TR.table_from_observations(_exact_observations(tab, win))
    assert np.array_equal(w[..., :2] >= 0, np.ones(w.shape[:-1] + (2,), bool))
    out = TR.triangulate(sph, w, tab["cams"], slot, centre)
    seen = (slot >= 0).sum(axis=-1)
    assert np.array_equal(out[:, :, 1, 0], seen) and np.array_equal(out[:, :, 0], out[:, :, 1], equal_nan=True)
    solved = ~np.isnan(out[:, :, 1, 4])
    assert np.array_equal(solved, seen >= 2) and solved.sum() >= 20  # one view alone never solves: joint 1 of the split config stays NaN
    if joints is not None:
        assert (seen == 1).any()
    print(f"exact projections: max error {out[:, :, 1, 4][solved].max():.3e} m, max ray residual {out[:, :, 1, 5][solved].max():.3e} m, "
          f"max reprojection {out[:, :, 1, 6][solved].max():.3e} px, min det {out[:, :, 1, 7][solved].min():.3e}")
    assert out[:, :, 1, 4][solved].max() <= 1e-9 and out[:, :, 1, 5][solved].max() <= 1e-9
    # the reprojection column uses R^T where the observations were made with R^-1: an f32 rotation is orthonormal to about 2e-7, times |f| = 352 px
    assert out[:, :, 1, 6][solved].max() <= 1e-4
    assert np.abs(out[:, :, 1, 1:4][solved] - centre[solved]).max() <= 1e-9
    assert (out[:, :, 1, 7][solved] > 1e-3).all() and (out[:, :, 1, 7][solved] <= 1.0).all()
    assert np.isnan(out[:, :, :, 1:7][~solved]).all() and (out[:, :, 1, 7][seen < 2] == 0).all()


def test_degenerate_inputs_are_unsolved():
    cfg, traj, _ = _episode()
    tab, win = _tables(cfg, traj, [0])
    cams = np.repeat(tab["cams"], 3, axis=0)  # three copies of step 0
    cams[2, 1] = cams[2, 0]
    cams[2, 1, [7, 11, 15]] += cams[2, 0, 4:16].reshape(3, 4)[:, :3] @ np.array([0.05, 0.02, 0.0], np.float32)  # view 1 = view 0 moved sideways
    point = tab["spheres"][0, 0, 0, [3, 7, 11]].astype(np.float64)
    centre = np.tile(point, (3, 1, 1))
    slot = np.full((3, 1, 4), -1, np.int32)
    slot[0, 0, 2] = 0             # one used view
    slot[1, 0, :2] = 0            # two views, but the second has no ground-truth mass
    slot[2, 0, :2] = 0            # two views sharing one ray direction: the same pixel seen from two positions with one orientation
    obs = [[[TR.observe(cams[n, v], point)] for v in range(4)] for n in range(3)]
    obs[2][1][0] = obs[2][0][0]
    sph, w = TR.table_from_observations(obs, S=1)
    sph[1, 1, 0, 5:9] = 0
    out = TR.triangulate(sph, w, cams, slot, centre)
    assert out[0, 0, 1, 0] == 1 and out[1, 0, 1, 0] == 1 and out[2, 0, 1, 0] == 2
    assert out[0, 0, 1, 7] == 0 and out[1, 0, 1, 7] == 0 and abs(out[2, 0, 1, 7]) <= 1e-12
    assert np.isnan(out[:, 0, :, 1:7]).all() and np.array_equal(out[:, 0, 0, [0, 7]], out[:, 0, 1, [0, 7]])


def _floor(scales):
    cfg, traj, frames = _episode()
    if scales is not None:
        cfg.camera_scales = scales
    steps = [0, 3, 6]
    tab, win = _tables(cfg, traj, steps)
    H, W = cfg.image_height, cfg.image_width
    atlas = R.load_atlas(RR.GOLDEN_SPHERES)
    cond = np.stack([[frames[c][ts] for c in CAMS] for ts in steps])
    full, occ = np.zeros_like(cond), np.zeros(cond.shape[:-1], np.uint8)
    for n in range(len(steps)):
        for v in range(4):
            img, _ = RF.render(tab["cams"][n, v], tab["spheres"][n, v], tab["tex_index"][n, v], tab["count"][n, v], atlas, H, W, cfg.samples)
            full[n, v], _, o = RF.composite(img, cond[n, v])
            occ[n, v] = o
    sph = SR.sphere_metrics(full, full, cond, occ, win, 30)
    slot, centre = TR.group_tables(tab["spheres"], tab["count"], win)
    return types.SimpleNamespace(cfg=cfg, tab=tab, win=win, sph=sph, slot=slot, centre=centre, out=TR.triangulate(sph, win, tab["cams"], slot, centre))


@pytest.fixture(scope="module")
def floor():
    return _floor((1.0,) * 5)


def _floor_figures(f, what):
    out = f.out
    solved = ~np.isnan(out[:, :, 1, 4])
    err, ray, px = (out[:, :, 1, k][solved] for k in (4, 5, 6))
    print(f"floor, {what}, over {int(solved.sum())} groups: error mean {err.mean() * 1e3:.2f} mm, median {np.median(err) * 1e3:.2f} mm, max {err.max() * 1e3:.2f} mm; "
          f"ray residual mean {ray.mean() * 1e3:.2f} mm; reprojection mean {px.mean():.2f} px; min det {out[:, :, 1, 7][solved].min():.3f}")
    multi = (f.slot >= 0).sum(axis=-1) >= 2
    assert multi.sum() >= 9 and np.array_equal(solved, multi)  # every group drawn in at least two views with non-empty windows is solved
    assert np.array_equal(out[:, :, 0], out[:, :, 1], equal_nan=True)  # gen = gt here: the two kinds see the same sums
    return solved


def test_the_floor_of_the_method_on_the_rendered_episode(floor):
    """The ground-truth row: the spheres as the renderer drew them, triangulated from their own centroids.  What is left is the method's bias
    (the centroid of change is not the projection of the centre), the number DESIGN.md quotes.

    The scene is the synthetic episode with every camera scale 1: each sphere is drawn with its nominal radius of 10 mm, about 4 px, and the
    windows of a view stay apart.  With render.yaml's scales (3 - 8) the same episode does NOT meet the radius condition: its seven joints lie
    within 0.15 m of the gripper while a sphere is up to 80 mm in radius, so the 2 r windows of a view overlap, a neighbour's mass enters
    every sum and the floor is 36 - 43 mm (seeds 7 - 10 alike) against a smallest radius of 30 mm -- see the next test."""
    out, slot = floor.out, floor.slot
    solved = _floor_figures(floor, "camera scales 1")
    # smaller than the sphere's own radius: the smallest radius any view that shows the group draws it with
    radius = floor.tab["spheres"][..., 12].astype(np.float64)  # [N, V, S]
    for n, g in zip(*np.nonzero(solved)):
        r = min(radius[n, v, slot[n, g, v]] for v in range(4) if slot[n, g, v] >= 0)
        assert out[n, g, 1, 4] < r, (n, g, out[n, g, 1, 4], r)


def test_the_crowded_scene_is_solved_too():
    """render.yaml's camera scales on the same episode: the windows overlap and the floor is tens of millimetres (printed; DESIGN.md quotes it
    as the reason the ground-truth row has to be read beside the generated one).  Asserted: every group seen twice is solved."""
    _floor_figures(_floor(None), "render.yaml's camera scales")


def _result(points, slot, centre, win, cams, tasks=("t",), task=None):
    N = len(points)
    return OpenLoopResult(None, {}, [0] * N, list(range(N)), [0] * N if task is None else task, list(tasks), list(CAMS), 7, 256, 256,
                          spheres=np.zeros(win.shape[:3] + (17,), np.int64), windows=win, points=points, point_slots=slot, point_centres=centre, cams=cams)


def test_triangulation_summary_on_known_tables(floor, tmp_path):
    """Generated observations: the ground truth's, but every view of group 0 moved by (+2, -1) px, view 0 of group 1 missing, and group 2 gone
    from every view."""
    f = floor
    obs = _exact_observations(f.tab, f.win)
    gen = [[list(v) for v in n] for n in obs]
    N, G, V = f.slot.shape
    for n in range(N):
        for v in range(V):
            s = f.slot[n, 0, v]
            if s >= 0:
                gen[n][v][s] = (obs[n][v][s][0] + 2.0, obs[n][v][s][1] - 1.0)
            if f.slot[n, 2, v] >= 0:
                gen[n][v][f.slot[n, 2, v]] = None
        first = int(np.nonzero(f.slot[n, 1] >= 0)[0][0])
        gen[n][first][f.slot[n, 1, first]] = None
    sph, w = TR.table_from_observations(obs, gen)
    points = TR.triangulate(sph, w, f.tab["cams"], f.slot, f.centre)
    res = _result(points, f.slot, f.centre, w, f.tab["cams"])
    s = res.triangulation_summary()
    multi = (f.slot >= 0).sum(axis=-1) >= 2
    assert s["n_groups"] == int(multi.sum()) and "per_task" not in s
    assert s["ground_truth"]["solved_rate"] == 1.0 and s["ground_truth"]["err_mm"] <= 1e-6 and s["ground_truth"]["views"] == (f.slot >= 0).sum(axis=-1)[multi].mean()
    gen_solved = multi & ~np.isnan(points[:, :, 0, 4])
    assert not gen_solved[:, 2].any() and gen_solved[:, 0].all()
    assert s["generated"]["solved_rate"] == gen_solved.sum() / multi.sum() < 1.0
    assert abs(s["generated"]["err_mm"] - points[:, :, 0, 4][gen_solved].mean() * 1e3) <= 1e-9
    assert s["generated"]["err_median_mm"] == float(np.median(points[:, :, 0, 4][gen_solved]) * 1e3)
    assert abs(s["excess_mm"] - (points[:, :, 0, 4] - points[:, :, 1, 4])[gen_solved].mean() * 1e3) <= 1e-9 and s["excess_mm"] > 0.5
    assert s["generated"]["reproj_px"] > s["ground_truth"]["reproj_px"] and s["generated"]["views"] < s["ground_truth"]["views"]
    # the penalty, one group by hand: half the 12 x 12 window's diagonal at the depth of each view that shows it
    n, g = 0, 2
    terms = []
    for v in range(V):
        if f.slot[n, g, v] >= 0:
            cam = f.tab["cams"][n, v].astype(np.float64)
            pose = cam[4:16].reshape(3, 4)
            z = -(pose[:, :3].T @ (f.centre[n, g] - pose[:, 3]))[2]
            terms.append(0.5 * np.hypot(12, 12) * z / abs(cam[0]))
    pen = res.point_penalty()
    assert abs(pen[n, g] - np.mean(terms)) <= 1e-12 and np.isnan(pen[(f.slot >= 0).sum(axis=-1) == 0]).all()
    scored = np.where(gen_solved, points[:, :, 0, 4], pen)[multi]
    assert abs(s["score_mm"] - scored.mean() * 1e3) <= 1e-9 and s["score_mm"] > s["generated"]["err_mm"]
    # two tasks: per_task blocks over each task's own rows
    two = _result(points, f.slot, f.centre, w, f.tab["cams"], tasks=("a", "b"), task=[0, 1, 1]).triangulation_summary()
    assert set(two["per_task"]) == {"a", "b"} and two["per_task"]["a"]["n_groups"] + two["per_task"]["b"]["n_groups"] == two["n_groups"]
    # to_json: the key appears only with points, and summary() does not change
    with_points = res.to_json(str(tmp_path / "a.json"))
    without = OpenLoopResult(None, {}, [0] * N, list(range(N)), [0] * N, ["t"], list(CAMS), 7, 256, 256, spheres=res.spheres, windows=w)
    assert without.triangulation_summary() is None
    plain = without.to_json(str(tmp_path / "b.json"))
    assert "spheres_3d" not in plain and plain == without.summary() == res.summary()
    assert with_points == dict(plain, spheres_3d=s) and json.load(open(tmp_path / "a.json"))["spheres_3d"]["n_groups"] == s["n_groups"]
    assert len(POINT_COLUMNS) == 8
    with pytest.raises(ValueError, match="points come with"):
        OpenLoopResult(None, {}, [0], [0], [0], ["t"], list(CAMS), 7, 256, 256, points=points[:1])


def test_setup_errors_need_no_device():
    cfg, traj, _ = _episode()
    controller = types.SimpleNamespace(execution=None, config={"num_queries": 4, "frame_stack": 1, "action_dim": 8}, device="cpu")
    with pytest.raises(ValueError, match="triangulate places the generated spheres"):
        OpenLoopEval(None, controller, [], CAMS, render_cfg=cfg, stats=({}, {}), triangulate=True)
    agent = types.SimpleNamespace(pipe=types.SimpleNamespace(device="cpu"))
    for kw in (dict(tri_min_det=0.0), dict(tri_min_det=-1e-6), dict(tri_min_det=float("nan")), dict(tri_min_ratio=-0.1), dict(tri_min_ratio=float("nan"))):
        with pytest.raises(ValueError, match="tri_min_ratio"):
            OpenLoopEval(agent, None, [], CAMS, render_cfg=cfg, stats=None, engine=object(), triangulate=True, **kw)
    # more distinct spheres in one transition than the kernel's G
    sph = np.zeros((1, 2, 8, 16), np.float32)
    sph[0, 0, :, 3], sph[0, 1, :, 3] = np.arange(8), np.arange(8) + 4
    with pytest.raises(ValueError, match="at most 8"):
        sphere_groups(sph, np.full((1, 2), 8), np.ones((1, 2, 8, 4), np.int32))
    slot, centre = sphere_groups(sph[:, :, :4], np.array([[4, 0]]), np.ones((1, 2, 4, 4), np.int32))
    assert slot.shape == (1, 4, 2) and slot[0].tolist() == [[0, -1], [1, -1], [2, -1], [3, -1]] and centre[0, :, 0].tolist() == [0, 1, 2, 3]
    empty = sphere_groups(np.zeros((2, 4, 4, 16), np.float32), np.zeros((2, 4), np.int32), np.zeros((2, 4, 4, 4), np.int32))
    assert empty[0].shape == (2, 1, 4) and (empty[0] == -1).all() and (empty[1] == 0).all()
