"""``OpenLoopResult``'s summaries against a recorded text: one result that carries every optional table, built from closed-form integer
expressions, must serialise to exactly ``tests/golden/openloop_summary.json`` -- the text the summaries gave before their shared pieces (the
per-camera assembly, the per-task wrapper, the guarded divide) were written once."""
import json
import os

import numpy as np

from genima_amd.openloop import OpenLoopResult, orientation_candidates

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "openloop_summary.json")
N, V, S, G, K, T, A = 6, 2, 3, 3, 5, 4, 8
EPISODE, STEP, TASK = [0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 0, 1], [0, 0, 0, 0, 1, 1]  # two episodes of four and two steps, one task each


def _ramp(shape, mod, div=1.0, dtype=np.float32):
    n = int(np.prod(shape))
    return ((np.arange(n) * 7 + 3) % mod / div).astype(dtype).reshape(shape)


def build_result() -> OpenLoopResult:
    image = (_ramp((N, V, 5), 97, dtype=np.int64) + 10) * np.array([40, 1, 90, 8, 300])
    image[4:, 1, 1] = 0  # the second task draws no sphere into the second camera: its sphere_rmse there is None
    actions = {kind: {"norm": np.stack([_ramp((N, T), 13 + k, 8.0), _ramp((N, T), 2)], -1), "rad": np.stack([_ramp((N, T), 11 + k, 4.0), _ramp((N, T), 2)], -1)}
               for k, kind in enumerate(("generated", "oracle"))}
    # ---- the sphere table: mass, mass * centroid, mass * (centroid^2 + spread^2) per side, the occupied pixels and the colour sums
    i = np.arange(N * V * S).reshape(N, V, S)
    sph = np.zeros((N, V, S, 17), np.int64)
    for o, (m, cx, cy, r2) in ((1, (20 + i % 7, 10 + i % 5, 12 + i % 3, 4 + i % 4)), (5, (22 + i % 6, 11 + i % 4, 12 + i % 5, 5 + i % 3))):
        sph[..., o], sph[..., o + 1], sph[..., o + 2], sph[..., o + 3] = m, m * cx, m * cy, m * (cx * cx + cy * cy + r2)
    sph[..., 0], sph[..., 9], sph[..., 10] = 144, 15 + i % 6, 900 + 17 * i
    sph[..., 11:14], sph[..., 14:17] = (i[..., None] * 5 + np.arange(3)) % 256 * 9, (i[..., None] * 3 + 2 * np.arange(3)) % 256 * 11
    sph[2, 1, 2, 5:9] = 0  # an undrawn sphere
    sph[4, 0, 0, 1:5] = 0  # a drawn sphere with no generated mass: not found, the penalty branches
    sph[1, 0, 1, 9] = 0  # no occupied pixel: the colour is NaN
    sph[3, 1, 0, 8] = sph[3, 1, 0, 5] * ((11 + i[3, 1, 0] % 4) ** 2 + (12 + i[3, 1, 0] % 5) ** 2)  # a true spread of 0: the spread ratio is NaN
    x0, y0, k = 5 + i % 9, 7 + i % 4, 1 + i % 3
    windows = np.stack([x0, y0, x0 + 6 * k, y0 + 8 * k], -1).astype(np.int32)  # diagonals of 10, 20 and 30 pixels
    # ---- one execution mode, both row kinds
    ex = {"h": 3, "temporal_agg": True, "m": 0.01, "K": 2}
    for k, kind in enumerate(("generated", "oracle")):
        ex[kind] = {"actions": _ramp((N, A), 17 + k, 16.0), "n_calls": (1 + (np.arange(N) + k) % 2).astype(np.int32),
                    "scores": {"norm": _ramp((N, 4), 19 + k, 8.0), "rad": _ramp((N, 4), 23 + k, 4.0)}}
    chunks = {kind: _ramp((N, T, A), 29 + k, 32.0, np.float16) for k, kind in enumerate(("generated", "oracle"))}
    # ---- the triangulation: group g of transition n, kind 0 generated, kind 1 ground truth
    n_, g_ = np.meshgrid(np.arange(N), np.arange(G), indexing="ij")
    points = np.zeros((N, G, 2, 8), np.float64)
    for kind in (0, 1):
        points[:, :, kind, 0] = 2
        points[:, :, kind, 1:4] = np.stack([n_ + g_, n_ - g_, 2 * g_ + 1], -1) / 8.0
        points[:, :, kind, 4] = (3 + (n_ + 2 * g_ + 4 * kind) % 5) / 1024.0
        points[:, :, kind, 5], points[:, :, kind, 6], points[:, :, kind, 7] = (1 + (n_ + g_) % 3) / 2048.0, (2 + (n_ * g_) % 4) / 4.0, 0.5
    points[1, 2, 0, 1:7], points[1, 2, 0, 0] = np.nan, 1  # the generated image shows the group to one view only: unsolved, the penalty
    points[3, 0, 0, 1:7], points[3, 0, 0, 0] = np.nan, 0  # ... and this one to none
    points[5, 0, :, 1:7], points[5, 0, :, 0] = np.nan, 1  # the ground truth draws it into one view only: not a group to ask of
    points[2, 1, 1, 1:7] = np.nan  # rays that do not cross in the ground truth: solved in neither row's "both"
    point_slots = ((n_ + g_)[..., None] + np.arange(V)) % S
    point_slots = point_slots.astype(np.int32)
    point_slots[1, 2, 1] = point_slots[5, 0, 0] = -1
    point_slots[4, 1] = -1  # a group no view shows
    point_centres = np.stack([g_ - 1, n_ % 2, g_ % 2], -1) / 8.0
    cams = np.zeros((N, V, 18), np.float32)
    cams[..., 0], cams[..., 1] = np.array([64.0, -128.0]), 64.0  # fx per view (a mirrored one among them), fy
    cams[..., 4], cams[..., 9], cams[..., 14] = 1.0, 1.0, 1.0  # R = I
    cams[..., 7], cams[..., 11], cams[..., 15] = 0.25, -0.125, 1.5 + np.arange(V) / 2.0  # t
    # ---- the orientation curves: a parabola about candidate i % K for the generated window, about the identity for the ground truth
    angles, _ = orientation_candidates(K, 40.0)
    c = np.arange(K)
    orient = np.zeros((N, V, S, K, 4), np.int64)
    orient[..., 0], orient[..., 1] = 1000 + 50 * (c - (i % K)[..., None]) ** 2 + 3 * i[..., None], 60 + i[..., None] % 4
    orient[..., 2], orient[..., 3] = 10 * (c - K // 2) ** 2, 64
    orient[0, 1, 1, :, 2] = 77  # a flat ground-truth curve: the sphere's texture is hidden, unreadable
    orient[3, 0, 2, :, 1] = 20  # found and readable, but too few pixels to score
    orient[5, 1, 0, :, 0] = 500  # a flat generated curve: no contrast, the first candidate wins (an edge)
    return OpenLoopResult(image, actions, EPISODE, STEP, TASK, ["push", "reach"], ["front", "wrist"], A - 1, 16, 16, spheres=sph, windows=windows,
                          executions=[ex], chunks=chunks, points=points, point_slots=point_slots, point_centres=point_centres, cams=cams,
                          orientation=orient, orientation_angles=angles)


def test_every_summary_serialises_to_the_recorded_text(tmp_path):
    res = build_result()
    got = json.dumps(res.to_json(str(tmp_path / "summary.json")), sort_keys=True)
    with open(GOLDEN) as f:
        assert got == f.read().strip()  # as text, so that NaN tokens compare equal


def test_the_result_takes_every_branch_the_summaries_have(tmp_path):
    """What the builder claims to exercise is there: without it the recorded text would pin less than it says."""
    res = build_result()
    s = res.to_json(str(tmp_path / "summary.json"))
    sp, tri, ori, ex = s["image"]["spheres"], s["spheres_3d"], s["orientation"], s["executions"][0]
    assert set(s["per_task"]) == {"push", "reach"} and s["per_task"]["reach"]["image"]["sphere_rmse"]["wrist"] is None
    assert s["image"]["sphere_missing"] == {"front": 0, "wrist": 2}
    assert sp["overall"]["n_drawn"] == N * V * S - 1 and sp["overall"]["found_rate"] < 1.0 and np.isnan(res.sphere_shift()[4, 0, 0])
    assert np.isnan(res.sphere_colour_l1()[1, 0, 1]) and np.isnan(res.sphere_spread_ratio()[3, 1, 0])
    assert sp["score"] > sp["overall"]["shift_px"]  # the sphere without generated mass counts as half its window's diagonal
    assert tri["n_groups"] == N * G - 1 and tri["generated"]["solved_rate"] < tri["ground_truth"]["solved_rate"] < 1.0
    assert np.isnan(res.point_penalty()[4, 1]) and tri["score_mm"] > tri["generated"]["err_mm"]
    assert ori["overall"]["n_unreadable"] == 1 and ori["overall"]["n_scored"] == N * V * S - 4 and ori["overall"]["floor_deg"] == 0.0
    assert ori["overall"]["at_edge"] > 0 and ori["score_deg"] > ori["overall"]["err_deg"]
    assert ex["per_task"]["reach"]["oracle"]["by_position"]["joint_l1_norm"][2] is None and ex["per_task"]["reach"]["generated"]["jump_boundary_norm"] is None
    assert ex["oracle"]["jump_boundary_norm"] is not None and ex["calls_per_step"] == 1.0 / 3
