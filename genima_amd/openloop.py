"""Open-loop evaluation: score a diffusion checkpoint and a controller snapshot on held-out demos without a simulator.

The reference answers "is this checkpoint good" with RLBench / CoppeliaSim success rates (controller/eval_genima.py), which are out of scope
here.  What a demo tree does give is, for every transition, the observation, the ground-truth joint target
(``gn_render_spheres`` over the observation's frames: what ``render.render_episode`` writes as ``rgb_rendered``) and the demo's action chunk.
``OpenLoopEval`` runs the body of the eval loop on every transition -- diffusion, then the controller, the device route of
``harness.control_step`` -- and scores

* the generated target against the rendered one, per camera, inside and outside the renderer's ``occupied`` mask, plus the reference's own
  wrapped-uint8 ``mse`` (``validation.normalized_error``) -- ``gn_openloop_image_metrics``;
* the predicted action chunk against the demo's, joint L1 and gripper agreement per chunk position -- ``gn_openloop_action_metrics``;
* a second controller pass on the GROUND-TRUTH target, the "oracle" row: what the controller does when the diffusion model is perfect, so the
  difference between the two rows is the diffusion model's share of the error.

* where each drawn sphere landed: per (transition, camera, sphere) the mass, centroid, spread and colour of what the generated image changed
  against the observation inside the sphere's window, beside the same of the rendered target -- ``gn_openloop_sphere_metrics`` over
  ``render.sphere_windows``.  The in-mask RMSE cannot tell a sphere drawn 6 px off from a blurred or a missing one; these can.

* optionally, what an execution mode would have executed: ``executions=[(execution_horizon, temporal_agg, m), ...]`` keeps every chunk in a
  device table and replays ``gn_action_ensemble``'s rule over it for every step of every episode -- ``gn_openloop_exec_actions``, bit for bit
  the controller's own ensembling kernel -- then scores the executed action against the demo's and measures how far it jumps from step to step
  -- ``gn_openloop_exec_metrics``.  Observations are teacher-forced, so a rollout with horizon h uses exactly the chunks of the transitions at
  steps 0, h, 2h, ... of each episode: a sweep costs a few launches per setting on top of the pass made anyway.

* optionally, where the generated spheres are in the WORLD: ``triangulate=True`` triangulates every drawn sphere across the views from the
  sphere table's centroids after the last batch -- ``gn_openloop_triangulate`` -- and compares the point with the sphere's true centre: the
  error in metres and the cross-view residuals (do the four tiles agree on one arm pose?), for the generated image and for the ground-truth
  render, whose row is the floor of the method.

* optionally, which ORIENTATION the generated spheres show: ``orientation=K`` re-draws every true sphere at K candidate rotations about its own
  z axis and sums the squared error of each against the generated window -- ``gn_openloop_orientation`` -- so ``orientation_summary()`` can say
  at which angle the generated stripes fit best and how sharply.  The stripe texture is the only place the image carries a joint's rotation;
  every other sphere score is blind to it.

* optionally, how much of all that is the SEED: ``seeds=R`` repeats the generation with R generator seeds, keeps the tables per seed and
  reduces over the seed axis on the device -- ``gn_openloop_seed_spheres`` (per sphere: the bias of the seeds' mean centroid, their spread
  about it) and ``gn_openloop_seed_actions`` (the error of the seed-mean chunk beside the mean of the seeds' errors) -- so ``seed_summary()``
  can give every score's seed-to-seed standard deviation, the noise floor a checkpoint difference has to beat, and say whether a sphere that
  lands off is wrong on average or wrong at random.

* optionally, all of that under a PERTURBED view: ``perturb=`` (a ``perturb.Perturbation``, a preset name or a spec) turns every camera about
  its own optical centre, zooms or shifts it and tints the scene's light, per episode -- ``gn_view_perturb`` warps and re-colours the gathered
  frames once per batch and the camera table changes with them, so the ground-truth render, the windows, the triangulation, the orientation
  read-out and the seed tables all describe the perturbed view.  ``robustness_sweep`` runs the clean evaluator and each setting in turn and
  reports every score's change, beside the seed-to-seed noise floor where there is one.  The rotation and the intrinsics are exact (no
  parallax); the light is a per-channel gain, a stand-in; a camera TRANSLATION and the other four Colosseum factors are left out; and the
  border a turned camera reveals is mirrored scene, not what it would have seen there (``OpenLoopResult.revealed`` counts it).

``OpenLoopEval(agent, None, ...)`` is the diffusion-only mode (no controller exists while the ControlNet is being fine-tuned):
``diffusion_validator`` makes a ``train_loop.TrainLoop`` ``validate`` callable of it.

Frames, scores and the per-transition tables stay on the device; ``run()`` ends with one device-to-host copy of the tables.

What this is NOT: a success rate.  Every chunk is predicted from a demo state, so errors never compound and nothing is executed.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import harness
from .replay import DEFAULT_CAMERAS, DeviceReplay

IMAGE_COLUMNS = ("se_in", "n_in", "se_out", "n_out", "wrap_sq")  # gn_openloop_image_metrics' five values per (transition, camera)
SPHERE_COLUMNS = ("area", "gen_m", "gen_mx", "gen_my", "gen_mr2", "gt_m", "gt_mx", "gt_my", "gt_mr2", "n_occ", "se_occ", "gen_r", "gen_g", "gen_b",
                  "gt_r", "gt_g", "gt_b")  # gn_openloop_sphere_metrics' 17 values per (transition, camera, sphere)


def _mean(x) -> Optional[float]:
    x = np.asarray(x, np.float64)
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else None


def _ratio(a, b, fill=np.nan) -> np.ndarray:
    """``a / b`` where ``b > 0``, ``fill`` elsewhere."""
    return np.divide(a, b, out=np.full(np.shape(a), fill), where=b > 0)


EXEC_COLUMNS = ("joint_l1", "gripper", "jump", "demo_jump")  # gn_openloop_exec_metrics' four values per transition
COMBINE_RULES = ("mean", "medoid")  # gn_openloop_exec_actions_samples' rules: execution row kinds ``seed_mean`` / ``seed_medoid``
POINT_COLUMNS = ("n_views", "x", "y", "z", "err_m", "ray_rms_m", "reproj_rms_px", "det")  # gn_openloop_triangulate's eight values per (transition, group, kind)
POINT_KINDS = ("generated", "ground_truth")
MAX_GROUPS = 8  # gn_openloop_triangulate's bound on G


ORIENTATION_COLUMNS = ("se_gen", "n_gen", "se_gt", "n_gt")  # gn_openloop_orientation's four values per (transition, camera, sphere, candidate)
MAX_CANDIDATES = 64  # gn_openloop_orientation's bound on K
SHIFT_FOUND_MASS = 0.5  # OpenLoopEval(orientation=): a sphere below this mass ratio is compared unshifted (summary()'s default found_mass)


SEED_SPHERE_COLUMNS = ("k", "bias_x", "bias_y", "spread", "shift_sq", "mass_ratio", "mass_ratio_var", "worst_sq")  # gn_openloop_seed_spheres' eight per sphere
SEED_ACTION_COLUMNS = ("seed_mean_l1", "gripper", "spread", "mean_of_seeds_l1")  # gn_openloop_seed_actions' four values per (transition, chunk position)
MAX_SEEDS = 64  # the bound of both on R
# the scalars of diffusion_validator's line, by name: seed_summary() scores each of them per seed
VALIDATOR_SCALARS = ("select", "found_rate", "shift_px", "mass_ratio", "spread_ratio", "colour_l1", "sphere_rmse", "background_rmse", "wrapped_mse")


def _across(values) -> Dict:
    """One score over the seeds -> ``{"values", "mean", "std", "min", "max"}``; ``std`` is the sample standard deviation (ddof = 1).  A None
    (the score does not exist for that seed: nothing drawn, nothing found) is left out of the four statistics."""
    v = np.asarray([x for x in values if x is not None], np.float64)
    return {"values": list(values), "mean": float(v.mean()) if v.size else None, "std": float(v.std(ddof=1)) if v.size > 1 else None,
            "min": float(v.min()) if v.size else None, "max": float(v.max()) if v.size else None}


def orientation_candidates(K: int = 37, span_deg: float = 180.0, axis=(0, 0, 1)):
    """``-> (angles_deg f64 [K], rot f32 [K, 9])``: the candidate rotations of ``gn_openloop_orientation``.  The angles are evenly spaced over
    ``[-span_deg / 2, span_deg / 2]``; K is odd, so 0 is on the grid.  Row k is the Rodrigues rotation by ``angles_deg[k]`` about ``axis``
    (normalised here) in f64, rounded once to f32, row-major; the 0 row is the exact identity.  The default axis is the sphere frame's z: the
    axis a revolute joint turns about in the simulator's joint frames, and the texture's projection axis."""
    K, span = int(K), float(span_deg)
    if not 1 <= K <= MAX_CANDIDATES or K % 2 == 0:
        raise ValueError(f"orientation_candidates: K = {K} must be odd and lie in [1, {MAX_CANDIDATES}]")
    if not 0.0 <= span <= 360.0 or (K > 1 and span == 0.0):
        raise ValueError(f"orientation_candidates: span_deg = {span_deg} must lie in (0, 360]")
    a = np.asarray(axis, np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0.0:
        raise ValueError(f"orientation_candidates: axis = {axis!r} must be a non-zero 3-vector")
    a = a / np.linalg.norm(a)
    mid = (K - 1) // 2
    angles = (np.arange(K, dtype=np.float64) - mid) * (span / (K - 1) if K > 1 else 0.0)
    cross = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    rot = np.empty((K, 3, 3), np.float64)
    for k, t in enumerate(np.deg2rad(angles)):
        rot[k] = np.cos(t) * np.eye(3) + np.sin(t) * cross + (1.0 - np.cos(t)) * np.outer(a, a)
    rot[mid] = np.eye(3)
    return angles, np.ascontiguousarray(rot.reshape(K, 9).astype(np.float32))


def _orientation_option(orientation):
    """``None | K | dict(K=, span_deg=, axis=)`` -> None or ``orientation_candidates``' keyword arguments."""
    if orientation is None:
        return None
    if isinstance(orientation, dict):
        extra = set(orientation) - {"K", "span_deg", "axis"}
        if extra:
            raise ValueError(f"OpenLoopEval: orientation takes K, span_deg and axis, got {sorted(extra)}")
        return dict(orientation)
    if isinstance(orientation, bool) or not isinstance(orientation, (int, np.integer)):
        raise ValueError(f"OpenLoopEval: orientation is None, the number of candidates K or dict(K=, span_deg=, axis=), got {orientation!r}")
    return {"K": int(orientation)}


def parse_orientation(text: str):
    """``K[,span]`` -> ``dict(K=, span_deg=)``: ``"37"`` -> 37 candidates over 180 degrees, ``"25,60"`` -> 25 over 60.  The command lines'
    ``--orientation``."""
    parts = [p.strip() for p in str(text).split(",")]
    try:
        if not 1 <= len(parts) <= 2:
            raise ValueError
        out = {"K": int(parts[0])}
        if len(parts) > 1:
            out["span_deg"] = float(parts[1])
    except ValueError:
        raise ValueError(f"orientation setting {text!r}: K[,span] expected, K an odd integer and span in degrees") from None
    return out


def sphere_groups(spheres, count, windows):
    """The group tables of ``gn_openloop_triangulate``, on the host: ``spheres`` [N, V, S, 16], ``count`` [N, V], ``windows`` int32
    [N, V, S, 4] (the per-transition view tables and ``render.sphere_windows`` of them) -> ``(slot int32 [N, G, V], centre f64 [N, G, 3])``.

    A group is one distinct world centre among the spheres a transition draws (``s < count``): the translation column of the sphere's pose,
    compared by exact f64 equality across the views -- every view packs the same f32 pose, so the same joint compares equal and nothing else
    does.  Groups are listed in order of first appearance (view by view, slot by slot).  ``slot[n, g, v]`` is the slot of view ``v`` that
    shows group ``g``, or -1 where the view does not draw it or where its window is ``(0, 0, 0, 0)``.  ``G`` is the largest group count of
    any transition, at least 1; the rows past a transition's own groups hold -1 and a zero centre."""
    sph, count, win = np.asarray(spheres, np.float64), np.asarray(count), np.asarray(windows)
    N, V, S = sph.shape[:3]
    found = []
    for n in range(N):
        groups = []  # [centre, {view: slot}]
        for v in range(V):
            for s in range(min(int(count[n, v]), S)):
                c = sph[n, v, s, [3, 7, 11]]
                for grp in groups:
                    if (grp[0] == c).all():
                        break
                else:
                    grp = [c, {}]
                    groups.append(grp)
                if v not in grp[1] and win[n, v, s].any():  # a view that packed one centre twice keeps its first slot
                    grp[1][v] = s
        found.append(groups)
    G = max([1] + [len(g) for g in found])
    if G > MAX_GROUPS:
        raise ValueError(f"sphere_groups: a transition draws {G} distinct spheres; gn_openloop_triangulate takes at most {MAX_GROUPS}")
    slot, centre = np.full((N, G, V), -1, np.int32), np.zeros((N, G, 3), np.float64)
    for n, groups in enumerate(found):
        for g, (c, where) in enumerate(groups):
            centre[n, g] = c
            for v, s in where.items():
                slot[n, g, v] = s
    return slot, centre


def parse_execution(text: str):
    """``H[,agg[,M]]`` -> ``(execution_horizon, temporal_agg, m)``: ``"5"`` -> (5, False, 0.01), ``"5,agg"`` / ``"5,on"`` -> (5, True, 0.01),
    ``"5,off,0.1"`` -> (5, False, 0.1).  The command lines' ``--execution`` / ``--val_execution``."""
    parts = [p.strip().lower() for p in str(text).split(",")]
    if not 1 <= len(parts) <= 3 or not parts[0]:
        raise ValueError(f"execution setting {text!r}: H[,agg[,M]] expected")
    try:
        h = int(parts[0])
        m = float(parts[2]) if len(parts) > 2 else 0.01
    except ValueError:
        raise ValueError(f"execution setting {text!r}: H[,agg[,M]] expected, H an integer and M a number") from None
    words = {"agg": True, "on": True, "1": True, "true": True, "off": False, "0": False, "false": False, "": False}
    if len(parts) > 1 and parts[1] not in words:
        raise ValueError(f"execution setting {text!r}: the second field is one of agg / on / off")
    return h, words[parts[1]] if len(parts) > 1 else False, m


class OpenLoopResult:
    """The per-transition tables of one evaluation, on the host.  ``image`` int64 [N, V, 5] (``IMAGE_COLUMNS``; None for a controller-only
    run); ``actions``: ``{"generated" | "oracle": {"norm" | "rad": f32 [N, T, 2]}}`` -- ``[.., 0]`` the joint L1 SUM over the ``joints`` arm
    joints, normalised or in radians, ``[.., 1]`` the gripper flag; ``episode`` / ``step`` / ``task`` int32 [N] (``task`` indexes ``tasks``).
    ``spheres`` int64 [N, V, S, 17] (``SPHERE_COLUMNS``) with ``windows`` int32 [N, V, S, 4], or both None: the per-sphere table and the
    windows it was summed over.  A sphere is DRAWN where the ground truth changed its window (gt mass > 0); the accessors are NaN elsewhere.
    Overlapping windows share pixels, so a neighbour's mass can enter a sphere's sums.

    ``executions``: None, or per replayed execution mode ``{"h", "temporal_agg", "m", "K"}`` plus per row kind (``generated`` / ``oracle``)
    ``{"actions": f32 [N, A], "n_calls": int32 [N], "scores": {"norm" | "rad": f32 [N, 4]}}`` (``EXEC_COLUMNS``: the joint L1 sum and the
    gripper flag of the EXECUTED action against the demo's, the executed jump from the step before and the demo's own).  ``chunks``: the f16
    [N, T, A] table per row kind that the modes were replayed from.  ``summary()`` reads neither; ``execution_summary()`` does.

    ``points``: None, or f64 [N, G, 2, 8] (``POINT_COLUMNS``; kind 0 the generated image, kind 1 the ground-truth render): each drawn sphere
    triangulated from the views that found it -- ``gn_openloop_triangulate`` -- with ``point_slots`` int32 [N, G, V] (the slot of each view
    that shows group g, or -1), ``point_centres`` f64 [N, G, 3] (the true centres) and ``cams`` f32 [N, V, 18] (the camera tables), as
    ``sphere_groups`` and the evaluator made them.  ``summary()`` does not read them; ``triangulation_summary()`` does.

    ``orientation``: None, or int64 [N, V, S, K, 4] (``ORIENTATION_COLUMNS``): per sphere and candidate rotation the squared error of the true
    sphere re-drawn at that rotation against the generated window and against the ground-truth render, each with its pixel count --
    ``gn_openloop_orientation`` -- with ``orientation_angles`` f64 [K], the candidates' angles in degrees (ascending, 0 among them).
    ``summary()`` does not read them; ``orientation_summary()`` does.

    ``seeds``: None, or the list of the R generator seeds a run was repeated with.  With it ``seed_tables``: ``{"image": int64 [R, N, V, 5],
    "spheres": int64 [R, N, V, S, 17]}`` and, with a controller, ``"generated": {"norm" | "rad": f32 [R, N, T, 2]}``, ``"chunks"`` f16
    [R, N, T, A] and ``"demo"`` f32 [N, T, A] (the normalised demo chunks) -- slice 0 of each IS ``image`` / ``spheres`` /
    ``actions["generated"]``; ``seed_spheres`` f64 [N, V, S, 8] (``SEED_SPHERE_COLUMNS``, ``gn_openloop_seed_spheres``) and ``seed_actions``
    ``{"norm" | "rad": f32 [N, T, 4]}`` (``SEED_ACTION_COLUMNS``, ``gn_openloop_seed_actions``; None without a controller).  ``summary()`` and
    the other read-outs describe the first seed and read none of these; ``seed_summary()`` does.

    ``perturbation``: None, or what the run was perturbed with: ``{"setting": Perturbation.describe(), "seed", "draws": per parameter the
    smallest and largest value drawn}``; with it ``revealed`` int32 [N, V], per view the number of pixels whose sample point fell outside
    the source frame (``gn_view_perturb``'s ``n_revealed``).  ``summary()`` reads neither; ``to_json`` adds them under ``"perturbation"``."""

    def __init__(self, image, actions, episode, step, task, tasks: Sequence[str], cameras: Sequence[str], joints: int, H: int, W: int,
                 spheres=None, windows=None, executions=None, chunks=None, points=None, point_slots=None, point_centres=None, cams=None,
                 orientation=None, orientation_angles=None, seeds=None, seed_tables=None, seed_spheres=None, seed_actions=None, perturbation=None,
                 revealed=None):
        if (perturbation is None) != (revealed is None):
            raise ValueError("OpenLoopResult: perturbation and revealed come together")
        self.perturbation, self.revealed = perturbation, revealed
        if seeds is not None and (seed_tables is None or seed_spheres is None or windows is None or len(seeds) != len(seed_tables["spheres"])):
            raise ValueError("OpenLoopResult: seeds come with seed_tables, seed_spheres and windows, one slice per seed")
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.seed_tables, self.seed_spheres, self.seed_actions = (seed_tables, seed_spheres, seed_actions) if seeds is not None else (None, None, None)
        if (spheres is None) != (windows is None):
            raise ValueError("OpenLoopResult: spheres and windows come together (the score needs the windows' diagonals)")
        if points is not None and (windows is None or point_slots is None or point_centres is None or cams is None):
            raise ValueError("OpenLoopResult: points come with windows, point_slots, point_centres and cams (the 3D score's penalty needs them)")
        if orientation is not None and (spheres is None or orientation_angles is None or len(orientation_angles) != orientation.shape[3]):
            raise ValueError("OpenLoopResult: orientation comes with spheres and one angle per candidate (which spheres are drawn and found)")
        self.orientation = orientation
        self.orientation_angles = None if orientation_angles is None else np.asarray(orientation_angles, np.float64)
        self.image, self.actions, self.spheres, self.windows = image, actions, spheres, windows
        self.executions, self.chunks = executions, chunks
        self.points, self.point_slots, self.point_centres, self.cams = points, point_slots, point_centres, cams
        self.episode, self.step, self.task = np.asarray(episode, np.int32), np.asarray(step, np.int32), np.asarray(task, np.int32)
        self.tasks, self.cameras, self.joints, self.H, self.W = list(tasks), list(cameras), int(joints), int(H), int(W)

    def __len__(self):
        return len(self.episode)

    def sphere_rmse(self) -> np.ndarray:
        """f64 [N, V]: ``sqrt(se_in / (3 n_in))``, NaN where ``n_in`` is 0 (no sphere drawn: the last two steps of a trajectory)."""
        return np.sqrt(_ratio(self.image[..., 0].astype(np.float64), 3.0 * self.image[..., 1].astype(np.float64)))

    def background_rmse(self) -> np.ndarray:
        return np.sqrt(_ratio(self.image[..., 2].astype(np.float64), 3.0 * self.image[..., 3].astype(np.float64)))

    def wrapped_mse(self) -> np.ndarray:
        """f64 [N]: the reference's validation ``mse`` (numpy's wrapping uint8 arithmetic) of the whole tiled image."""
        return self.image[..., 4].astype(np.float64).sum(axis=1) / float(len(self.cameras) * self.H * self.W * 3)

    # ---- per sphere, f64 [N, V, S]
    def _col(self, i: int) -> np.ndarray:
        return self.spheres[..., i].astype(np.float64)

    def sphere_drawn(self) -> np.ndarray:
        """bool [N, V, S]: the ground truth changed something in the window (gt mass > 0)."""
        return self.spheres[..., 5] > 0

    def _moments(self, o: int):
        """-> (mass, centroid x, centroid y, radial RMS spread) of the four sums at columns o .. o + 3; NaN where the mass is 0."""
        m = self._col(o)
        cx, cy, r2 = (_ratio(self._col(o + k), m) for k in (1, 2, 3))
        with np.errstate(invalid="ignore"):
            return m, cx, cy, np.sqrt(np.maximum(0.0, r2 - cx * cx - cy * cy))

    def sphere_shift(self) -> np.ndarray:
        """The distance in pixels between the generated and the true centroid; NaN where either mass is 0."""
        (_, gx, gy, _), (_, tx, ty, _) = self._moments(1), self._moments(5)
        return np.hypot(gx - tx, gy - ty)

    def sphere_mass_ratio(self) -> np.ndarray:
        return _ratio(self._col(1), self._col(5))

    def sphere_spread_ratio(self) -> np.ndarray:
        """Generated over true radial RMS spread; NaN where either mass is 0 or the true spread is 0 (a one-pixel target)."""
        return _ratio(self._moments(1)[3], self._moments(5)[3])

    def sphere_colour_l1(self) -> np.ndarray:
        """Mean over the channels of |sum gen_c - sum gt_c| / n_occ over the window's occupied pixels; NaN where undrawn or n_occ is 0."""
        n = self._col(9)
        d = np.abs(self.spheres[..., 11:14] - self.spheres[..., 14:17]).astype(np.float64).mean(axis=-1)
        return np.where(self.sphere_drawn(), _ratio(d, n), np.nan)

    def _per_camera(self, drawn: np.ndarray, block) -> Dict:
        """``block(sel) -> dict`` over ``drawn`` (bool [n, V, S]) restricted to each camera in turn -> ``{key: {camera: value}}`` for every key
        of the block, and the block over all of ``drawn`` under ``overall``."""
        per = {c: block(drawn & (np.arange(len(self.cameras)) == v)[None, :, None]) for v, c in enumerate(self.cameras)}
        overall = block(drawn)
        return dict({k: {c: per[c][k] for c in self.cameras} for k in overall}, overall=overall)

    def _over_tasks(self, block, **extra) -> Dict:
        """``block(rows) -> dict`` over all transitions, then ``extra``, then the block per task under ``per_task`` when there is more than one."""
        out = dict(block(np.ones(len(self), bool)), **extra)
        if len(self.tasks) > 1:
            out["per_task"] = {t: block(self.task == i) for i, t in enumerate(self.tasks)}
        return out

    def _sphere_summary(self, rows: np.ndarray, found_mass: float) -> Dict:
        drawn = self.sphere_drawn()[rows]
        shift, mass = self.sphere_shift()[rows], self.sphere_mass_ratio()[rows]
        spread, colour = self.sphere_spread_ratio()[rows], self.sphere_colour_l1()[rows]
        w = self.windows[rows].astype(np.float64)
        penalty = 0.5 * np.hypot(w[..., 2] - w[..., 0], w[..., 3] - w[..., 1])  # half the window's diagonal: a sphere that is not there
        scored = np.where(np.isnan(shift), penalty, shift)

        def block(sel):  # sel: bool over [n, V', S], the drawn spheres of one camera or of all
            n = int(sel.sum())
            return {"n_drawn": n, "found_rate": float((mass[sel] >= found_mass).mean()) if n else None, "shift_px": _mean(shift[sel]),
                    "mass_ratio": _mean(mass[sel]), "spread_ratio": _mean(spread[sel]), "colour_l1": _mean(colour[sel])}

        out = self._per_camera(drawn, block)
        out["score"] = float(scored[drawn].mean()) if drawn.any() else None
        return out

    def _summary(self, rows: np.ndarray, found_mass: float = 0.5) -> Dict:
        out: Dict = {"n": int(rows.sum())}
        for name, tabs in self.actions.items():
            norm, rad = tabs["norm"][rows].astype(np.float64), tabs["rad"][rows].astype(np.float64)
            out[name] = {"joint_l1_norm": _mean(norm[..., 0] / self.joints), "joint_l1_rad": _mean(rad[..., 0] / self.joints),
                         "gripper_acc": _mean(norm[..., 1]),
                         "per_t": {"joint_l1_norm": (norm[..., 0] / self.joints).mean(axis=0).tolist() if len(norm) else [],
                                   "joint_l1_rad": (rad[..., 0] / self.joints).mean(axis=0).tolist() if len(rad) else [],
                                   "gripper_acc": norm[..., 1].mean(axis=0).tolist() if len(norm) else []}}
        if self.image is not None:
            sph, bg = self.sphere_rmse()[rows], self.background_rmse()[rows]
            out["image"] = {"sphere_rmse": {c: _mean(sph[:, v]) for v, c in enumerate(self.cameras)},  # None: no transition drew a sphere there
                            "sphere_missing": {c: int(np.isnan(sph[:, v]).sum()) for v, c in enumerate(self.cameras)},
                            "background_rmse": {c: _mean(bg[:, v]) for v, c in enumerate(self.cameras)},
                            "wrapped_mse": _mean(self.wrapped_mse()[rows])}
            if self.spheres is not None:
                out["image"]["spheres"] = self._sphere_summary(rows, found_mass)
        return out

    def summary(self, found_mass: float = 0.5) -> Dict:
        """Means over all transitions, in numpy f64: per row (``generated``, ``oracle``) the joint L1 per joint -- normalised and in radians --
        and the gripper accuracy, overall and per chunk position; per camera the sphere-region RMSE over the transitions that drew a sphere
        there (None where none did; ``sphere_missing`` counts the others), the background RMSE and the wrapped ``mse``; ``per_task`` the same
        for each task when there is more than one.  With a sphere table, ``["image"]["spheres"]``: per camera (and under ``overall``) ``n_drawn``,
        ``found_rate`` (the share of drawn spheres whose mass ratio is at least ``found_mass``) and the means of the shift in pixels, the mass
        ratio, the spread ratio and the colour L1; ``score``, lower is better: the mean over the drawn spheres of the shift, a sphere without
        generated mass counting as half the diagonal of its window.  Like every score here it is not a success rate."""
        return self._over_tasks(lambda rows: self._summary(rows, found_mass), cameras=self.cameras, tasks=self.tasks)

    def _execution_block(self, tabs: Dict, h: int, rows: np.ndarray) -> Dict:
        J = float(self.joints)
        norm, rad = tabs["scores"]["norm"][rows].astype(np.float64), tabs["scores"]["rad"][rows].astype(np.float64)
        step = self.step[rows].astype(np.int64)
        pos = step % h
        boundary, inside = (pos == 0) & (step > 0), pos > 0
        out = {"joint_l1_norm": _mean(norm[:, 0] / J), "joint_l1_rad": _mean(rad[:, 0] / J), "gripper_acc": _mean(norm[:, 1]),
               "mean_calls": _mean(tabs["n_calls"][rows]),
               "by_position": {"n": [int((pos == p).sum()) for p in range(h)],
                               "joint_l1_norm": [_mean(norm[pos == p, 0] / J) for p in range(h)],
                               "joint_l1_rad": [_mean(rad[pos == p, 0] / J) for p in range(h)],
                               "gripper_acc": [_mean(norm[pos == p, 1]) for p in range(h)]}}
        for unit, t in (("norm", norm), ("rad", rad)):
            for where, sel in (("boundary", boundary), ("inside", inside)):
                out[f"jump_{where}_{unit}"] = _mean(t[sel, 2] / J)
                out[f"demo_jump_{where}_{unit}"] = _mean(t[sel, 3] / J)
        p = tabs["picks"][rows].astype(np.int64) if "picks" in tabs else np.zeros(0, dtype=np.int64)
        if p.size and int(p.min()) >= 0:  # the medoid's: which seed's chunk was executed (the mean's picks are -1)
            out["pick_histogram"] = np.bincount(p, minlength=len(self.seeds)).tolist()
            out["pick_is_seed0_rate"] = _mean(p == 0)
        return out

    def execution_summary(self) -> Optional[list]:
        """None without ``executions``; else one dict per replayed mode, in numpy f64: ``h``, ``temporal_agg``, ``m``, ``K``, ``calls_per_step``
        (= 1 / h: what the mode costs), and per row kind the per-joint L1 of the EXECUTED action (``joint_l1_norm`` / ``joint_l1_rad``), its
        ``gripper_acc``, ``mean_calls`` (the calls averaged per step), ``by_position``: the three scores and the row count ``n`` by the
        position ``s % h`` inside the call (how the error grows with the age of the prediction; None where no step has that position),
        ``jump_boundary_*`` / ``jump_inside_*``: the mean per-joint jump between consecutive executed actions where a new call takes over
        (``s % h == 0, s > 0``) and inside a call, beside ``demo_jump_*``, the demo's own over the same steps.  ``per_task``: the same per task
        when there is more than one.  Open-loop like every score here: each chunk was predicted from a demo state.

        With ``OpenLoopEval(combine=...)`` the row kinds ``seed_mean`` / ``seed_medoid`` stand beside ``generated`` (which is seed 0 alone): the
        same scores of what the mode executes when the R seeds' chunks of every call are combined first (``GenimaACT.set_execution(samples=R,
        combine=...)``).  ``seed_medoid`` also holds ``pick_histogram`` (how often each seed's chunk was the medoid, over the transitions)
        and ``pick_is_seed0_rate``.  Still teacher-forced, still no success rate; a mean over seeds whose targets lie in different modes is an
        action of neither mode -- the case the medoid exists for."""
        if self.executions is None:
            return None
        out = []
        kinds = ("generated", "oracle") + tuple("seed_" + r for r in COMBINE_RULES)
        for ex in self.executions:
            h = int(ex["h"])
            d = {"h": h, "temporal_agg": bool(ex["temporal_agg"]), "m": float(ex["m"]), "K": int(ex["K"]), "calls_per_step": 1.0 / h}
            d.update(self._over_tasks(lambda rows: {k: self._execution_block(ex[k], h, rows) for k in kinds if k in ex}))
            out.append(d)
        return out

    def point_penalty(self) -> np.ndarray:
        """f64 [N, G], metres: what an unsolved generated group counts as in ``score_mm`` -- half its mean window diagonal at the sphere's
        depth.  Per view ``v`` with ``s = point_slots[n, g, v] >= 0``: the window ``windows[n, v, s]`` has the diagonal ``hypot(x1 - x0,
        y1 - y0)`` pixels; with ``R | t`` the pose in ``cams[n, v, 4:16]`` and ``c = point_centres[n, g]`` the sphere lies ``z = -(R^T (c -
        t)).z`` metres ahead, where one pixel spans ``z / |fx|`` metres (``fx = cams[n, v, 0]``); the view's term is ``0.5 diagonal z /
        |fx|`` and the penalty is the mean of the terms.  NaN where no view shows the group."""
        slots = self.point_slots
        N, G, V = slots.shape
        w = np.take_along_axis(self.windows.astype(np.float64), np.maximum(slots, 0).transpose(0, 2, 1)[..., None], axis=2)  # [N, V, G, 4]
        diag = np.hypot(w[..., 2] - w[..., 0], w[..., 3] - w[..., 1]).transpose(0, 2, 1)  # [N, G, V]
        cams = self.cams.astype(np.float64)
        pose = cams[..., 4:16].reshape(N, V, 3, 4)
        d = self.point_centres[:, :, None, :] - pose[:, None, :, :, 3]  # c - t, [N, G, V, 3]
        z = -np.einsum("nvj,ngvj->ngv", pose[..., 2], d)  # -(R^T (c - t)).z: R's third column
        term = np.where(slots >= 0, 0.5 * diag * z / np.abs(cams[:, None, :, 0]), np.nan)
        return _ratio(np.nansum(term, axis=-1), (slots >= 0).sum(axis=-1))

    def _triangulation_block(self, rows: np.ndarray) -> Dict:
        P = self.points[rows]
        multi = P[:, :, 1, 0] >= 2  # the ground truth drew the group into at least two views
        n = int(multi.sum())
        out: Dict = {"n_groups": n}
        solved = {}
        for k, kind in enumerate(POINT_KINDS):
            ok = solved[kind] = multi & ~np.isnan(P[:, :, k, 4])
            err = P[:, :, k, 4][ok] * 1e3
            out[kind] = {"solved_rate": float(ok.sum() / n) if n else None, "err_mm": _mean(err), "err_median_mm": float(np.median(err)) if err.size else None,
                         "ray_mm": _mean(P[:, :, k, 5][ok] * 1e3), "reproj_px": _mean(P[:, :, k, 6][ok]), "views": _mean(P[:, :, k, 0][multi])}
        both = solved["generated"] & solved["ground_truth"]
        out["excess_mm"] = _mean((P[:, :, 0, 4] - P[:, :, 1, 4])[both] * 1e3)
        scored = np.where(solved["generated"], P[:, :, 0, 4], self.point_penalty()[rows])
        out["score_mm"] = float(scored[multi].mean() * 1e3) if n else None
        return out

    def triangulation_summary(self) -> Optional[Dict]:
        """None without ``points``; else, in numpy f64: ``n_groups``, the number of spheres the ground truth drew into at least two views
        (kind 1's view count >= 2: the spheres a triangulation can be asked of), and per kind (``generated``, ``ground_truth``) over those
        groups ``solved_rate``, the mean and median 3D error ``err_mm`` / ``err_median_mm``, the mean RMS ray residual ``ray_mm`` and
        reprojection residual ``reproj_px`` of the solved ones, and ``views``, the mean number of views used.  ``excess_mm``: the mean over
        the groups solved in both kinds of the generated error minus the ground-truth error.  The centroid of "change against the
        observation" is not the projection of the sphere's centre -- texture, perspective and overlapping windows bias it -- so the
        ``ground_truth`` row is that bias, the floor of the method, and the excess is the model's own part.  ``score_mm``, lower is better:
        the mean over the groups of the generated error, an unsolved group counting as ``point_penalty()``.  ``per_task``: the same per
        task when there is more than one.  Teacher-forced like every score here, and not a success rate."""
        if self.points is None:
            return None
        return self._over_tasks(self._triangulation_block)

    def orientation_scores(self, found_mass: float = 0.5, min_pixels: int = 50) -> Dict[str, np.ndarray]:
        """Per sphere, [N, V, S], in numpy f64.  ``readable`` (bool): the ground-truth cost curve ``se_gt / n_gt`` over the candidates is not
        flat (max > min); a flat curve means the sphere's own texture is not visible in its window (it is hidden behind a neighbour), so no
        rotation of it changes a pixel.  ``scored`` (bool): drawn, found (mass ratio >= ``found_mass``), readable and at least ``min_pixels``
        pixels in ``n_gen``.  Over the generated curve ``se_gen / n_gen`` of a scored sphere, NaN elsewhere: ``err_deg`` = |the angle at the
        first argmin|, ``contrast`` = 1 - min / mean (0: the orientation is not in the image), ``at_edge`` (1.0 where the argmin is the first
        or the last candidate).  ``floor_deg``: ``err_deg`` of the ground-truth curve for every drawn, readable sphere, NaN elsewhere -- 0 by
        construction, since the identity candidate reproduces the ground truth."""
        O = self.orientation.astype(np.float64)
        ang, K = self.orientation_angles, self.orientation.shape[3]
        cg, ct = _ratio(O[..., 0], O[..., 1]), _ratio(O[..., 2], O[..., 3])
        drawn = self.sphere_drawn()
        readable = (O[..., 3] > 0).all(axis=-1) & (self.orientation[..., 2].max(axis=-1) > self.orientation[..., 2].min(axis=-1))
        with np.errstate(invalid="ignore"):
            found = self.sphere_mass_ratio() >= found_mass
        scored = drawn & found & readable & (self.orientation[..., 0, 1] >= max(1, int(min_pixels)))
        cg, ct = np.where(scored[..., None], cg, 0.0), np.where((drawn & readable)[..., None], ct, 0.0)  # no NaN reaches an argmin
        ig, it = np.argmin(cg, axis=-1), np.argmin(ct, axis=-1)
        cmin, cmean = cg.min(axis=-1), cg.mean(axis=-1)
        contrast = 1.0 - _ratio(cmin, cmean, fill=1.0)
        return {"readable": readable, "scored": scored, "found": found, "err_deg": np.where(scored, np.abs(ang[ig]), np.nan),
                "contrast": np.where(scored, contrast, np.nan), "at_edge": np.where(scored, ((ig == 0) | (ig == K - 1)).astype(np.float64), np.nan),
                "floor_deg": np.where(drawn & readable, np.abs(ang[it]), np.nan)}

    def _orientation_block(self, sc: Dict[str, np.ndarray], rows: np.ndarray) -> Dict:
        ang = self.orientation_angles
        step = float(ang[1] - ang[0]) if len(ang) > 1 else 0.0
        half = 0.5 * float(ang[-1] - ang[0])
        drawn = self.sphere_drawn() & rows[:, None, None]

        def block(sel):  # sel: bool over [N, V, S], the drawn spheres of one camera or of all
            s = sel & sc["scored"]
            err = sc["err_deg"][s]
            floor = sc["floor_deg"][sel & sc["readable"]]
            return {"n_scored": int(s.sum()), "n_unreadable": int((sel & ~sc["readable"]).sum()), "err_deg": _mean(err),
                    "err_median_deg": float(np.median(err)) if err.size else None,
                    "within_step": float((err <= step * (1.0 + 1e-12)).mean()) if err.size else None, "contrast": _mean(sc["contrast"][s]),
                    "at_edge": _mean(sc["at_edge"][s]), "floor_deg": float(floor.max()) if floor.size else None}

        out = self._per_camera(drawn, block)
        counted = drawn & sc["readable"] & (sc["scored"] | ~sc["found"])
        out["score_deg"] = float(np.where(sc["scored"], sc["err_deg"], half)[counted].mean()) if counted.any() else None
        return out

    def orientation_summary(self, found_mass: float = 0.5, min_pixels: int = 50) -> Optional[Dict]:
        """None without ``orientation``; else, in numpy f64 over ``orientation_scores(found_mass, min_pixels)``: per camera and under
        ``overall`` ``n_scored``, ``n_unreadable`` (drawn spheres with a flat ground-truth curve), the mean and median ``err_deg`` /
        ``err_median_deg``, ``within_step`` (the share of scored spheres within one grid step of 0), the mean ``contrast``, the ``at_edge``
        share (the best candidate is an end of the searched range: the true minimum may lie outside it) and ``floor_deg``, the largest error
        of the ground-truth curve over the drawn readable spheres: it is 0, or the read-out is broken.  ``score_deg``, lower is better: the
        mean of ``err_deg`` over the drawn, readable spheres, a sphere that was not found counting as half the searched span (a found
        sphere with fewer than ``min_pixels`` pixels is left out).  ``angles_deg``: the candidates.  ``per_task``: the same per task when
        there is more than one.  It says whether the IMAGE carries the orientation; it does not measure whether the controller reads the
        stripes, a stripe pattern that repeats under a half turn cannot be told from its twin, and like every score here it is teacher-forced
        and not a success rate."""
        if self.orientation is None:
            return None
        sc = self.orientation_scores(found_mass, min_pixels)
        return self._over_tasks(lambda rows: self._orientation_block(sc, rows), angles_deg=self.orientation_angles.tolist())

    def validator_scalars(self, found_mass: float = 0.5) -> Dict:
        """The scalars of ``diffusion_validator``'s line (``VALIDATOR_SCALARS``) from ``summary(found_mass)``: ``select`` is the sphere
        ``score``, the five sphere fields its ``overall`` block, the two RMSEs the means over all cameras."""
        im = self.summary(found_mass)["image"]
        sp = im["spheres"]
        return {"select": sp["score"], "found_rate": sp["overall"]["found_rate"], "shift_px": sp["overall"]["shift_px"],
                "mass_ratio": sp["overall"]["mass_ratio"], "spread_ratio": sp["overall"]["spread_ratio"], "colour_l1": sp["overall"]["colour_l1"],
                "sphere_rmse": _mean(self.sphere_rmse()), "background_rmse": _mean(self.background_rmse()), "wrapped_mse": im["wrapped_mse"]}

    def seed_result(self, r: int) -> "OpenLoopResult":
        """The tables of seed ``r`` alone as a result of their own: what a run without ``seeds`` and with ``seed = seeds[r]`` returns in
        ``image``, ``spheres`` and ``actions["generated"]`` (no oracle row, none of the optional tables)."""
        st = self.seed_tables
        acts = {"generated": {u: t[r] for u, t in st["generated"].items()}} if "generated" in st else {}
        return OpenLoopResult(st["image"][r], acts, self.episode, self.step, self.task, self.tasks, self.cameras, self.joints, self.H, self.W,
                              spheres=st["spheres"][r], windows=self.windows)

    def _seed_sphere_block(self, sel: np.ndarray) -> Dict:
        """``sel``: bool [N, V, S] -> the spread block over the selected spheres that at least two seeds found."""
        t = self.seed_spheres
        sel = sel & (t[..., 0] >= 2)
        n = int(sel.sum())
        if not n:
            return {"n": 0, "found_all_rate": None, "bias_px": None, "spread_px": None, "rms_shift_px": None, "variance_share": None,
                    "mass_ratio_std": None, "worst_px": None}
        q = t[sel]
        shift = float(q[:, 4].sum())
        return {"n": n, "found_all_rate": float((q[:, 0] == len(self.seeds)).mean()), "bias_px": float(np.hypot(q[:, 1], q[:, 2]).mean()),
                "spread_px": float(np.sqrt(q[:, 3].mean())), "rms_shift_px": float(np.sqrt(q[:, 4].mean())),
                "variance_share": float(q[:, 3].sum() / shift) if shift > 0 else None, "mass_ratio_std": float(np.sqrt(q[:, 6].mean())),
                "worst_px": float(np.sqrt(q[:, 7].max()))}

    def seed_summary(self, found_mass: float = 0.5) -> Optional[Dict]:
        """None without ``seeds``; else, in numpy f64:

        ``seeds``: the seed values.  ``scores``: per scalar of the validator's line (``VALIDATOR_SCALARS``; ``select`` is the sphere
        ``score``) and, with a controller, ``joint_l1_norm`` / ``joint_l1_rad`` / ``gripper_acc`` of ``generated``: ``{"values": [R], "mean",
        "std", "min", "max"}`` -- ``values[r]`` is ``summary(found_mass)``'s own code on seed r's tables, so ``values[0]`` is the number
        ``summary()`` reports, and ``std`` (ddof = 1) is the noise floor a difference between two checkpoints has to beat.

        ``spheres``: ``overall`` and ``per_camera`` over the spheres at least two seeds found (``seed_spheres[..., 0] >= 2``, the evaluator's
        ``seed_min_ratio`` deciding "found"): ``n``, ``found_all_rate`` (the share every seed found), ``bias_px`` (the mean distance of the
        seeds' mean centroid from the true one), ``spread_px`` (the RMS distance of a seed's centroid from the seeds' mean), ``rms_shift_px``
        (the RMS distance from the true centroid; ``rms_shift_px^2 = RMS(bias)^2 + spread_px^2``), ``variance_share`` = sum spread / sum
        squared shift: 0 means every seed is wrong in the same way (bias: train more), 1 means the seeds scatter about the truth (noise: the
        seed matters), ``mass_ratio_std`` (the RMS over the spheres of the seeds' standard deviation of the mass ratio) and ``worst_px``, the
        largest shift of any seed.

        ``actions`` (with a controller), per unit ``norm`` / ``rad``, per joint: ``mean_of_seeds`` (the seeds' own joint L1, averaged),
        ``seed_mean`` (the joint L1 of the chunk averaged over the seeds), ``gain`` = 1 - seed_mean / mean_of_seeds: what executing the mean
        of R sampled chunks would buy, ``spread`` (the mean absolute deviation of a joint across the seeds) and ``gripper_acc_seed_mean``.

        Teacher-forced like every score here: a seed spread is not a success rate, and ``gain`` is what averaging buys open loop, on demo
        states -- nothing is executed."""
        if self.seeds is None:
            return None
        per = [self.seed_result(r) for r in range(len(self.seeds))]
        scalars = [p.validator_scalars(found_mass) for p in per]
        scores = {k: _across([s[k] for s in scalars]) for k in VALIDATOR_SCALARS}
        if "generated" in self.seed_tables:
            rows = np.ones(len(self), bool)
            gen = [p._summary(rows, found_mass)["generated"] for p in per]
            scores.update({k: _across([g[k] for g in gen]) for k in ("joint_l1_norm", "joint_l1_rad", "gripper_acc")})
        out: Dict = {"seeds": list(self.seeds), "scores": scores}
        everything = np.ones(self.seed_spheres.shape[:3], bool)
        out["spheres"] = {"overall": self._seed_sphere_block(everything),
                          "per_camera": {c: self._seed_sphere_block(everything & (np.arange(len(self.cameras)) == v)[None, :, None])
                                         for v, c in enumerate(self.cameras)}}
        if self.seed_actions is not None:
            J, out["actions"] = float(self.joints), {}
            for unit, t in self.seed_actions.items():
                t = t.astype(np.float64)
                each, mean = _mean(t[..., 3] / J), _mean(t[..., 0] / J)
                out["actions"][unit] = {"mean_of_seeds": each, "seed_mean": mean, "gain": 1.0 - mean / each if each else None,
                                        "spread": _mean(t[..., 2] / J), "gripper_acc_seed_mean": _mean(t[..., 1])}
        return out

    def revealed_share(self) -> Optional[float]:
        """None without a perturbation; else the mean over every view of the share of its pixels that the perturbation revealed."""
        return None if self.revealed is None else float(self.revealed.astype(np.float64).mean() / float(self.H * self.W))

    def perturbation_summary(self) -> Optional[Dict]:
        """None without a perturbation; else ``perturbation`` (the setting's ``describe()``, the seed, the draws' ranges) plus
        ``revealed_share`` overall and per camera.  An open-loop score under a perturbation is still not a success rate."""
        if self.perturbation is None:
            return None
        per = self.revealed.astype(np.float64).mean(axis=0) / float(self.H * self.W)
        return dict(self.perturbation, revealed_share=self.revealed_share(), revealed_share_per_camera={c: float(per[v]) for v, c in enumerate(self.cameras)})

    def to_json(self, path: str) -> Dict:
        s = self.summary()
        for key, extra in (("executions", self.execution_summary()), ("spheres_3d", self.triangulation_summary()), ("orientation", self.orientation_summary()),
                           ("seeds", self.seed_summary()), ("perturbation", self.perturbation_summary())):
            if extra is not None:  # a key of its own, and only with its table: summary() itself is as it was
                s[key] = extra
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(s, f, indent=1)
        return s


def _task_of(ep, description: str) -> str:
    """``<root>/<task>/variation<k>/episodes/<episode>`` -> ``<task>``; anything else is named by its description."""
    if isinstance(ep, (str, os.PathLike)):
        parts = os.path.normpath(os.fspath(ep)).split(os.sep)
        if len(parts) >= 4 and parts[-2] == "episodes" and parts[-3].startswith("variation"):
            return parts[-4]
    return description


_NUMPY_OF = {torch.int64: np.int64, torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32, torch.float16: np.float16}


def readback_layout(tables: Dict[str, Optional[torch.Tensor]]) -> Dict[str, int]:
    """name -> byte offset of each table in ``read_back``'s packed buffer, in packing order.  None entries are dropped and the rest are
    stable-sorted by element size, widest first: the sizes are powers of two, so every table starts on a multiple of its own."""
    offsets, o = {}, 0
    for name in sorted((k for k, t in tables.items() if t is not None), key=lambda k: -tables[k].element_size()):
        offsets[name] = o
        o += tables[name].numel() * tables[name].element_size()
    return offsets


def read_back(tables: Dict[str, Optional[torch.Tensor]]) -> Dict[str, np.ndarray]:
    """Named contiguous tensors of one device (None entries are dropped) -> a host copy of each under its name, with its dtype and shape, in
    the order given.  One ``torch.cat`` of the tables' bytes, laid out as ``readback_layout`` says, and one copy to the host."""
    offsets = readback_layout(tables)
    if not offsets:
        return {}
    host = torch.cat([tables[k].reshape(-1).view(torch.uint8) for k in offsets]).cpu().numpy()
    return {k: host[offsets[k]: offsets[k] + t.numel() * t.element_size()].view(_NUMPY_OF[t.dtype]).reshape(tuple(t.shape)).copy()
            for k, t in tables.items() if t is not None}


def _map_tensors(tree, fn, name: str = ""):
    """``tree``: nested dicts and lists -> the same tree with every tensor ``t`` in it replaced by ``fn(name, t)``, ``name`` the keys and list
    positions that lead to it joined by ``/`` (``executions/0/oracle/scores/norm``); every other leaf stays as it is."""
    if isinstance(tree, torch.Tensor):
        return fn(name, tree)
    if isinstance(tree, dict):
        return {k: _map_tensors(v, fn, f"{name}/{k}".lstrip("/")) for k, v in tree.items()}
    return [_map_tensors(v, fn, f"{name}/{i}") for i, v in enumerate(tree)] if isinstance(tree, list) else tree


class OpenLoopEval:
    """``OpenLoopEval(diffusion_agent, controller, episodes, ...).run() -> OpenLoopResult``.

    ``diffusion_agent``: any agent of ``agent.py`` (its ``pipe`` is called as ``SDControlNetAgent.infer`` calls it, with ``output_type="pt"``),
    or None: the controller alone on the ground-truth targets (``controller_validator``).  ``controller``: a ``GenimaACT`` with no execution
    mode set (whole chunks are compared) and ``frame_stack`` 1.  ``episodes``: directories holding ``demo.npz``, ``traj.npz``, the camera PNGs
    and optionally ``description.txt``, or ``(demo, frames, traj[, description])`` tuples.  ``render_cfg``: the ``render.RenderConfig`` the
    targets are drawn with (the one the diffusion model's training targets were rendered with).  ``stats``: the TRAINING run's ``(action_stats,
    proprio_stats)`` (``replay.load_stats`` of the snapshot directory) -- a held-out set must not be normalised with its own statistics.
    ``tokenizer``: the controller's task-token source, as ``DeviceReplay`` takes it.  ``change_threshold``: ``gn_openloop_sphere_metrics``'
    threshold on the summed absolute channel difference against the observation (a starting value, not measured against a trained checkpoint).

    ``controller=None`` with a diffusion agent is the diffusion-only mode: no controller pass, no action tables (``result.actions == {}``); the
    device and the engine come from the agent's pipeline, ``stats`` may be None (the replay then normalises with the set's own statistics, and
    nothing that depends on them is scored) and ``action_sequence`` (default: the controller's ``num_queries``, else 20) sets the replay's
    chunk length.  Its image and sphere tables equal those of a run with a controller on the same seed bit for bit.

    ``executions``: None, or a sequence of ``(execution_horizon, temporal_agg, m)`` (``m`` may be left out: 0.01), each checked as
    ``GenimaACT.set_execution`` checks them.  The controller passed in still has NO mode set: the modes are replayed from its whole chunks.
    With them ``run()`` also keeps every scored chunk in an f16 device table [N, T, A] per row kind, and after the last batch launches
    ``gn_openloop_exec_actions`` once and ``gn_openloop_exec_metrics`` twice (normalised, radians) per setting and row kind; the new tables
    ride in the same device-to-host copy (``OpenLoopResult.executions`` / ``.chunks``).  With None nothing changes: the same launches, the
    same tables, the same bits.

    ``triangulate``: also place every drawn sphere in the world.  At setup the group tables are built on the host (``sphere_groups``: which slot
    of which view shows which sphere, and its true centre) and uploaded once; after the last batch ``run()`` launches
    ``gn_openloop_triangulate`` once over the finished sphere table and the f64 table [N, G, 2, 8] rides in the same device-to-host copy
    (``OpenLoopResult.points``, ``triangulation_summary()``).  ``tri_min_ratio``: a view counts for the generated image when its mass is at
    least this share of the ground truth's; ``tri_min_det``: rays that cross worse than this are left unsolved.  It needs a diffusion agent;
    with False nothing changes: the same launches, the same tables, the same bits.

    ``orientation``: None, the number of candidates K, or ``dict(K=, span_deg=, axis=)`` (``orientation_candidates``' arguments): also read the
    orientation the generated spheres show.  Per batch, after the sphere metrics, the shift of every sphere is computed on the device from
    that batch's rows of the sphere table -- the difference of the generated and the true centroid (columns 1..3 and 5..7) in f64, rounded to
    the nearest integer pixel; 0 where either mass is 0 or the mass ratio is below ``SHIFT_FOUND_MASS`` -- and ``gn_openloop_orientation``
    fills the batch's rows of an int64 [N, V, S, K, 4] table, which rides in the same device-to-host copy (``OpenLoopResult.orientation``,
    ``orientation_summary()``).  It needs a diffusion agent; with None nothing changes: the same launches, the same tables, the same bits.

    ``seeds``: None, or the number R in [2, 64] of generator seeds to repeat the generation with: how much of a score is the checkpoint and how
    much the noise draw.  ``run()`` then makes R device generators seeded ``seed + r``; per batch the targets are made once and, for r in order,
    the pipeline runs with generator r, then ``act_tiled`` and the image / sphere / action scores, into seed r's rows of tables with a leading
    seed axis (each seed's chunk is copied out of the program's output buffer before the next ``act_tiled`` overwrites it); the oracle pass
    runs once, and the batch's normalised demo chunk is kept.  Seed 0's slices ARE ``image`` / ``spheres`` / ``actions["generated"]`` /
    ``chunks["generated"]``, so ``summary()``, ``triangulate``, ``orientation`` and ``executions`` describe the first seed, exactly as a run
    without ``seeds`` and the same ``seed`` does.  After the last batch ``gn_openloop_seed_spheres`` runs once (``seed_min_ratio``: a seed
    found a sphere when its mass is at least this share of the true one) and, with a controller, ``gn_openloop_seed_actions`` twice
    (normalised, radians); their outputs and the seed tables ride in the same device-to-host copy (``OpenLoopResult.seed_tables`` /
    ``.seed_spheres`` / ``.seed_actions``, ``seed_summary()``).  It needs a diffusion agent and costs R generations per transition; with None
    nothing changes: the same launches, the same tables, the same bits.

    ``combine``: None, ``"mean"``, ``"medoid"`` or a sequence of the two; it needs ``seeds`` and ``executions``.  After the last batch, per
    execution setting and rule, ``gn_openloop_exec_actions_samples`` replays the setting over the COMBINATION of the R seeds' chunks of every
    transition -- their mean in seed order, or their medoid -- bit for bit what ``GenimaACT.set_execution(..., samples=R, combine=)`` executes,
    and ``gn_openloop_exec_metrics`` scores it twice; the tables ride in the same copy (``executions[i]["seed_mean" | "seed_medoid"]``:
    ``actions``, ``n_calls``, ``picks``, ``scores``) and ``execution_summary()`` gets those row kinds beside ``generated``, which stays seed
    0.  Still teacher-forced; a mean across two modes is an action of neither, which is what the medoid is for.  With None nothing changes.

    ``perturb``: None, a ``perturb.Perturbation``, a preset name or a spec (``perturb.parse``), drawn with ``perturb_seed``; the same as
    calling ``set_perturbation(perturb, perturb_seed)`` after the setup.  The clean host view tables are kept.  ``set_perturbation`` draws
    the values per episode (``perturb.draw``), recomputes the camera table (``perturb.perturb_cams``) and from it the windows -- with
    ``triangulate`` also the group tables and the host camera table -- and uploads them with a per-(transition, view) homography f64
    [N, V, 9] and colour row f64 [N, V, 6]; ``set_perturbation(None)`` puts the clean tables back.  ``targets()`` then launches
    ``gn_view_perturb`` once per batch on the gathered ``images_u8``, and the warped frames take their place in the batch: as
    ``images_u8``, as the background of the ground-truth render (the spheres are drawn untinted over the tinted frame, as a renderer would
    overlay them) and as ``tiled``.  The proprioception, the actions and the tokens are untouched.  The per-view revealed counts go into an
    int32 [N, V] table that rides in the one device-to-host copy (``OpenLoopResult.revealed``).  ``seeds``, ``executions``, ``triangulate``
    and ``orientation`` compose with it: they read the batch and the tables.  Both the diffusion-only and the controller-only mode take it;
    the controller-only mode's oracle pass sees the target over the perturbed frame.  With None there is no launch, no table and no bit
    changed.  A score under a perturbation is still open-loop and not a success rate.

    Per batch, on the device: ``DeviceReplay.sample`` (the frames, proprioception, normalised action chunk, task tokens) -> ``gn_render_spheres``
    over the frames (``full``, ``occupied``) -> the four views on the 2x2 canvas -> the pipeline (``harness.make_prompt`` ids, one generator
    seeded ``seed`` and advanced call by call) -> ``act_tiled`` -> the image, sphere and action scores -> the controller again on ``full`` -> its action
    scores.  The transitions are walked in order; the last batch is padded by repeating its last index and scores only its first rows, so one
    recorded program per network serves the whole run."""

    def __init__(self, diffusion_agent, controller, episodes, cameras: Sequence[str] = DEFAULT_CAMERAS, *, render_cfg, stats, tokenizer=None,
                 batch_size: int = 8, num_inference_steps: int = 5, guidance_scale: float = 0.0, seed: int = 0, engine=None,
                 change_threshold: int = 30, action_sequence: Optional[int] = None, executions=None, triangulate: bool = False,
                 tri_min_ratio: float = 0.5, tri_min_det: float = 1e-6, orientation=None, seeds: Optional[int] = None, seed_min_ratio: float = 0.5,
                 perturb=None, perturb_seed: int = 0, combine=None):
        from .render import load_traj

        device, engine, T = self._check_options(diffusion_agent, controller, cameras, stats, engine, change_threshold, action_sequence, executions,
                                                triangulate, tri_min_ratio, tri_min_det, orientation, seeds, seed_min_ratio, combine)
        self.cfg, self.batch_size = render_cfg, int(batch_size)
        self.num_inference_steps, self.guidance_scale, self.seed = int(num_inference_steps), float(guidance_scale), int(seed)
        H, W = int(render_cfg.image_height), int(render_cfg.image_width)
        eps, trajs = [], []
        for ep in episodes:
            if isinstance(ep, (str, os.PathLike)):
                eps.append(os.fspath(ep))
                trajs.append(load_traj(os.path.join(os.fspath(ep), "traj.npz")))
            else:
                eps.append((ep[0], ep[1]) + tuple(ep[3:4]))
                trajs.append(ep[2])
        rp = self.replay = DeviceReplay(eps, self.cameras, engine=engine, device=device, frame_stack=1, action_sequence=T, batch_size=self.batch_size, tokenizer=tokenizer,
                                        image_size=H if H == W and isinstance(eps[0], str) else None, stats=stats)
        if (rp.H, rp.W) != (H, W):
            raise ValueError(f"OpenLoopEval: the frames are {rp.H} x {rp.W}, the render config draws {H} x {W}")
        if controller is not None and rp.A != int(controller.config["action_dim"]):
            raise ValueError(f"OpenLoopEval: the demos' actions have {rp.A} elements, the controller's {controller.config['action_dim']}")
        if self.executions is not None and tuple(rp.action.shape) != (rp.N, rp.A):
            raise ValueError(f"OpenLoopEval: the replay's demo actions are {tuple(rp.action.shape)}, expected {(rp.N, rp.A)}")
        self.E, self.N, self.H, self.W, self.T, self.A = rp.E, rp.N, H, W, rp.T, rp.A
        self._upload(self._transition_tables(trajs, episodes), stats)
        self.perturbation, self.perturb_seed, self.perturb_draws, self.perturb_M, self.perturb_colour = None, 0, None, None, None
        if perturb is not None:
            self.set_perturbation(perturb, perturb_seed)

    def _check_options(self, diffusion_agent, controller, cameras, stats, engine, change_threshold, action_sequence, executions, triangulate,
                       tri_min_ratio, tri_min_det, orientation, seeds=None, seed_min_ratio=0.5, combine=None):
        """Part one of the setup, before any device work: every option checked and kept -> ``(device, engine, T)`` for the replay."""
        if controller is None:
            if diffusion_agent is None:
                raise ValueError("OpenLoopEval: nothing to score -- give a diffusion agent, a controller or both")
            device = diffusion_agent.pipe.device
            if engine is None:
                engine = diffusion_agent.pipe.unet.engine()
            T = 20 if action_sequence is None else int(action_sequence)
        else:
            if controller.execution is not None:
                raise ValueError(f"OpenLoopEval: the controller has an execution mode set ({controller.execution}); open-loop scoring compares whole "
                                 "chunks -- call set_execution() with nothing set first")
            if int(controller.config.get("frame_stack", 1)) > 1:
                raise NotImplementedError("OpenLoopEval: frame-stacked controllers (frame_stack > 1) are not scored")
            if stats is None:
                raise ValueError("OpenLoopEval: stats = (action_stats, proprio_stats) of the TRAINING run is required (replay.load_stats)")
            device, T = controller.device, int(controller.config["num_queries"])
            if action_sequence is not None and int(action_sequence) != T:
                raise ValueError(f"OpenLoopEval: action_sequence = {action_sequence} contradicts the controller's num_queries = {T}")
        if int(change_threshold) < 0:
            raise ValueError(f"OpenLoopEval: change_threshold = {change_threshold} must not be negative")
        self.executions = None
        if executions is not None:  # the execution modes to replay over the chunks, checked as GenimaACT.set_execution checks them
            from .act import check_ensemble_m, execution_slots

            if controller is None:
                raise ValueError("OpenLoopEval: executions replays the controller's chunks; the diffusion-only mode has none")
            self.executions = []
            for ex in executions:
                ex = tuple(ex)
                if not 2 <= len(ex) <= 3:
                    raise ValueError(f"OpenLoopEval: an execution setting is (execution_horizon, temporal_agg[, m]), got {ex!r}")
                h, K = execution_slots(T, ex[0], bool(ex[1]))
                self.executions.append({"h": int(h), "temporal_agg": bool(ex[1]), "m": check_ensemble_m(ex[2] if len(ex) > 2 else 0.01), "K": int(K)})
        self.triangulate, self.tri_min_ratio, self.tri_min_det = bool(triangulate), float(tri_min_ratio), float(tri_min_det)
        if self.triangulate:
            if diffusion_agent is None:
                raise ValueError("OpenLoopEval: triangulate places the generated spheres; without a diffusion agent nothing is generated")
            if not self.tri_min_ratio >= 0.0 or not self.tri_min_det > 0.0:
                raise ValueError(f"OpenLoopEval: tri_min_ratio = {tri_min_ratio} must be >= 0 and tri_min_det = {tri_min_det} > 0")
        self.orientation_angles = self.orientation_rot = None
        orient = _orientation_option(orientation)
        if orient is not None:
            if diffusion_agent is None:
                raise ValueError("OpenLoopEval: orientation reads the generated spheres; without a diffusion agent nothing is generated")
            self.orientation_angles, self.orientation_rot = orientation_candidates(**orient)  # on the host until _upload
        self.seeds, self.seed_min_ratio = None, float(seed_min_ratio)
        if seeds is not None:
            if isinstance(seeds, bool) or not isinstance(seeds, (int, np.integer)) or not 2 <= int(seeds) <= MAX_SEEDS:
                raise ValueError(f"OpenLoopEval: seeds is None or the number of generator seeds R, an integer in [2, {MAX_SEEDS}], got {seeds!r}")
            if diffusion_agent is None:
                raise ValueError("OpenLoopEval: seeds repeats the generation with other noise; without a diffusion agent nothing is generated")
            if not self.seed_min_ratio >= 0.0:
                raise ValueError(f"OpenLoopEval: seed_min_ratio = {seed_min_ratio} must be >= 0")
            self.seeds = int(seeds)
        self.combine = None
        if combine is not None:  # the rules that turn the R seeds' chunks into the executed one, scored per execution setting
            rules = (combine,) if isinstance(combine, str) else tuple(combine)
            if not rules or len(set(rules)) != len(rules) or any(r not in COMBINE_RULES for r in rules):
                raise ValueError(f"OpenLoopEval: combine is None or distinct rules out of {COMBINE_RULES}, got {combine!r}")
            if self.seeds is None or self.executions is None:
                raise ValueError("OpenLoopEval: combine scores the combination of the seeds' chunks under an execution mode: it needs seeds=R and executions=[...]")
            self.combine = rules
        self.agent, self.controller, self.cameras, self.V, self.change_threshold = diffusion_agent, controller, tuple(cameras), len(cameras), int(change_threshold)
        if diffusion_agent is not None and self.V != 4:
            raise ValueError(f"OpenLoopEval: the 2x2 canvas takes exactly four cameras, got {self.V}")
        return device, engine, T

    def _transition_tables(self, trajs, episodes) -> Dict[str, np.ndarray]:
        """Part two, on the host: transition n of episode e, step t, reads observation t of trajectory e -> the view tables [N, V, ...] to
        upload; the step, episode and task of every transition, the spheres' windows, the groups and the episodes' first transitions are kept."""
        from .replay import view_tables

        rp = self.replay
        vt = view_tables(trajs, self.cfg, self.cameras)  # row obs * V + v over EVERY step of every trajectory
        starts = np.concatenate([[0], np.cumsum([len(t["gripper_open"]) for t in trajs])])
        ep_of = rp.host["episode"]
        counts = np.bincount(ep_of, minlength=rp.N_ep)  # transitions per episode
        step = (np.arange(rp.N) - np.concatenate([[0], np.cumsum(counts)[:-1]])[ep_of]).astype(np.int32)
        for e, t in enumerate(trajs):
            if len(t["gripper_open"]) != int(counts[e]) + 1:
                raise ValueError(f"OpenLoopEval: episode {e} has {int(counts[e]) + 1} observations in its demo and {len(t['gripper_open'])} steps in its trajectory")
        rows = ((starts[ep_of] + step)[:, None] * self.V + np.arange(self.V)[None]).reshape(-1)
        views = {k: np.ascontiguousarray(vt[k][rows].reshape((rp.N, self.V) + vt[k].shape[1:])) for k in vt}
        self.views_host = views  # the CLEAN tables: set_perturbation derives the perturbed ones from them and puts them back
        self._camera_tables(views["cams"])
        # with execution modes to replay: the first transition of each one's episode
        self.first_tr_host = np.ascontiguousarray((np.arange(rp.N) - step).astype(np.int32)) if self.executions is not None else None
        self.step_index, self.episode_index = step, ep_of.copy()
        names = [_task_of(ep, d) for ep, d in zip(episodes, rp.descriptions)]
        self.tasks = sorted(set(names))
        self.task_index = np.asarray([self.tasks.index(names[e]) for e in ep_of], np.int32)
        return views

    def _camera_tables(self, cams: np.ndarray) -> None:
        """The host tables that follow from a camera table f32 [N, V, 18] (the clean one, or a perturbed one): with a diffusion agent the
        spheres' windows of every transition, int32 [N, V, S, 4], and with ``triangulate`` which slot of which view shows which sphere and
        where it truly is, int32 [N, G, V] and f64 [N, G, 3], beside the camera table itself."""
        from .render import sphere_windows

        views = self.views_host
        self.windows_host = self.point_slots_host = self.point_centres_host = self.cams_host = None
        if self.agent is not None:
            self.windows_host = np.ascontiguousarray(sphere_windows(cams, views["spheres"], views["count"], self.H, self.W))
            if self.triangulate:
                self.point_slots_host, self.point_centres_host = sphere_groups(views["spheres"], views["count"], self.windows_host)
                self.cams_host = cams

    def set_perturbation(self, p=None, seed: int = 0) -> None:
        """``p``: None, a ``perturb.Perturbation``, a preset name or a spec.  Draws the values of every episode with ``seed``, recomputes the
        camera table and what follows from it on the host and uploads them with the homographies and the colour rows; None puts the clean
        tables back.  The next ``run()`` / ``targets()`` uses them; nothing is launched here."""
        from . import perturb as PB

        def up(a):
            return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.E.device)

        clean = self.views_host["cams"]
        if p is None:
            cams, M, colour = clean, None, None
            self.perturbation, self.perturb_seed, self.perturb_draws = None, 0, None
        else:
            p = PB.parse(p)
            cams, M, colour, draws = PB.transition_tables(p, clean, self.episode_index, self.replay.N_ep, self.cameras, int(seed))
            self.perturbation, self.perturb_seed, self.perturb_draws = p, int(seed), draws
        self._camera_tables(cams)
        self.views["cams"] = up(cams)
        self.windows, self.point_slots, self.point_centres = up(self.windows_host), up(self.point_slots_host), up(self.point_centres_host)
        self.perturb_M, self.perturb_colour = up(M), up(colour)

    def _upload(self, views: Dict[str, np.ndarray], stats) -> None:
        """Part three: the view tables, the atlas, a device copy of every host table that part two kept, the scales and the prompt ids."""
        from .render import load_atlas

        def up(a):
            return None if a is None else torch.from_numpy(a).to(self.E.device)

        self.views = {k: up(a) for k, a in views.items()}
        self.atlas = up(load_atlas(self.cfg.texture_dir))
        self.windows, self.point_slots, self.point_centres = up(self.windows_host), up(self.point_slots_host), up(self.point_centres_host)
        self.first_tr, self.orientation_rot = up(self.first_tr_host), up(self.orientation_rot)
        self.samples = int(self.cfg.samples)
        self.joint_std = up(np.asarray(stats[0]["std"], np.float64)[: self.A - 1].astype(np.float32)) if self.controller is not None else None
        self.prompts = [harness.make_prompt(d) for d in self.replay.descriptions]
        self.prompt_ids = torch.cat([self.agent.pipe.encode_ids([p]) for p in self.prompts]) if self.agent is not None else None


    # ---- the steps of one batch (the tests recompute a batch from these inputs)
    def batch_indices(self, start: int) -> np.ndarray:
        """Transitions ``start .. start + batch_size - 1``; past the end the last index repeats (the padding of the last batch)."""
        return np.minimum(np.arange(start, start + self.batch_size), self.N - 1).astype(np.int64)

    def targets(self, idx: np.ndarray) -> Dict[str, torch.Tensor]:
        """Steps 1 - 3: the sampled batch, the ground-truth render over its frames and the tiled canvas, all on the device."""
        E, B, V, H, W = self.E, len(idx), self.V, self.H, self.W
        batch = self.replay.sample(idx, want_u8=True)
        sel = torch.from_numpy(np.asarray(idx, np.int64)).to(E.device, non_blocking=True)
        v = {k: t.index_select(0, sel).reshape((B * V,) + tuple(t.shape[2:])).contiguous() for k, t in self.views.items()}
        if self.perturb_M is not None:  # the gathered frames warped and re-coloured, one launch; they take the clean ones' place
            counts = torch.empty((B * V,), dtype=torch.int32, device=E.device)
            warped = E.view_perturb(batch["images_u8"].view(B * V, H, W, 3), self.perturb_M.index_select(0, sel).reshape(B * V, 9),
                                    self.perturb_colour.index_select(0, sel).reshape(B * V, 6), n_revealed=counts)
            batch["images_u8"], batch["revealed"] = warped.view(tuple(batch["images_u8"].shape)), counts.view(B, V)
        frames = batch["images_u8"].view(B * V, H, W, 3)
        full = torch.empty((B * V, H, W, 3), dtype=torch.uint8, device=E.device)
        occupied = torch.empty((B * V, H, W), dtype=torch.uint8, device=E.device)
        E.render_spheres(v["cams"], v["spheres"], v["tex_index"], v["count"], self.atlas, H, W, self.samples, bg=frames, full=full, occupied=occupied)
        batch["full"], batch["occupied"], batch["views"] = full, occupied, v
        if self.windows is not None:
            batch["windows"] = self.windows.index_select(0, sel).reshape(B * V, -1, 4).contiguous()
        if V == 4:  # view v -> the tile at row v / 2, column v % 2 (tiling.CROP_ORDER): layout only
            batch["tiled"] = frames.view(B, 2, 2, H, W, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, 3)
        return batch

    def generate(self, batch, idx: np.ndarray, generator) -> torch.Tensor:
        """Step 4: the agent's pipeline on the tiled frames -> the generated tiled targets, uint8 [B, 2H, 2W, 3] on the device."""
        ep = self.episode_index[np.asarray(idx)]
        with torch.inference_mode():
            return self.agent.pipe(prompt=[self.prompts[e] for e in ep], prompt_ids=self.prompt_ids[torch.from_numpy(ep.astype(np.int64))],
                                   image=batch["tiled"], num_inference_steps=self.num_inference_steps, guidance_scale=self.guidance_scale,
                                   generator=generator, output_type="pt").images

    def _fresh_controller(self):
        c = self.controller
        if getattr(c, "_dirty", False):  # weights moved by update(): re-pack once before acting, as ``act`` does
            from .act import pack_act

            c._own_state()
            c.W = pack_act(c._sd, c.device)
            c._progs, c._dirty = {}, False

    def _chunk(self, img_bvhw3: torch.Tensor, batch) -> torch.Tensor:
        """The controller on per-view frames uint8 [B, V, H, W, 3] -> its f16 chunk, a view of the program's padded output buffer."""
        io = self.controller._run(img_bvhw3, batch["low_dim_state"].flatten(1), batch.get("lang_tokens"))
        return io.a_hat[..., : self.A]

    def _score_actions(self, a_hat, batch, tabs, row0: int, n_valid: int):
        self.E.openloop_action_metrics(a_hat, batch["action"], tabs["norm"], row0=row0, n_valid=n_valid)
        self.E.openloop_action_metrics(a_hat, batch["action"], tabs["rad"], joint_scale=self.joint_std, row0=row0, n_valid=n_valid)

    def _tables(self):
        dev, N, T = self.E.device, self.N, self.T

        def act():
            return {unit: torch.zeros((N, T, 2), dtype=torch.float32, device=dev) for unit in ("norm", "rad")}

        tabs = {"oracle": act()} if self.controller is not None else {}
        if self.agent is not None:
            if self.controller is not None:
                tabs["generated"] = act()
            tabs["image"] = torch.zeros((N, self.V, 5), dtype=torch.int64, device=dev)
            tabs["spheres"] = torch.zeros((N, self.V, int(self.windows.shape[2]), 17), dtype=torch.int64, device=dev)
            if self.orientation_rot is not None:
                tabs["orientation"] = torch.zeros((N, self.V, int(self.windows.shape[2]), int(self.orientation_rot.shape[0]), 4), dtype=torch.int64, device=dev)
        if self.perturb_M is not None:  # per view, the pixels the perturbation revealed
            tabs["revealed"] = torch.zeros((N, self.V), dtype=torch.int32, device=dev)
        if self.executions is not None:  # every scored chunk, as the controller's head wrote it
            tabs["chunks"] = {k: torch.zeros((N, T, self.A), dtype=torch.float16, device=dev) for k in ("generated", "oracle") if k in tabs}
        if self.seeds is not None:
            self._seed_tables(tabs)
        return tabs

    def _seed_tables(self, tabs) -> None:
        """With ``seeds=R``: the generated tables get a leading seed axis -- ``tabs["seed"]`` holds them whole, ``tabs["per_seed"][r]`` seed
        r's slices under the names ``run_batch`` scores into -- and seed 0's slices take the place of the tables ``_tables`` made: the
        existing names ARE the first seed."""
        dev, N, T, R = self.E.device, self.N, self.T, self.seeds
        whole = {"image": torch.zeros((R,) + tuple(tabs["image"].shape), dtype=torch.int64, device=dev),
                 "spheres": torch.zeros((R,) + tuple(tabs["spheres"].shape), dtype=torch.int64, device=dev)}
        if self.controller is not None:
            whole["generated"] = {unit: torch.zeros((R, N, T, 2), dtype=torch.float32, device=dev) for unit in ("norm", "rad")}
            whole["chunks"] = torch.zeros((R, N, T, self.A), dtype=torch.float16, device=dev)
            whole["demo"] = torch.zeros((N, T, self.A), dtype=torch.float32, device=dev)
        per = []
        for r in range(R):
            t = {"image": whole["image"][r], "spheres": whole["spheres"][r]}
            if self.controller is not None:
                t["generated"] = {unit: whole["generated"][unit][r] for unit in ("norm", "rad")}
                t["chunks"] = {"generated": whole["chunks"][r]}
            per.append(t)
        if "orientation" in tabs:  # the orientation of the first seed's spheres only
            per[0]["orientation"] = tabs["orientation"]
        tabs["image"], tabs["spheres"] = per[0]["image"], per[0]["spheres"]
        if self.controller is not None:
            tabs["generated"] = per[0]["generated"]
            if "chunks" in tabs:
                tabs["chunks"]["generated"] = per[0]["chunks"]["generated"]
        tabs["seed"], tabs["per_seed"] = whole, per

    def _keep_chunk(self, a_hat, tabs, kind: str, row0: int, n_valid: int):
        if kind in tabs.get("chunks", {}):
            tabs["chunks"][kind][row0: row0 + n_valid].copy_(a_hat[:n_valid, : self.T, : self.A])

    def seed_reductions(self, tabs):
        """After the last batch, with ``seeds``: the two reductions over the seed axis -- one ``gn_openloop_seed_spheres`` launch over the
        sphere tables and, with a controller, two ``gn_openloop_seed_actions`` launches over the chunks (normalised, then radians) ->
        ``(f64 [N, V, S, 8], {"norm" | "rad": f32 [N, T, 4]} or None)`` on the device; nothing is read back."""
        if self.seeds is None:
            return None, None
        whole = tabs["seed"]
        spheres = self.E.openloop_seed_spheres(whole["spheres"], min_ratio=self.seed_min_ratio)
        if self.controller is None:
            return spheres, None
        return spheres, {"norm": self.E.openloop_seed_actions(whole["chunks"], whole["demo"]),
                         "rad": self.E.openloop_seed_actions(whole["chunks"], whole["demo"], joint_scale=self.joint_std)}

    def replay_executions(self, tabs) -> Optional[list]:
        """After the last batch: per setting and row kind, the executed action of every transition (``gn_openloop_exec_actions`` over the chunk
        table) and its scores in both units (``gn_openloop_exec_metrics``).  Device tensors; nothing is read back."""
        if self.executions is None:
            return None
        E, dev, N, out = self.E, self.E.device, self.N, []
        for ex in self.executions:
            d = dict(ex)
            for kind, chunks in tabs["chunks"].items():
                n_calls = torch.empty((N,), dtype=torch.int32, device=dev)
                acts = E.openloop_exec_actions(chunks, self.first_tr, ex["h"], ex["temporal_agg"], ex["m"], n_calls=n_calls, first_tr_host=self.first_tr_host)
                d[kind] = {"actions": acts, "n_calls": n_calls,
                           "scores": {"norm": E.openloop_exec_metrics(acts, self.replay.action, self.first_tr),
                                      "rad": E.openloop_exec_metrics(acts, self.replay.action, self.first_tr, joint_scale=self.joint_std)}}
            for rule in self.combine or ():  # what the mode executes when the R seeds' chunks are combined first: the same two score launches
                n_calls = torch.empty((N,), dtype=torch.int32, device=dev)
                picks = torch.empty((N,), dtype=torch.int32, device=dev)
                acts, _ = E.openloop_exec_actions_samples(tabs["seed"]["chunks"], self.first_tr, ex["h"], ex["temporal_agg"], ex["m"], combine=rule,
                                                          n_calls=n_calls, pick=picks, first_tr_host=self.first_tr_host)
                d["seed_" + rule] = {"actions": acts, "n_calls": n_calls, "picks": picks,
                                     "scores": {"norm": E.openloop_exec_metrics(acts, self.replay.action, self.first_tr),
                                                "rad": E.openloop_exec_metrics(acts, self.replay.action, self.first_tr, joint_scale=self.joint_std)}}
            out.append(d)
        return out

    def triangulate_spheres(self, tabs) -> Optional[torch.Tensor]:
        """After the last batch: every drawn sphere of the finished sphere table triangulated across the views, for the generated image and
        for the ground-truth render -- one ``gn_openloop_triangulate`` launch -> f64 [N, G, 2, 8] on the device; nothing is read back."""
        if not self.triangulate:
            return None
        return self.E.openloop_triangulate(tabs["spheres"], self.windows, self.views["cams"], self.point_slots, self.point_centres,
                                           min_ratio=self.tri_min_ratio, min_det=self.tri_min_det, slot_host=self.point_slots_host, win_host=self.windows_host)

    def sphere_shifts(self, sph_rows: torch.Tensor, B: int) -> torch.Tensor:
        """``sph_rows`` int64 [n, V, S, 17], a batch's finished rows of the sphere table -> int32 [B * V, S, 2] = (dx, dy), where
        ``gn_openloop_orientation`` reads the generated image relative to each window: ``rint`` of the generated minus the true centroid in
        f64; 0 where either mass is 0, where the mass ratio is below ``SHIFT_FOUND_MASS`` and in the rows past ``n`` (the padding of a last
        batch).  Device tensors; nothing is read back."""
        t = sph_rows.to(torch.float64)
        gm, tm = t[..., 1], t[..., 5]
        ok = (gm > 0) & (tm > 0) & (gm >= SHIFT_FOUND_MASS * tm)
        one = torch.ones_like(gm)
        gm, tm = torch.where(ok, gm, one), torch.where(ok, tm, one)
        d = torch.stack([t[..., 2] / gm - t[..., 6] / tm, t[..., 3] / gm - t[..., 7] / tm], dim=-1)
        d = torch.where(ok[..., None], torch.round(d), torch.zeros_like(d)).clamp_(-127.0, 127.0).to(torch.int32)  # torch.round: half to even, rint
        out = torch.zeros((B,) + tuple(d.shape[1:]), dtype=torch.int32, device=d.device)
        out[: d.shape[0]] = d
        return out.view(B * d.shape[1], d.shape[2], 2)

    def _score_generated(self, batch, idx, generator, tabs, start: int, n_valid: int) -> None:
        """Steps 4 - 6 for one generator: the pipeline, the controller on its image, and the image, sphere and action scores into ``tabs``."""
        B = len(idx)
        gen = self.generate(batch, idx, generator)
        if self.controller is not None:
            a_hat = self.controller.act_tiled(gen, batch["low_dim_state"], batch.get("lang_tokens"))
        self.E.openloop_image_metrics(gen, batch["full"], batch["occupied"], tabs["image"], row0=start, n_valid=n_valid)
        self.E.openloop_sphere_metrics(gen, batch["full"], batch["images_u8"].view(B * self.V, self.H, self.W, 3), batch["occupied"],
                                       batch["windows"], tabs["spheres"], threshold=self.change_threshold, row0=start, n_valid=n_valid)
        if "orientation" in tabs:
            v = batch["views"]
            self.E.openloop_orientation(gen, batch["full"], batch["occupied"], batch["windows"], v["cams"], v["spheres"], v["tex_index"], v["count"],
                                        self.atlas, self.orientation_rot, tabs["orientation"], samples=self.samples,
                                        shift=self.sphere_shifts(tabs["spheres"][start: start + n_valid], B), row0=start, n_valid=n_valid)
        if self.controller is not None:
            self._score_actions(a_hat, batch, tabs["generated"], start, n_valid)  # before the next pass overwrites the program's chunk
            self._keep_chunk(a_hat, tabs, "generated", start, n_valid)

    def run_batch(self, start: int, tabs, generator) -> None:
        """One evaluator batch: steps 1 - 7 for transitions ``start ..``, everything on the device, nothing read back.  With ``seeds``,
        ``generator`` is the list of the R generators: the targets are made once, steps 4 - 6 run per seed in order into that seed's tables
        (seed 0's are ``tabs``' own, and only they carry an orientation table), and the oracle pass runs once."""
        if self.controller is not None:
            self._fresh_controller()
        idx = self.batch_indices(start)
        n_valid = min(self.batch_size, self.N - start)
        with torch.inference_mode():  # as harness.control_step runs the same two programs
            batch = self.targets(idx)
            B = len(idx)
            if "revealed" in tabs:
                tabs["revealed"][start: start + n_valid].copy_(batch["revealed"][:n_valid])
            if self.agent is not None and self.seeds is None:
                self._score_generated(batch, idx, generator, tabs, start, n_valid)
            elif self.agent is not None:
                for r, g in enumerate(generator):
                    # seed r's chunk leaves the program's output buffer (into its slice of the chunk table) before seed r + 1's act_tiled
                    self._score_generated(batch, idx, g, tabs["per_seed"][r], start, n_valid)
                if self.controller is not None:
                    tabs["seed"]["demo"][start: start + n_valid].copy_(batch["action"][:n_valid])
            if self.controller is not None:
                a_hat = self._chunk(batch["full"].view(B, self.V, self.H, self.W, 3), batch)
                self._score_actions(a_hat, batch, tabs["oracle"], start, n_valid)
                self._keep_chunk(a_hat, tabs, "oracle", start, n_valid)

    def run(self) -> OpenLoopResult:
        tabs = self._tables()
        generator = torch.Generator(device=self.E.device).manual_seed(self.seed) if self.agent is not None else None
        if self.seeds is not None:  # one generator per seed, each advanced call by call as the one of a run with that seed is
            generator = [torch.Generator(device=self.E.device).manual_seed(self.seed + r) for r in range(self.seeds)]
        for start in range(0, self.N, self.batch_size):
            self.run_batch(start, tabs, generator)
        dev = {"actions": {k: tabs[k] for k in ("generated", "oracle") if k in tabs}, "image": tabs.get("image"), "spheres": tabs.get("spheres"),
               "points": self.triangulate_spheres(tabs), "orientation": tabs.get("orientation"), "executions": self.replay_executions(tabs),
               "chunks": tabs.get("chunks")}
        if "revealed" in tabs:
            dev["revealed"] = tabs["revealed"]
        if self.seeds is not None:  # the first seed's tables travel once, inside the seed tables, and are sliced out of them on the host
            dev["seed_spheres"], dev["seed_actions"] = self.seed_reductions(tabs)
            dev["seed_tables"] = tabs["seed"]
            dev["image"] = dev["spheres"] = None
            dev["actions"] = {k: t for k, t in dev["actions"].items() if k != "generated"}
            if dev["chunks"] is not None:
                dev["chunks"] = {k: t for k, t in dev["chunks"].items() if k != "generated"}
        # the one device-to-host copy, after the last launch: every table by its name in the tree, as bytes of one buffer
        named: Dict[str, torch.Tensor] = {}
        _map_tensors(dev, named.__setitem__)
        copies = read_back(named)
        host = _map_tensors(dev, lambda name, t: copies[name])
        extra = {}
        if "revealed" in host:
            from .perturb import draw_ranges

            extra = dict(revealed=host["revealed"], perturbation={"setting": self.perturbation.describe(), "seed": self.perturb_seed,
                                                                  "draws": draw_ranges(self.perturb_draws)})
        if self.seeds is not None:
            st = host["seed_tables"]
            host["image"], host["spheres"] = st["image"][0], st["spheres"][0]
            if "generated" in st:
                host["actions"] = dict({"generated": {unit: t[0] for unit, t in st["generated"].items()}}, **host["actions"])
                if host["chunks"] is not None:
                    host["chunks"] = dict({"generated": st["chunks"][0]}, **host["chunks"])
            extra = dict(extra, seeds=[self.seed + r for r in range(self.seeds)], seed_tables=st, seed_spheres=host["seed_spheres"], seed_actions=host["seed_actions"])
        return OpenLoopResult(host["image"], host["actions"], self.episode_index, self.step_index, self.task_index, self.tasks, self.cameras, self.A - 1,
                              self.H, self.W, spheres=host["spheres"], windows=self.windows_host if host["spheres"] is not None else None,
                              executions=host["executions"], chunks=host["chunks"], points=host["points"], point_slots=self.point_slots_host,
                              point_centres=self.point_centres_host, cams=self.cams_host, orientation=host["orientation"],
                              orientation_angles=self.orientation_angles if host["orientation"] is not None else None, **extra)


def robustness_sweep(ev: OpenLoopEval, settings, found_mass: float = 0.5, seed: int = 0) -> Dict:
    """The clean evaluator, then each of ``settings`` (``perturb.Perturbation``s, preset names or specs, each drawn with ``seed``) on the same
    evaluator -- the same programs, the same generator seeds -- and the clean tables put back at the end, whatever happened.  ->

    ``{"clean": validator_scalars(found_mass) of the clean run, "n", "settings": [...]}``, one entry per setting: ``setting`` (its
    ``describe()``), ``seed``, ``draws`` (the ranges drawn), ``scores`` (``validator_scalars(found_mass)`` under it), ``delta`` (scores minus
    clean, None where either is), ``revealed_share`` and ``lost_spheres``, the number of spheres the clean run drew whose window is empty
    after the perturbation (they left the view, so their scores are about other spheres than the clean run's).  When the evaluator has
    ``seeds``, each entry also holds ``delta_over_std``: the delta over the CLEAN run's seed-to-seed standard deviation of that score (None
    where there is none or it is 0) -- a ratio to read, not a verdict.  Open-loop like every score here: a score under a perturbation is
    still not a success rate, and revealed borders are mirrored scene, not what a rotated camera would have seen there."""
    from . import perturb as PB

    if ev.agent is None:
        raise ValueError("robustness_sweep: the scores are the generated image's; it needs an evaluator with a diffusion agent")
    settings = [PB.parse(s) for s in settings]
    try:
        ev.set_perturbation(None)
        clean = ev.run()
        base = clean.validator_scalars(found_mass)
        std = {k: v["std"] for k, v in clean.seed_summary(found_mass)["scores"].items()} if clean.seeds is not None else None
        drawn = clean.sphere_drawn()
        out: Dict = {"clean": base, "n": len(clean), "settings": []}
        for p in settings:
            ev.set_perturbation(p, seed)
            res = ev.run()
            scores = res.validator_scalars(found_mass)
            delta = {k: None if scores[k] is None or base[k] is None else scores[k] - base[k] for k in base}
            entry = {"setting": p.describe(), "seed": int(seed), "draws": res.perturbation["draws"], "scores": scores, "delta": delta,
                     "revealed_share": res.revealed_share(), "lost_spheres": PB.lost_windows(clean.windows, res.windows, drawn)}
            if std is not None:
                entry["delta_over_std"] = {k: None if delta[k] is None or not std.get(k) else delta[k] / std[k] for k in base}
            out["settings"].append(entry)
        return out
    finally:
        ev.set_perturbation(None)


def controller_validator(episodes, cameras: Sequence[str] = DEFAULT_CAMERAS, *, render_cfg, stats, tokenizer=None, batch_size: int = 8, engine=None,
                         execution=None):
    """-> a ``validate`` callable for ``ControllerTrainLoop``: ``(agent, epochs_done) -> {"select", "joint_l1_norm", "joint_l1_rad",
    "gripper_acc", "n"}``.  It scores the controller ALONE on held-out demos with the ground-truth targets (the oracle row: sample, render,
    controller; no diffusion agent), reads the agent's current weights and changes none; ``select`` is the normalised joint L1, so
    ``best.pt`` follows its minimum.  The demo set is loaded onto the device at the first call and kept.

    ``execution = (execution_horizon, temporal_agg[, m])``: the mode the controller will be run with.  ``select`` is then the normalised joint
    L1 of the EXECUTED action under that mode (``OpenLoopResult.execution_summary``), and the dict gains ``exec_joint_l1_norm``,
    ``exec_joint_l1_rad``, ``exec_gripper_acc``, ``exec_jump_boundary_norm``, ``exec_jump_inside_norm`` (None where no step qualifies) and
    ``exec_calls_per_step``.  Without it the dict is as before."""
    state: Dict = {}

    def validate(agent, epochs_done: int) -> Dict[str, float]:
        ev = state.get("ev")
        if ev is None or ev.controller is not agent:
            ev = state["ev"] = OpenLoopEval(None, agent, episodes, cameras, render_cfg=render_cfg, stats=stats, tokenizer=tokenizer,
                                            batch_size=batch_size, engine=engine, executions=None if execution is None else [execution])
        res = ev.run()
        s = res.summary()["oracle"]
        out = {"select": s["joint_l1_norm"], "joint_l1_norm": s["joint_l1_norm"], "joint_l1_rad": s["joint_l1_rad"],
               "gripper_acc": s["gripper_acc"], "n": float(len(ev.replay))}
        if execution is not None:
            x = res.execution_summary()[0]
            o = x["oracle"]
            out.update(select=o["joint_l1_norm"], exec_joint_l1_norm=o["joint_l1_norm"], exec_joint_l1_rad=o["joint_l1_rad"],
                       exec_gripper_acc=o["gripper_acc"], exec_jump_boundary_norm=o["jump_boundary_norm"], exec_jump_inside_norm=o["jump_inside_norm"],
                       exec_calls_per_step=x["calls_per_step"])
        return out

    return validate


VALIDATION_JSONL = "validation.jsonl"


def diffusion_validator(make_pipe, episodes, cameras: Sequence[str] = DEFAULT_CAMERAS, *, render_cfg, out_dir=None, tokenizer=None, batch_size: int = 8,
                        num_inference_steps: int = 5, seed: int = 0, engine=None, triangulate: bool = False, tri_min_ratio: float = 0.5,
                        tri_min_det: float = 1e-6, orientation=None, seeds: Optional[int] = None, seed_min_ratio: float = 0.5):
    """-> a ``validate(global_step)`` callable for ``train_loop.TrainLoop``: each call wraps ``make_pipe()`` (for instance
    ``validation.validation_pipeline(..., trainer, "euler_discrete")`` over the trainer's current weights) as the agent of a diffusion-only
    ``OpenLoopEval`` on held-out demos and returns ``{"step", "select", "found_rate", "shift_px", "mass_ratio", "spread_ratio", "colour_l1",
    "sphere_rmse", "background_rmse", "wrapped_mse", "n"}`` -- ``select`` is ``summary()["image"]["spheres"]["score"]`` (lower is better), the
    sphere fields are its ``overall`` block, the two RMSEs the means over all cameras.  With ``out_dir`` the dict is also appended as one JSON
    line to ``<out_dir>/validation.jsonl``.  The demo set is loaded onto the device at the first call and kept; later calls swap the agent.
    ``TrainLoop`` ignores the return value; it is there for callers that rank checkpoints themselves.

    ``triangulate``: the evaluator's option; the dict then gains ``err_3d_mm`` (the mean 3D error of the generated spheres,
    ``triangulation_summary()["generated"]["err_mm"]``) and ``excess_mm`` (what of it is the model's own); ``tri_min_ratio`` and
    ``tri_min_det`` are the evaluator's and are read only with it.  ``select`` stays what it is.

    ``orientation``: the evaluator's option (None, K or a dict); the dict then gains ``orient_err_deg``, the mean orientation error of the
    scored spheres (``orientation_summary()["overall"]["err_deg"]``; None where none was scored).

    ``seeds``: the evaluator's option (None or R); ``select`` and every other field stay the FIRST seed's numbers, so lines with and without
    the option rank alike, and the dict gains ``select_mean`` and ``select_std`` (``seed_summary()["scores"]["select"]``: the mean over the
    seeds and the seed-to-seed standard deviation, the noise floor a difference between two lines has to beat) and ``variance_share``
    (``seed_summary()["spheres"]["overall"]``: 0 all bias, 1 all noise).  ``seed_min_ratio`` is the evaluator's and is read only with it."""
    import types

    state: Dict = {}
    # the three options reach the evaluator only when triangulate is on: with it off OpenLoopEval is called with exactly the arguments it was
    # called with before the option existed (tests/test_sphere_metrics_cpu.py compares them), so the default path cannot have changed
    tri = dict(triangulate=True, tri_min_ratio=tri_min_ratio, tri_min_det=tri_min_det) if triangulate else {}
    if orientation is not None:  # likewise: only when it is on
        tri["orientation"] = orientation
    if seeds is not None:  # likewise
        tri.update(seeds=seeds, seed_min_ratio=seed_min_ratio)

    def validate(global_step: int) -> Dict:
        agent = types.SimpleNamespace(pipe=make_pipe())
        ev = state.get("ev")
        if ev is None:
            ev = state["ev"] = OpenLoopEval(agent, None, episodes, cameras, render_cfg=render_cfg, stats=None, tokenizer=tokenizer, batch_size=batch_size,
                                            num_inference_steps=num_inference_steps, seed=seed, engine=engine, **tri)
        ev.agent = agent
        res = ev.run()
        line = dict({"step": int(global_step)}, **res.validator_scalars(), n=len(res))
        if triangulate:
            s3 = res.triangulation_summary()
            line.update(err_3d_mm=s3["generated"]["err_mm"], excess_mm=s3["excess_mm"])
        if orientation is not None:
            line.update(orient_err_deg=res.orientation_summary()["overall"]["err_deg"])
        if seeds is not None:
            ss = res.seed_summary()
            line.update(select_mean=ss["scores"]["select"]["mean"], select_std=ss["scores"]["select"]["std"],
                        variance_share=ss["spheres"]["overall"]["variance_share"])
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, VALIDATION_JSONL), "a") as f:
                f.write(json.dumps(line) + "\n")
        return line

    return validate
