"""``gn_openloop_triangulate``'s rule (include/genima_hip.h) and the group tables of ``OpenLoopEval(triangulate=True)``, restated in numpy f64
for tests/test_triangulate_cpu.py and tests/test_triangulate_gpu.py.

TEST INFRASTRUCTURE ONLY, written from the stated rule and not from the kernel: one ray at a time with matrices, ``np.linalg.solve`` and
``np.linalg.det`` where the kernel writes the adjugate out, the ray distance through a cross product where the kernel subtracts the
projection.  Nothing of genima_amd is imported.
"""
from __future__ import annotations

import numpy as np


def group_tables(spheres, count, windows):
    """spheres [N, V, S, 16], count [N, V], windows int32 [N, V, S, 4] -> (slot int32 [N, G, V], centre f64 [N, G, 3]): one group per
    distinct world centre (the pose's translation column, exact f64 equality) among the drawn spheres ``s < count`` of a transition, in order
    of first appearance; slot -1 where a view does not draw the group or its window is (0, 0, 0, 0); G the largest group count, at least 1."""
    sph = np.asarray(spheres, np.float64)
    N, V, S = sph.shape[:3]
    per_n = []
    for n in range(N):
        keys, rows = [], []
        for v in range(V):
            for s in range(int(count[n][v])):
                key = (float(sph[n, v, s, 3]), float(sph[n, v, s, 7]), float(sph[n, v, s, 11]))
                if key not in keys:
                    keys.append(key)
                    rows.append([-1] * V)
                g = keys.index(key)
                if rows[g][v] < 0 and tuple(int(q) for q in windows[n][v][s]) != (0, 0, 0, 0):
                    rows[g][v] = s
        per_n.append((keys, rows))
    G = max(1, max(len(k) for k, _ in per_n)) if per_n else 1
    slot, centre = np.full((N, G, V), -1, np.int32), np.zeros((N, G, 3))
    for n, (keys, rows) in enumerate(per_n):
        for g in range(len(keys)):
            slot[n, g], centre[n, g] = rows[g], keys[g]
    return slot, centre


def observe(cam, point, exact: bool = True):
    """The image coordinates (u, v) of a world point in a camera table [18].  ``exact``: the renderer's ray rule inverted exactly, p = R^-1
    (point - t) -- the ray through (u, v) then passes through the point to f64 rounding.  Otherwise ``render.sphere_windows``' p = R^T (point -
    t), which is what the rule's reprojection column uses; the two differ by how far the f32 rotation of a camera table is from orthonormal
    (about 1e-7 relative)."""
    cam = np.asarray(cam, np.float64)
    pose = cam[4:16].reshape(3, 4)
    d = np.asarray(point, np.float64) - pose[:, 3]
    p = np.linalg.solve(pose[:, :3], d) if exact else pose[:, :3].T @ d
    z = -p[2]
    return cam[2] + cam[0] * p[0] / z, cam[3] - cam[1] * p[1] / z


def triangulate(sph, win, cams, slot, centre, min_ratio: float = 0.5, min_det: float = 1e-6) -> np.ndarray:
    """sph int64 [N, V, S, 17], win int32 [N, V, S, 4], cams [N, V, 18], slot int32 [N, G, V], centre f64 [N, G, 3] -> f64 [N, G, 2, 8]."""
    sph, cams = np.asarray(sph), np.asarray(cams, np.float64)
    N, V, S = sph.shape[:3]
    G = slot.shape[1]
    out = np.full((N, G, 2, 8), np.nan)
    for n in range(N):
        for g in range(G):
            for kind in (0, 1):
                rays = []
                for v in range(V):
                    s = int(slot[n, g, v])
                    if not 0 <= s < S:
                        continue
                    gen_m, gt_m = float(sph[n, v, s, 1]), float(sph[n, v, s, 5])
                    if not gt_m > 0 or (kind == 0 and not (gen_m > 0 and gen_m >= min_ratio * gt_m)):
                        continue
                    o = 1 if kind == 0 else 5
                    m = float(sph[n, v, s, o])
                    u = float(win[n, v, s, 0]) + float(sph[n, v, s, o + 1]) / m + 0.5
                    w = float(win[n, v, s, 1]) + float(sph[n, v, s, o + 2]) / m + 0.5
                    fx, fy, cx, cy = cams[n, v, :4]
                    pose = cams[n, v, 4:16].reshape(3, 4)
                    d = pose[:, :3] @ np.array([(u - cx) / fx, (cy - w) / fy, -1.0])
                    rays.append((pose[:, 3].copy(), d / np.linalg.norm(d), u, w, v))
                out[n, g, kind, 0], out[n, g, kind, 7] = len(rays), 0.0
                if len(rays) < 2:
                    continue
                A, b = np.zeros((3, 3)), np.zeros(3)
                for o_, d, *_ in rays:
                    P = np.eye(3) - np.outer(d, d)
                    A += P
                    b += P @ o_
                det = np.linalg.det(A) / (np.trace(A) / 3.0) ** 3
                out[n, g, kind, 7] = det
                if not det >= min_det:
                    continue
                x = np.linalg.solve(A, b)
                ray2 = px2 = 0.0
                for o_, d, u, w, v in rays:
                    ray2 += float(np.sum(np.cross(x - o_, d) ** 2))
                    pose = cams[n, v, 4:16].reshape(3, 4)
                    z = -(pose[:, :3].T @ (x - pose[:, 3]))[2]
                    ur, wr = observe(cams[n, v], x, exact=False)
                    px2 += (ur - u) ** 2 + (wr - w) ** 2 if z > 0 else np.nan
                out[n, g, kind, 1:4] = x
                out[n, g, kind, 4] = np.linalg.norm(x - centre[n, g])
                out[n, g, kind, 5] = np.sqrt(ray2 / len(rays))
                out[n, g, kind, 6] = np.sqrt(px2 / len(rays))
    return out


def table_from_observations(obs, gen_obs=None, mass: int = 1 << 40, S: int = 4):
    """Build a sphere table whose centroids are given observations EXACTLY enough: ``obs[n][v][s] = (u, v) | None`` -> (sph int64
    [N, V, S, 17], win int32 [N, V, S, 4]).  A window is 12 x 12 and starts at the pixel that holds the point less 4, or at the image's
    border 0; the sums are ``mass * local`` rounded to integers, so the centroid is the point to within 1 / mass = 1e-12 of a pixel (and every
    sum stays below 2^44, exact in f64).  ``gen_obs`` (default: ``obs``) fills the generated columns and has to lie inside the same window (the
    table's sums are unsigned); None in either leaves that mass 0."""
    N, V = len(obs), len(obs[0])
    sph, win = np.zeros((N, V, S, 17), np.int64), np.zeros((N, V, S, 4), np.int32)
    gen_obs = obs if gen_obs is None else gen_obs
    for n in range(N):
        for v in range(V):
            for s in range(S):
                p = obs[n][v][s] if s < len(obs[n][v]) else None
                q = gen_obs[n][v][s] if s < len(gen_obs[n][v]) else None
                if p is None:
                    continue
                x0, y0 = max(0, int(np.floor(p[0])) - 4), max(0, int(np.floor(p[1])) - 4)
                win[n, v, s] = (x0, y0, x0 + 12, y0 + 12)
                sph[n, v, s, 0] = 144
                for o, pt in ((5, p), (1, q)):
                    if pt is not None:
                        sph[n, v, s, o] = mass
                        sph[n, v, s, o + 1] = int(round(mass * (pt[0] - 0.5 - x0)))
                        sph[n, v, s, o + 2] = int(round(mass * (pt[1] - 0.5 - y0)))
                        assert 0 <= pt[0] - 0.5 - x0 <= 11 and 0 <= pt[1] - 0.5 - y0 <= 11, (n, v, s, pt, x0, y0)
    return sph, win
