"""``gn_openloop_sphere_metrics``' 17 columns and the values ``OpenLoopResult`` derives from them, restated in plain numpy from the rule
include/genima_hip.h states, for tests/test_sphere_metrics_cpu.py, tests/test_sphere_metrics_gpu.py and tests/test_openloop_spheres_gpu.py.

TEST INFRASTRUCTURE ONLY: int64 sums, f64 derived values; nothing of genima_amd is imported.
"""
from __future__ import annotations

import numpy as np


def sphere_metrics(gen: np.ndarray, gt: np.ndarray, cond: np.ndarray, occupied: np.ndarray, win: np.ndarray, threshold: int) -> np.ndarray:
    """gen, gt, cond uint8 [B, V, H, W, 3], occupied uint8 [B, V, H, W], win int32 [B, V, S, 4] = (x0, y0, x1, y1) half-open and valid
    (inside the image, x0 <= x1, y0 <= y1) -> int64 [B, V, S, 17]."""
    B, V, S = win.shape[:3]
    out = np.zeros((B, V, S, 17), np.int64)
    for b in range(B):
        for v in range(V):
            for s in range(S):
                x0, y0, x1, y1 = (int(q) for q in win[b, v, s])
                if x1 <= x0 or y1 <= y0:
                    continue  # an empty window: 17 zeros
                g, t, c = (a[b, v, y0:y1, x0:x1].astype(np.int64) for a in (gen, gt, cond))
                occ = occupied[b, v, y0:y1, x0:x1] != 0
                ly, lx = np.mgrid[0:y1 - y0, 0:x1 - x0].astype(np.int64)
                row = [(x1 - x0) * (y1 - y0)]
                for img in (g, t):
                    a = np.maximum(0, np.abs(img - c).sum(axis=-1) - int(threshold))
                    row += [a.sum(), (a * lx).sum(), (a * ly).sum(), (a * (lx * lx + ly * ly)).sum()]
                row += [occ.sum(), (((g - t) ** 2).sum(axis=-1) * occ).sum()]
                row += [(img[..., k] * occ).sum() for img in (g, t) for k in range(3)]
                out[b, v, s] = row
    return out


def derived(tab: np.ndarray):
    """int64 [..., 17] -> dict of f64 [...]: ``shift``, ``mass_ratio``, ``spread_ratio``, ``colour_l1``; NaN where the ground truth drew
    nothing (column 5 == 0), and where the quantity has no value (no generated mass; a true spread of 0; no occupied pixel)."""
    t = tab.astype(np.float64)
    nan = np.full(t.shape[:-1], np.nan)

    def moments(o):
        m = t[..., o]
        with np.errstate(divide="ignore", invalid="ignore"):
            cx, cy, r2 = (np.where(m > 0, t[..., o + k] / m, np.nan) for k in (1, 2, 3))
            return cx, cy, np.sqrt(np.maximum(0.0, r2 - cx * cx - cy * cy))

    (gx, gy, gs), (tx, ty, ts) = moments(1), moments(5)
    drawn = t[..., 5] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        colour = np.abs(t[..., 11:14] - t[..., 14:17]).mean(axis=-1) / t[..., 9]
        return {"shift": np.where(drawn, np.hypot(gx - tx, gy - ty), nan), "mass_ratio": np.where(drawn, t[..., 1] / t[..., 5], nan),
                "spread_ratio": np.where(drawn & (ts > 0), gs / ts, nan), "colour_l1": np.where(drawn & (t[..., 9] > 0), colour, nan)}
