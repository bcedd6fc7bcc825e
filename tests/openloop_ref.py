"""The two scoring rules of the open-loop evaluation (``gn_openloop_image_metrics`` / ``gn_openloop_action_metrics``; include/genima_hip.h
states them), restated in plain numpy for tests/test_openloop_cpu.py, tests/test_openloop_metrics_gpu.py and tests/test_openloop_gpu.py.

TEST INFRASTRUCTURE ONLY: int64 sums for the image rule, f64 for the action sum; nothing of genima_amd is imported.
"""
from __future__ import annotations

import numpy as np


def untile(tiled: np.ndarray) -> np.ndarray:
    """uint8 [B, 2H, 2W, 3] -> [B, 4, H, W, 3]: view v is the tile at row v // 2, column v % 2."""
    B, H2, W2, _ = tiled.shape
    H, W = H2 // 2, W2 // 2
    return np.stack([tiled[:, (v // 2) * H:(v // 2 + 1) * H, (v % 2) * W:(v % 2 + 1) * W] for v in range(4)], axis=1)


def image_metrics(gen: np.ndarray, gt: np.ndarray, occupied: np.ndarray) -> np.ndarray:
    """gen, gt uint8 [B, V, H, W, 3], occupied uint8 [B, V, H, W] -> int64 [B, V, 5] = (se_in, n_in, se_out, n_out, wrap_sq)."""
    d = gen.astype(np.int64) - gt.astype(np.int64)
    se = (d * d).sum(axis=-1)  # per pixel
    inside = occupied != 0
    w = d & 255
    wrap = ((w * w) & 255).sum(axis=(-1, -2, -3))
    return np.stack([(se * inside).sum(axis=(-1, -2)), inside.sum(axis=(-1, -2)), (se * ~inside).sum(axis=(-1, -2)), (~inside).sum(axis=(-1, -2)), wrap],
                    axis=-1).astype(np.int64)


def action_metrics(a_hat: np.ndarray, actions: np.ndarray, scale=None):
    """a_hat f16 [B, T, A], actions f32 [B, T, A], scale f32 [A - 1] or None -> (joint sums f64 [B, T], gripper flags f64 [B, T], bound f64
    [B, T]).  bound = (A + 2) 2^-24 sum_j scale_j |d_j|: each device term is one f32 subtraction of exactly converted halves (relative error
    2^-24), one f32 multiplication (2^-24) and takes part in at most A - 2 f32 additions of the sequential sum of A - 1 terms."""
    A = actions.shape[-1]
    s = np.ones(A - 1, np.float64) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
    d = np.abs(a_hat[..., : A - 1].astype(np.float64) - actions[..., : A - 1].astype(np.float64)) * s
    total = d.sum(axis=-1)
    flag = ((a_hat[..., A - 1].astype(np.float64) > 0) == (actions[..., A - 1].astype(np.float64) > 0.5)).astype(np.float64)
    return total, flag, (A + 2) * 2.0 ** -24 * total
