"""The pixel rule of ``gn_view_perturb`` (include/genima_hip.h states it), restated in numpy f64 one rounded operation at a time, for
tests/test_perturb_cpu.py, tests/test_view_perturb_gpu.py and tests/test_openloop_perturb_gpu.py.

TEST INFRASTRUCTURE ONLY.  It is the reference the kernel is compared with bit for bit and goes through nothing of genima_amd: every numpy
ufunc call below is one IEEE f64 operation per element (numpy fuses nothing), in the order the header writes them.
"""
from __future__ import annotations

import numpy as np


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _fold(i, n: int):
    """One reflection about the edge pixel's centre (i < 0 -> -i, else i > n - 1 -> 2 (n - 1) - i), then the clamp to [0, n - 1]."""
    i = np.where(i < 0, -i, np.where(i > n - 1, 2 * (n - 1) - i, i))
    return np.clip(i, 0, n - 1)


def view_perturb(src, M, colour):
    """``src`` uint8 [B, H, W, 3], ``M`` f64 [B, 9], ``colour`` f64 [B, 6] (gain rgb | offset rgb) -> ``(dst uint8 [B, H, W, 3], valid uint8
    [B, H, W], n_revealed int32 [B])``."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[3] == 3
    B, H, W = src.shape[:3]
    M, colour = np.asarray(M, np.float64).reshape(B, 9), np.asarray(colour, np.float64).reshape(B, 6)
    dst, valid = np.zeros_like(src), np.zeros((B, H, W), np.uint8)
    X = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    Y = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        for b in range(B):
            m = M[b]
            a = (m[0] * X + m[1] * Y) + m[2]
            c = (m[3] * X + m[4] * Y) + m[5]
            w = (m[6] * X + m[7] * Y) + m[8]
            ok = (w > 0.0) & np.isfinite(a) & np.isfinite(c) & np.isfinite(w)
            ws = np.where(ok, w, 1.0)  # the refused pixels are overwritten below: any divisor does
            u, v = np.where(ok, a, 0.0) / ws, np.where(ok, c, 0.0) / ws
            valid[b] = ok & (u >= 0.0) & (u <= float(W)) & (v >= 0.0) & (v <= float(H))
            su = _clamp(u - 0.5, -float(W - 1), 2.0 * float(W - 1))
            sv = _clamp(v - 0.5, -float(H - 1), 2.0 * float(H - 1))
            fx, fy = np.floor(su), np.floor(sv)
            tx, ty = su - fx, sv - fy
            x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
            xa, xb, ya, yb = _fold(x0, W), _fold(x0 + 1, W), _fold(y0, H), _fold(y0 + 1, H)
            img = src[b].astype(np.float64)
            p00, p01, p10, p11 = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]  # [H, W, 3]
            tx, ty = tx[..., None], ty[..., None]
            top = p00 * (1.0 - tx) + p01 * tx
            bot = p10 * (1.0 - tx) + p11 * tx
            cc = top * (1.0 - ty) + bot * ty
            t = cc * colour[b, None, None, :3] + colour[b, None, None, 3:]
            t = np.where(t > 0.0, np.where(t > 255.0, 255.0, t), 0.0)  # clamp(t, 0, 255); a NaN gives 0
            out = np.rint(t).astype(np.uint8)  # half to even
            dst[b] = np.where(ok[..., None], out, 0)
    n_revealed = (valid == 0).reshape(B, -1).sum(axis=1).astype(np.int32)
    return dst, valid, n_revealed


def identity(B: int):
    """-> (M f64 [B, 9], colour f64 [B, 6]): the identity of both parts."""
    return np.tile(np.eye(3).reshape(1, 9), (B, 1)), np.tile(np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]), (B, 1))


def project(cam, point):
    """``gn_render_spheres``' ray rule inverted for one f32 camera row [18] and one world point [3], in f64 -> (u, v) pixels: the pixel whose
    ray ``R (dx, dy, -1)`` passes through the point, R as the table stores it (solved, not transposed: an f32 R is not exactly orthonormal)."""
    cam = np.asarray(cam, np.float64)
    pose = cam[4:16].reshape(3, 4)
    p = np.linalg.solve(pose[:, :3], np.asarray(point, np.float64) - pose[:, 3])
    z = -p[2]
    return cam[2] + cam[0] * p[0] / z, cam[3] - cam[1] * p[1] / z


def through(M, u, v):
    """Pixel (u, v) through the homography ``M`` [9] -> the source pixel."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    q = M @ np.array([u, v, 1.0])
    return q[0] / q[2], q[1] / q[2]
