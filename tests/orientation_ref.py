"""``gn_openloop_orientation``'s rule (include/genima_hip.h) restated in plain numpy: the pose composition elementwise in f64 in the stated
order (no ``@``), and the four integer sums per (view, sphere, candidate) given the candidates' images.  The images themselves come from
whoever draws them: ``gn_render_spheres`` in the GPU tests, tests/render_reference.py on the CPU."""
import numpy as np

SHIFT_MAX = 127
WIN_MAX = 256


def compose(spheres: np.ndarray, s: int, R) -> np.ndarray:
    """``spheres`` f32 [S, 16], one view's table -> a copy whose sphere ``s`` has the rotation ``Rs * R`` (``R`` f32 [9], row-major):
    ``Rs_k[i][l] = (float)((double)Rs[i][0] * R[0][l] + (double)Rs[i][1] * R[1][l] + (double)Rs[i][2] * R[2][l])``, added left to right."""
    out = np.array(spheres, np.float32, copy=True)
    Rs, R = np.asarray(spheres, np.float32)[s], np.asarray(R, np.float32).reshape(9)
    for i in range(3):
        for l in range(3):
            t = np.float64(Rs[i * 4 + 0]) * np.float64(R[0 * 3 + l])
            t = t + np.float64(Rs[i * 4 + 1]) * np.float64(R[1 * 3 + l])
            t = t + np.float64(Rs[i * 4 + 2]) * np.float64(R[2 * 3 + l])
            out[s, i * 4 + l] = np.float32(t)
    return out


def candidate_tables(spheres: np.ndarray, rot: np.ndarray) -> np.ndarray:
    """``spheres`` f32 [n, S, 16], ``rot`` f32 [K, 9] -> f32 [n, S, K, S, 16]: for every view, sphere slot and candidate the view's whole
    table with that one sphere rotated."""
    n, S = spheres.shape[:2]
    K = len(rot)
    out = np.empty((n, S, K, S, 16), np.float32)
    for i in range(n):
        for s in range(S):
            for k in range(K):
                out[i, s, k] = compose(spheres[i], s, rot[k])
    return out


def clamp_window(w, H: int, W: int):
    """The kernel's clamp of one window ``(x0, y0, x1, y1)`` -> ``(x0, y0, width, height)``."""
    x0, y0 = min(max(int(w[0]), 0), W), min(max(int(w[1]), 0), H)
    wd = min(max(min(max(int(w[2]), 0), W) - x0, 0), WIN_MAX)
    ht = min(max(min(max(int(w[3]), 0), H) - y0, 0), WIN_MAX)
    return x0, y0, wd, ht


def orientation_sums(cand: np.ndarray, gen: np.ndarray, gt: np.ndarray, occupied: np.ndarray, win: np.ndarray, shift=None) -> np.ndarray:
    """``cand`` uint8 [n, S, K, H, W, 3] (the candidates' raw renders), ``gen`` / ``gt`` uint8 [n, H, W, 3] per VIEW (a tiled ``gen`` is
    untiled by the caller), ``occupied`` [n, H, W], ``win`` int32 [n, S, 4], ``shift`` int32 [n, S, 2] or None -> int64 [n, S, K, 4]:
    the sums over the window's occupied pixels, pixel by pixel in integers."""
    n, S, K, H, W = cand.shape[:5]
    out = np.zeros((n, S, K, 4), np.int64)
    for i in range(n):
        for s in range(S):
            x0, y0, wd, ht = clamp_window(win[i, s], H, W)
            dx, dy = (0, 0) if shift is None else (min(max(int(d), -SHIFT_MAX), SHIFT_MAX) for d in shift[i, s])
            ys, xs = np.nonzero(np.asarray(occupied[i, y0: y0 + ht, x0: x0 + wd]) != 0)
            ys, xs = ys + y0, xs + x0
            inside = (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H)
            g = gen[i, (ys + dy)[inside], (xs + dx)[inside]].astype(np.int64)
            t = gt[i, ys, xs].astype(np.int64)
            for k in range(K):
                c = cand[i, s, k, ys, xs].astype(np.int64)
                out[i, s, k] = (((c[inside] - g) ** 2).sum(), int(inside.sum()), ((c - t) ** 2).sum(), len(xs))
    return out


def untile(gen: np.ndarray) -> np.ndarray:
    """uint8 [B, 2H, 2W, 3] -> [B * 4, H, W, 3]: view v is the tile at row v / 2, column v % 2."""
    B, H2, W2 = gen.shape[:3]
    H, W = H2 // 2, W2 // 2
    return np.ascontiguousarray(gen.reshape(B, 2, H, 2, W, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B * 4, H, W, 3))


def tile(views: np.ndarray) -> np.ndarray:
    """The inverse of ``untile``: uint8 [B * 4, H, W, 3] -> [B, 2H, 2W, 3]."""
    n, H, W = views.shape[:3]
    return np.ascontiguousarray(views.reshape(n // 4, 2, 2, H, W, 3).transpose(0, 1, 3, 2, 4, 5).reshape(n // 4, 2 * H, 2 * W, 3))
