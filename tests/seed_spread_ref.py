"""The rules of ``gn_openloop_seed_spheres`` / ``gn_openloop_seed_actions`` (include/genima_hip.h states them) and the arithmetic of
``OpenLoopResult.seed_summary`` in plain numpy, for tests/test_seed_spread_cpu.py, tests/test_seed_spread_kernels_gpu.py and
tests/test_openloop_seeds_gpu.py.

Every restatement walks the seeds in the kernels' order, r = 0 .. R - 1, one numpy operation per kernel operation, so in the kernels' own
precision (f64 for the spheres, ``dtype=np.float32`` for the actions) it rounds where they round.

The bounds.  u is the unit roundoff of the working precision (2^-53, 2^-24).  Every bound has the form ``(R + A + 8) u M`` (A = 0 for the
spheres), M the summed magnitudes of what went into the column:

* a seed mean is R - 1 additions and one division or multiplication: R roundings of the mean magnitude;
* a sum over the A - 1 joints adds A - 2 more, the scale and the subtraction two more: column 0 and 3 of the action kernel make at most
  R + A + 3 roundings of ``sum_j s_j (mean_r |a_rj| + |d_j|)``;
* a deviation ``x_r - mean`` carries the mean's R roundings and its own: (R + 1) of ``|x_r| + |mean|``.  Summing R of them, dividing and (for
  the actions) scaling and adding the joints comes to at most 2 R + A + 3 roundings; M takes a factor 2 instead, so that
  (R + A + 8) 2 >= 2 R + A + 3;
* a SQUARED deviation doubles the relative error of the difference, 2 (R + 2) roundings of ``(|x_r| + |mean|)^2``, plus the R + 2 of the sum
  and the division: 3 R + 6.  M takes a factor 4 -- (R + 8) 4 >= 3 R + 6 -- and is written with all three magnitudes, the seed's, the
  mean's and the truth's, so that one M serves the spread, the squared shift and the squared bias."""
import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24


def _found(gen_m, gt_m, min_ratio):
    return (gen_m > 0) & (gt_m > 0) & (gen_m >= min_ratio * gt_m)


def seed_spheres(sph, min_ratio=0.5):
    """``sph`` integer [R, N, V, S, 17] -> ``(out f64 [N, V, S, 8], bound f64 [N, V, S, 8])``; the bound of column 0 is 0 (a count)."""
    t = np.asarray(sph).astype(np.float64)
    R = t.shape[0]
    gt_m = t[0, ..., 5]
    one = np.ones_like(gt_m)
    safe_gt = np.where(gt_m > 0, gt_m, one)
    tx, ty = t[0, ..., 6] / safe_gt, t[0, ..., 7] / safe_gt

    def seed(r):
        gen_m = t[r, ..., 1]
        ok = _found(gen_m, gt_m, min_ratio)
        g = np.where(ok, gen_m, one)
        return ok, t[r, ..., 2] / g, t[r, ..., 3] / g, g / safe_gt

    k, sx, sy, sq = (np.zeros_like(gt_m) for _ in range(4))
    ax_, ay_, aq_ = (np.zeros_like(gt_m) for _ in range(3))  # the summed magnitudes
    for r in range(R):
        ok, cx, cy, q = seed(r)
        k += ok
        sx, sy, sq = np.where(ok, sx + cx, sx), np.where(ok, sy + cy, sy), np.where(ok, sq + q, sq)
        ax_, ay_, aq_ = ax_ + ok * np.abs(cx), ay_ + ok * np.abs(cy), aq_ + ok * np.abs(q)
    kd = np.where(k > 0, k, one)
    mx, my, mq = sx / kd, sy / kd, sq / kd
    spread, shift, qvar, worst, m_sq, m_q, m_worst = (np.zeros_like(gt_m) for _ in range(7))
    for r in range(R):
        ok, cx, cy, q = seed(r)
        ax, ay, bx, by, dq = cx - mx, cy - my, cx - tx, cy - ty, q - mq
        d2 = bx * bx + by * by
        spread = np.where(ok, spread + (ax * ax + ay * ay), spread)
        shift = np.where(ok, shift + d2, shift)
        qvar = np.where(ok, qvar + dq * dq, qvar)
        worst = np.where(ok & (d2 > worst), d2, worst)
        term = (np.abs(cx) + np.abs(mx) + np.abs(tx)) ** 2 + (np.abs(cy) + np.abs(my) + np.abs(ty)) ** 2
        m_sq, m_q, m_worst = m_sq + ok * term, m_q + ok * (np.abs(q) + np.abs(mq)) ** 2, np.maximum(m_worst, ok * term)
    out = np.stack([k, mx - tx, my - ty, spread / kd, shift / kd, mq, qvar / kd, worst], axis=-1)
    out[..., 1:] = np.where((k > 0)[..., None], out[..., 1:], np.nan)
    n = (R + 8) * U64
    bound = np.stack([0 * k, n * (ax_ / kd + np.abs(tx)), n * (ay_ / kd + np.abs(ty)), n * 4 * m_sq / kd, n * 4 * m_sq / kd, n * aq_ / kd,
                      n * 4 * m_q / kd, n * 4 * m_worst], axis=-1)
    return out, bound


def action_l1(chunk, demo, scale, dtype=np.float32):
    """``gn_openloop_action_metrics``' column 0 in its own order: ``chunk`` f16 [..., >= A], ``demo`` [..., A] -> [...] in ``dtype``."""
    A = demo.shape[-1]
    total = np.zeros(demo.shape[:-1], dtype)
    for j in range(A - 1):
        d = np.abs(chunk[..., j].astype(dtype) - demo[..., j].astype(dtype))
        total = (total + (dtype(scale[j]) * d if scale is not None else d)).astype(dtype)
    return total


def seed_actions(chunks, demo, scale=None, dtype=np.float32):
    """``chunks`` f16 [R, N, T, >= A], ``demo`` f32 [N, T, A], ``scale`` f32 [A - 1] or None -> ``(out [N, T, 4] in dtype, bound f64
    [N, T, 4])``.  With ``dtype=np.float32`` every operation rounds where the kernel's does; with f64 it is the rule itself.  The bound is
    that of the F32 kernel against the f64 rule; column 1 is a flag (bound 0)."""
    R, A = chunks.shape[0], demo.shape[-1]
    inv = dtype(np.float32(1.0 / R))
    s64 = np.ones(A - 1) if scale is None else np.asarray(scale, np.float64)
    a64, d64 = chunks[..., :A].astype(np.float64), demo.astype(np.float64)
    out = np.zeros(demo.shape[:2] + (4,), dtype)
    err_mean, mad = np.zeros(demo.shape[:2], dtype), np.zeros(demo.shape[:2], dtype)
    for j in range(A - 1):
        s = np.zeros(demo.shape[:2], dtype)
        for r in range(R):
            s = (s + chunks[r, ..., j].astype(dtype)).astype(dtype)
        mean = (s * inv).astype(dtype)
        dev = np.zeros(demo.shape[:2], dtype)
        for r in range(R):
            dev = (dev + np.abs(chunks[r, ..., j].astype(dtype) - mean)).astype(dtype)
        d, m = np.abs(mean - demo[..., j].astype(dtype)), (dev * inv).astype(dtype)
        err_mean = (err_mean + (dtype(scale[j]) * d if scale is not None else d)).astype(dtype)
        mad = (mad + (dtype(scale[j]) * m if scale is not None else m)).astype(dtype)
    grip, errs = np.zeros(demo.shape[:2], dtype), np.zeros(demo.shape[:2], dtype)
    for r in range(R):
        grip = (grip + chunks[r, ..., A - 1].astype(dtype)).astype(dtype)
        errs = (errs + action_l1(chunks[r], demo, scale, dtype)).astype(dtype)
    out[..., 0], out[..., 2], out[..., 3] = err_mean, mad, (errs * inv).astype(dtype)
    out[..., 1] = (((grip * inv).astype(dtype) > 0) == (demo[..., A - 1] > 0.5)).astype(dtype)
    mean_abs = np.abs(a64[..., : A - 1]).mean(axis=0)  # [N, T, A - 1]
    m_err = ((mean_abs + np.abs(d64[..., : A - 1])) * s64).sum(axis=-1)
    m_dev = 2.0 * ((mean_abs + np.abs(a64[..., : A - 1].mean(axis=0))) * s64).sum(axis=-1)
    n = (R + A + 8) * U32
    return out, np.stack([n * m_err, 0 * m_err, n * m_dev, n * m_err], axis=-1)


def across(values):
    """``seed_summary``'s entry for one score: the values, their mean, SAMPLE standard deviation (ddof = 1), min and max."""
    v = np.asarray(values, np.float64)
    mean = v.sum() / len(v)
    return {"values": list(values), "mean": float(mean), "std": float(np.sqrt(((v - mean) ** 2).sum() / (len(v) - 1))) if len(v) > 1 else None,
            "min": float(v.min()), "max": float(v.max())}


def sphere_block(table, R, sel=None):
    """``seed_summary()["spheres"]``' block over the rows of ``table`` f64 [..., 8] with k >= 2 (and ``sel``)."""
    q = table.reshape(-1, 8)
    keep = q[:, 0] >= 2
    if sel is not None:
        keep &= np.asarray(sel).reshape(-1)
    q = q[keep]
    n = len(q)
    if not n:
        return {"n": 0, "found_all_rate": None, "bias_px": None, "spread_px": None, "rms_shift_px": None, "variance_share": None, "mass_ratio_std": None,
                "worst_px": None}
    return {"n": n, "found_all_rate": float((q[:, 0] == R).sum() / n), "bias_px": float(np.sqrt(q[:, 1] ** 2 + q[:, 2] ** 2).sum() / n),
            "spread_px": float(np.sqrt(q[:, 3].sum() / n)), "rms_shift_px": float(np.sqrt(q[:, 4].sum() / n)),
            "variance_share": float(q[:, 3].sum() / q[:, 4].sum()) if q[:, 4].sum() > 0 else None, "mass_ratio_std": float(np.sqrt(q[:, 6].sum() / n)),
            "worst_px": float(np.sqrt(q[:, 7].max()))}


def action_block(table, joints):
    """``seed_summary()["actions"][unit]`` of ``table`` f32 [N, T, 4]."""
    t = table.astype(np.float64).reshape(-1, 4)
    each, mean = t[:, 3].sum() / len(t) / joints, t[:, 0].sum() / len(t) / joints
    return {"mean_of_seeds": float(each), "seed_mean": float(mean), "gain": float(1.0 - mean / each) if each else None,
            "spread": float(t[:, 2].sum() / len(t) / joints), "gripper_acc_seed_mean": float(t[:, 1].sum() / len(t))}
