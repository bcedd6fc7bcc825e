"""numpy restatement of csrc/loss_weight.hip (gn_change_mask, gn_loss_weight_pool, gn_mse_loss_weighted) in the operation order
include/genima_hip.h states: every product and sum of the f32 rules is its own np.float32 operation, ``rintf`` is ``np.rint``.  Shared by
test_sphere_loss_cpu.py and the two test_sphere_loss_*_gpu.py files, together with the inputs they agree on."""
import numpy as np

F32 = np.float32


def image_bytes(x16: np.ndarray, mul: float, add: float) -> np.ndarray:
    """clamp(rintf(x * mul + add), 0, 255) in f32 (fmaxf / fminf: a NaN gives 0)."""
    with np.errstate(all="ignore"):
        v = np.rint((x16.astype(F32) * F32(mul)).astype(F32) + F32(add)).astype(F32)
        return np.fmin(np.fmax(v, F32(0)), F32(255))


def change_mask(target16: np.ndarray, cond16: np.ndarray, t_mul, t_add, c_mul, c_add, threshold: int) -> np.ndarray:
    """target16 / cond16: f16 [B, H, W, >= 3] -> f16 [B, H, W, 8], channel 0 = (sum_c |tb_c - cb_c| > threshold)."""
    tb, cb = image_bytes(target16[..., :3], t_mul, t_add), image_bytes(cond16[..., :3], c_mul, c_add)
    d = np.zeros(tb.shape[:-1], F32)
    for c in range(3):
        d = (d + np.abs((tb[..., c] - cb[..., c]).astype(F32))).astype(F32)
    out = np.zeros(d.shape + (8,), np.float16)
    out[..., 0] = (d > F32(threshold)).astype(np.float16)
    return out


def loss_weight_pool(mask16: np.ndarray, h: int, w: int, lam: float):
    """mask16 f16 [B, H, W, ld] -> (weight f32 [B, h, w], count_total int, wsum np.float64)."""
    B, H, W = mask16.shape[:3]
    F = H // h
    assert H == F * h and W == F * w and 1 <= F <= 16
    n = (mask16[..., 0] != 0).reshape(B, h, F, w, F).sum(axis=(2, 4)).astype(np.int64)
    lam = F32(lam)
    weight = (F32(1.0) + (lam * (n.astype(F32) / F32(F * F)).astype(F32)).astype(F32)).astype(F32)
    count = int(n.sum())
    wsum = np.float64(B * h * w) + np.float64(lam) * np.float64(count) / np.float64(F * F)
    return weight, count, wsum


def mse_loss_weighted(pred16: np.ndarray, target16: np.ndarray, weight: np.ndarray, wsum, C: int, grad_scale: float):
    """f64 from the same f16 inputs, the f32 weights and the f64 wsum: pred16 [pixels, ldp], target16 [pixels, ldt], weight [pixels]
    -> (loss, dpred [pixels, ldp] with zeros in the padded channels), both np.float64."""
    d = pred16[:, :C].astype(np.float64) - target16[:, :C].astype(np.float64)
    wt = weight.reshape(-1, 1).astype(np.float64)
    den = np.float64(C) * np.float64(wsum)
    dpred = np.zeros(pred16.shape, np.float64)
    dpred[:, :C] = (np.float64(grad_scale) * 2.0 / den) * wt * d
    return float((wt * d * d).sum() / den), dpred


def gs_f32(wsum, C: int, grad_scale: float) -> np.float32:
    """The kernel's gradient scale: __fdiv_rn(grad_scale * 2.0f, (float)((double)C * wsum))."""
    return F32(F32(F32(grad_scale) * F32(2.0)) / F32(np.float64(C) * np.float64(wsum)))


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------------------
def byte_grid_pair(B: int, H: int, W: int, seed: int = 0):
    """-> (target f16 [B, H, W, 8] in [-1, 1], cond f16 [B, H, W, 8] in [0, 1]) made from bytes: cond = random bytes / 255, target = the same
    bytes with one rectangle and one disc per image overwritten by a flat colour, / 127.5 - 1.  Channels 3..7 are zero."""
    rng = np.random.default_rng(seed)
    cb = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.int64)
    tb = cb.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        y0, x0 = int(rng.integers(0, H - H // 4)), int(rng.integers(0, W - W // 3))
        tb[b, y0:y0 + max(2, H // 4), x0:x0 + max(2, W // 3)] = rng.integers(0, 256, size=3)
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), max(2.0, min(H, W) / 5.0)
        tb[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(0, 256, size=3)
    target, cond = np.zeros((B, H, W, 8), np.float16), np.zeros((B, H, W, 8), np.float16)
    target[..., :3] = (tb / 127.5 - 1.0).astype(np.float16)
    cond[..., :3] = (cb / 255.0).astype(np.float16)
    return target, cond


def off_grid_pair(B: int, H: int, W: int, seed: int = 1):
    """Arbitrary f16 values off the byte grid, for the scales (2, 0.5) / (1, 0.5): every integer-valued entry scales to a .5 tie (both
    parities), others land beyond 255 or below 0, the rest are plain fractions; cond is twice the target plus a few levels of noise, so the
    summed difference falls on both sides of a threshold of 30.  -> (target, cond) f16 [B, H, W, 8], channels 3..7 junk."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, size=(B, H, W, 8))
    v = np.where(kind == 0, rng.integers(-3, 140, size=kind.shape).astype(np.float64),   # ties: 2 v + 0.5 in the target, an integer + 0.5 in cond
                 np.where(kind == 1, rng.uniform(100.0, 4000.0, size=kind.shape),         # mostly beyond 255
                          np.where(kind == 2, rng.uniform(-4000.0, -0.25, size=kind.shape),  # below 0
                                   rng.uniform(0.0, 130.0, size=kind.shape))))
    target = v.astype(np.float16)
    noise = rng.integers(-30, 31, size=kind.shape) + rng.choice([0.0, 0.0, 0.25, 0.5], size=kind.shape)
    cond = (2.0 * target.astype(np.float64) + noise).astype(np.float16)
    return target, cond


def marked_share(mask16: np.ndarray) -> float:
    return float((mask16[..., 0] != 0).mean())
