"""numpy f64 restatement of gn_mse_loss_parts (csrc/loss_weight.hip, include/genima_hip.h): the subtraction pred - target is taken in f32 as
the kernel takes it, everything else is f64 in numpy's own summation order.  Shared by test_loss_parts_cpu.py and the two
test_loss_parts_*_gpu.py files."""
import numpy as np

COLS = 5  # S, G, A, P, n
U = 2.0 ** -53


def sample_parts(pred16: np.ndarray, target16: np.ndarray, mask16, C: int):
    """pred16 [B, h, w, ldp], target16 [B, h, w, ldt] f16, mask16 [B, H, W, ld] f16 (channel 0) or None -> per sample (S, G, A, P), each
    np.float64 [B]: the squared error times the marked share of its latent pixel, times the unmarked share, the marked area in latent
    pixels, the latent pixels."""
    B, h, w = pred16.shape[:3]
    d = (pred16[..., :C].astype(np.float32) - target16[..., :C].astype(np.float32)).astype(np.float32)
    e = (d.astype(np.float64) ** 2).sum(axis=-1)
    if mask16 is None:
        s = np.zeros((B, h, w), np.float64)
    else:
        H, W = mask16.shape[1:3]
        F = H // h
        assert H == F * h and W == F * w and 1 <= F <= 16
        n = (mask16[..., 0] != 0).reshape(B, h, F, w, F).sum(axis=(2, 4)).astype(np.int64)
        s = n.astype(np.float64) / np.float64(F * F)
    S = (s * e).sum(axis=(1, 2))
    G = ((1.0 - s) * e).sum(axis=(1, 2))
    A = s.sum(axis=(1, 2))
    return S, G, A, np.full(B, float(h * w))


def table_add(table: np.ndarray, pred16, target16, mask16, bucket, C: int) -> np.ndarray:
    """``table`` f64 [n_buckets + 1, 5] gains every sample's (S, G, A, P, 1) in row bucket[b]; out-of-range buckets go to the last row."""
    S, G, A, P = sample_parts(pred16, target16, mask16, C)
    nb = table.shape[0] - 1
    for b, k in enumerate(bucket):
        row = int(k) if 0 <= int(k) < nb else nb
        table[row] += (S[b], G[b], A[b], P[b], 1.0)
    return table


def total_sq_error(pred16, target16, C: int) -> float:
    d = (pred16[..., :C].astype(np.float32) - target16[..., :C].astype(np.float32)).astype(np.float32)
    return float((d.astype(np.float64) ** 2).sum())


def assert_table_close(got, ref, h, w, adds_per_row, C=4):
    """``got`` against ``ref`` (both [rows, 5]): A, P, n exactly; S, G within the bound tests/test_loss_parts_kernels_gpu.py derives --
    2 ops u / (1 - ops u) relative, ops = (C + 2) + (h w - 1) + the samples the row received, u = 2^-53."""
    assert np.array_equal(got[:, 2:], ref[:, 2:]), (got[:, 2:], ref[:, 2:])
    N = h * w * C
    for row in range(ref.shape[0]):
        ops = (C + 2) + (h * w - 1) + max(1, adds_per_row[row])
        assert ops <= 2 * N
        for col in (0, 1):
            bar = 2 * ops * U / (1 - ops * U) * abs(ref[row, col])
            err = abs(got[row, col] - ref[row, col])
            print(f"row {row} col {'SG'[col]}: ref {ref[row, col]:.17g} err {err:.3e} bar {bar:.3e}")
            assert err <= bar, (row, col, err, bar)
