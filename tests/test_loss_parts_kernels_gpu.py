"""-m gpu: gn_mse_loss_parts (csrc/loss_weight.hip) against tests/loss_parts_ref.py, on the byte-grid inputs of tests/sphere_loss_ref.py (their
marked share is asserted real: neither empty nor full).

Exact: the marked area A (an integer count over F^2, F a power of two here), the latent pixels P and the sample counts.

S and G, derived bound.  Every term is >= 0.  One term s_p e_p (or (1 - s_p) e_p) carries C - 1 roundings of the channel sum (the squares of
f32 differences are exact in f64), one of n / F^2, one of 1 - s, one of the product: C + 2.  Summing the h w terms of a sample in ANY order
adds at most h w - 1, adding the sample into its row one per sample the row receives (``adds``).  So with ops = (C + 2) + (h w - 1) + adds and
u = 2^-53 the kernel is within ops u / (1 - ops u) of the exact value, relatively, and so is the numpy reference in its own order: the two
differ by at most 2 ops u / (1 - ops u) |ref|.  With N = h w C terms, ops <= 2 N in every case below (asserted), so the bar is at most
4 N 2^-53 -- the multiple is 4, from the count above, not tuned.

The f32 loss of gn_mse_loss on the same inputs: (pixels C + 8) 2^-24 relative, that kernel's own bound in tests/test_sphere_loss_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from genima_amd import _lib
from genima_amd import train_ops as T
import loss_parts_ref as P
import sphere_loss_ref as R

pytestmark = pytest.mark.gpu

C = 4
U = P.U
# name: (B, h, w, F, ld_target, buckets, n_buckets, mask kind)
CASES = {
    "odd-5x7-F8": (3, 5, 7, 8, 8, [2, 0, 2], 3, "grid"),            # odd sizes, lane tails, a repeated bucket
    "odd-5x7-F8-ldt4": (3, 5, 7, 8, 4, [2, 0, 2], 3, "grid"),
    "33x33-F2": (2, 33, 33, 2, 8, [1, 0], 2, "grid"),                # 1089 pixels: five ranges of 256 per sample, the last with 65
    "F1": (2, 16, 24, 1, 8, [0, 0], 1, "grid"),
    "F16": (1, 2, 3, 16, 8, [1], 2, "grid"),
    "no-mask": (3, 5, 7, 8, 8, [2, 0, 2], 3, None),
    "all-marked": (3, 5, 7, 8, 8, [2, 0, 2], 3, "ones"),
    "empty-mask": (3, 5, 7, 8, 8, [2, 0, 2], 3, "zeros"),
    "bucket-out-of-range": (3, 5, 7, 8, 8, [3, -1, 1], 3, "grid"),  # 3 == n_buckets and -1 both land in the extra row
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint64)


def _inputs(name):
    B, h, w, F, ldt, buckets, nb, kind = CASES[name]
    rng = np.random.default_rng(17)
    pred = rng.standard_normal((B, h, w, 8)).astype(np.float16)
    target = np.ascontiguousarray(rng.standard_normal((B, h, w, 8)).astype(np.float16)[..., :ldt])  # junk in the padded channels
    mask = None
    if kind is not None:
        tg, cond = R.byte_grid_pair(B, h * F, w * F, seed=3)
        mask = R.change_mask(tg, cond, 127.5, 127.5, 255.0, 0.0, 30)
        share = R.marked_share(mask)
        assert 0.01 <= share <= 0.5, share
        if kind == "ones":
            mask[..., 0] = 1.0
        elif kind == "zeros":
            mask[..., 0] = 0.0
    return pred, target, mask, np.array(buckets, np.int32), nb


def _run(E, pred, target, mask, bucket, table):
    B, h, w, ldp = pred.shape
    ws = torch.empty(int(E.lib.gn_mse_loss_parts_workspace_bytes(B, h, w)) // 8, dtype=torch.float64, device="cuda")
    H, W, ld_m = mask.shape[1:] if mask is not None else (0, 0, 0)
    _lib.check(E.lib.gn_mse_loss_parts(E._ctx, pred.data_ptr(), target.data_ptr(), mask.data_ptr() if mask is not None else None, bucket.data_ptr(),
                                       table.data_ptr(), ws.data_ptr(), B, h, w, C, ldp, target.shape[-1], H, W, ld_m, table.shape[0] - 1), "gn_mse_loss_parts")
    return table


@pytest.mark.parametrize("name", list(CASES))
def test_parts_against_the_reference(engine, name):
    B, h, w, F, ldt, buckets, nb, kind = CASES[name]
    pred, target, mask, bucket, nb = _inputs(name)
    ref = P.table_add(np.zeros((nb + 1, 5)), pred, target, mask, bucket, C)
    p, t, m, bk = _dev(pred), _dev(target), (_dev(mask) if mask is not None else None), _dev(bucket)
    got_t = _run(engine, p, t, m, bk, torch.zeros((nb + 1, 5), dtype=torch.float64, device="cuda"))
    got = got_t.cpu().numpy()
    adds = [sum(1 for k in buckets if (k if 0 <= k < nb else nb) == row) for row in range(nb + 1)]
    assert got[:, 4].tolist() == [float(a) for a in adds] and got[:, 3].tolist() == [float(a * h * w) for a in adds]
    P.assert_table_close(got, ref, h, w, adds)
    if kind == "ones":
        assert (got[:, 1] == 0.0).all() and np.array_equal(got[:, 2], got[:, 3]) and got[:, 0].sum() > 0.0
    elif kind in ("zeros", None):
        assert (got[:, 0] == 0.0).all() and (got[:, 2] == 0.0).all() and got[:, 1].sum() > 0.0
    else:
        assert 0.0 < got[:, 2].sum() < got[:, 3].sum() and got[:, 0].sum() > 0.0 and got[:, 1].sum() > 0.0
    # two runs, the same bits; the wrapper is the same call
    again = _run(engine, p, t, m, bk, torch.zeros((nb + 1, 5), dtype=torch.float64, device="cuda"))
    assert np.array_equal(_bits(again), _bits(got_t))
    wrapped = T.mse_loss_parts(engine, p, t, m, bk, torch.zeros((nb + 1, 5), dtype=torch.float64, device="cuda"), C)
    assert np.array_equal(_bits(wrapped), _bits(got_t))
    # every row together is gn_mse_loss's mean, within that kernel's f32 summation bound (the f64 side's own error, 4 N u, is far below it)
    pixels = B * h * w
    loss32, _ = T.mse_loss(engine, p.view(pixels, 8), t.view(pixels, ldt), C)
    loss_parts = float((got[:, 0].sum() + got[:, 1].sum()) / (C * got[:, 3].sum()))
    print(f"{name}: parts loss {loss_parts!r}, gn_mse_loss {float(loss32.item())!r}, bar {(pixels * C + 8) * 2.0 ** -24 * loss_parts:.3e}")
    assert abs(float(loss32.item()) - loss_parts) <= ((pixels * C + 8) * 2.0 ** -24 + 4 * h * w * C * U) * loss_parts


def test_a_second_call_accumulates(engine):
    pred, target, mask, bucket, nb = _inputs("odd-5x7-F8")
    pred2 = np.ascontiguousarray(pred[::-1])
    ref = P.table_add(np.zeros((nb + 1, 5)), pred, target, mask, bucket, C)
    ref = P.table_add(ref, pred2, target, mask, [1, 1, 5], C)
    table = torch.zeros((nb + 1, 5), dtype=torch.float64, device="cuda")
    _run(engine, _dev(pred), _dev(target), _dev(mask), _dev(bucket), table)
    first = table.clone()
    _run(engine, _dev(pred2), _dev(target), _dev(mask), _dev(np.array([1, 1, 5], np.int32)), table)
    got = table.cpu().numpy()
    assert got[:, 4].tolist() == [1.0, 2.0, 2.0, 1.0] and bool((table[:, 4] >= first[:, 4]).all())
    P.assert_table_close(got, ref, 5, 7, [1, 2, 2, 1])
    assert np.array_equal(_bits(table[0]), _bits(first[0]))  # a row no sample of the second call names keeps its bits


def test_refusals_write_nothing(engine):
    E, lib = engine, engine.lib
    pred, target, mask, bucket, nb = _inputs("odd-5x7-F8")
    p, t, m, bk = _dev(pred), _dev(target), _dev(mask), _dev(bucket)
    table = torch.full((nb + 2, 5), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((64,), -2.0, dtype=torch.float64, device="cuda")
    good = dict(pred=p.data_ptr(), target=t.data_ptr(), mask=m.data_ptr(), bucket=bk.data_ptr(), table=table.data_ptr(), ws=ws.data_ptr(), B=3, h=5, w=7, C=C,
                ldp=8, ldt=8, H=40, W=56, ld_m=8, nb=nb)
    bad_args = [dict(pred=None), dict(target=None), dict(bucket=None), dict(table=None), dict(ws=None), dict(B=0), dict(h=0), dict(w=-1), dict(C=0),
                dict(ldp=0), dict(ldt=-8), dict(ldp=3), dict(ldt=3), dict(nb=0), dict(nb=-1), dict(table=table.data_ptr() + 4), dict(H=41), dict(W=57),
                dict(H=80), dict(W=112), dict(H=5 * 17, W=7 * 17), dict(H=0), dict(W=0), dict(ld_m=0)]
    for bad in bad_args:
        a = dict(good, **bad)
        assert lib.gn_mse_loss_parts(E._ctx, *a.values()) != 0, bad
        assert b"gn_mse_loss_parts" in lib.gn_last_error(), bad
    torch.cuda.synchronize()
    assert bool((table == 7.0).all()) and bool((ws == -2.0).all())
    # ... and the same arguments unbroken are taken (H, W, ld_m are not looked at without a mask)
    fresh = torch.zeros((2, nb + 1, 5), dtype=torch.float64, device="cuda")
    assert lib.gn_mse_loss_parts(E._ctx, *dict(good, table=fresh[0].data_ptr()).values()) == 0
    assert lib.gn_mse_loss_parts(E._ctx, *dict(good, mask=None, H=0, W=0, ld_m=0, table=fresh[1].data_ptr()).values()) == 0
    torch.cuda.synchronize()
    assert fresh[:, :, 4].sum().item() == 6.0 and bool((table == 7.0).all())
