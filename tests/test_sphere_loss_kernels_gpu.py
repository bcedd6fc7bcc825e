"""-m gpu: gn_change_mask, gn_loss_weight_pool and gn_mse_loss_weighted (csrc/loss_weight.hip) against tests/sphere_loss_ref.py.

The mask, the pooled weight, the marked count and wsum are compared BIT for bit (the rules are stated one rounded operation at a time and the
file is built without fma contraction; the count is an integer sum).  The weighted loss is compared with f64 from the same f16 inputs:
  dpred   |dev - ref| <= |ref| (2^-11 + 6 * 2^-24) + 2^-25: room for five f32 roundings and one to spare (the kernel makes four: (float)(C wsum),
          the division, gs * w, pred - target; the last product is exact and rounded once to f16, as gn_mse_loss's compiled code does), the f16
          rounding of the result, and half an f16 subnormal step as the floor;
  loss    |dev - ref| <= (pixels * C + 8) 2^-24 ref: the worst case of summing pixels * C non-negative f32 terms in any order, plus the
          roundings of a term and of the final quotient.
Every test asserts that its byte-grid input marks between 1 % and 50 % of the pixels, so none passes on an empty or a full mask."""
import numpy as np
import pytest
import torch

from genima_amd import _lib
from genima_amd import train_ops as T
import sphere_loss_ref as R

pytestmark = pytest.mark.gpu

SCALES = (127.5, 127.5, 255.0, 0.0)  # the trainer's: target in [-1, 1], conditioning image in [0, 1]
THR = 30


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().numpy()
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _np_bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _grid_mask(shape, seed=3):
    """Byte-grid inputs of ``shape`` and their reference mask at the trainer's scales, with the share every test must see."""
    target, cond = R.byte_grid_pair(*shape, seed=seed)
    mask = R.change_mask(target, cond, *SCALES, THR)
    share = R.marked_share(mask)
    assert 0.01 <= share <= 0.5, share
    return target, cond, mask


def _run_mask(E, target, cond, scales, thr):
    B, H, W, ld_t = target.shape
    mask = torch.full((B, H, W, 8), 7.0, dtype=torch.float16, device="cuda")
    _lib.check(E.lib.gn_change_mask(E._ctx, target.data_ptr(), cond.data_ptr(), mask.data_ptr(), B, H, W, ld_t, cond.shape[-1], *scales, thr), "gn_change_mask")
    return mask


@pytest.mark.parametrize("ld_c", [8, 3])
@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 8, 24)])
def test_change_mask_bit_equal(engine, shape, ld_c):
    target, cond, ref = _grid_mask(shape)
    got = _run_mask(engine, _dev(target), _dev(cond[..., :ld_c]), SCALES, THR)
    assert np.array_equal(_bits(got), _np_bits(ref))
    assert not _bits(got)[..., 1:].any()
    assert torch.equal(T.change_mask(engine, _dev(target), _dev(cond), THR), got)  # the wrapper's defaults are the trainer's scales
    # off the byte grid: .5 ties of both parities, values beyond 255 and below 0, junk in channels 3..7
    t2, c2 = R.off_grid_pair(*shape)
    scales2 = (2.0, 0.5, 1.0, 0.5)
    ref2 = R.change_mask(t2, c2, *scales2, THR)
    assert 0.0 < R.marked_share(ref2) < 1.0
    got2 = _run_mask(engine, _dev(t2), _dev(c2[..., :ld_c]), scales2, THR)
    assert np.array_equal(_bits(got2), _np_bits(ref2))


def _run_pool(E, mask, h, w, lam):
    B, H, W, ld = mask.shape
    weight = torch.full((B, h, w), -1.0, dtype=torch.float32, device="cuda")
    count = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")  # the entry point zeroes the word itself
    wsum = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    _lib.check(E.lib.gn_loss_weight_pool(E._ctx, mask.data_ptr(), ld, weight.data_ptr(), count.data_ptr(), wsum.data_ptr(), B, H, W, h, w, lam), "gn_loss_weight_pool")
    return weight, count, wsum


@pytest.mark.parametrize("lam", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("shape,hw", [((2, 16, 16), (2, 2)), ((1, 8, 24), (1, 3)), ((2, 16, 16), (16, 16)), ((1, 32, 32), (2, 2))])
def test_loss_weight_pool_bit_equal(engine, shape, hw, lam):
    _, _, mask = _grid_mask(shape)
    w_ref, c_ref, s_ref = R.loss_weight_pool(mask, hw[0], hw[1], lam)
    m = _dev(mask)
    weight, count, wsum = _run_pool(engine, m, hw[0], hw[1], lam)
    assert np.array_equal(_bits(weight), _np_bits(w_ref))
    assert int(count.item()) == c_ref > 0
    assert _bits(wsum)[0] == _np_bits(np.array([s_ref], np.float64))[0]
    again = _run_pool(engine, m, hw[0], hw[1], lam)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((weight, count, wsum), again))
    wt, ct, st = T.loss_weight_pool(engine, m, hw[0], hw[1], lam)
    assert torch.equal(wt, weight) and torch.equal(ct, count) and torch.equal(st, wsum)


def _loss_case(pixels, seed=5):
    """pred [pixels, 8] / target [pixels, 8] f16 with junk in the padded channels, and the reference weights of a byte-grid mask."""
    shape, hw = {70: ((1, 14, 20), (7, 10)), 2 * 192 * 192: ((2, 192, 192), (192, 192))}[pixels]
    _, _, mask = _grid_mask(shape)
    weight, _, wsum = R.loss_weight_pool(mask, hw[0], hw[1], 4.0)
    assert weight.size == pixels and weight.max() > 1.0
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((pixels, 8)).astype(np.float16)
    target = rng.standard_normal((pixels, 8)).astype(np.float16)
    return pred, target, weight.reshape(-1), wsum


def _run_loss(E, pred, target, weight, wsum, C, grad_scale):
    dpred = torch.full_like(pred, 9.0)
    loss = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(1024, dtype=torch.float32, device="cuda")
    _lib.check(E.lib.gn_mse_loss_weighted(E._ctx, pred.data_ptr(), target.data_ptr(), weight.data_ptr(), wsum.data_ptr(), dpred.data_ptr(), loss.data_ptr(),
                                          ws.data_ptr(), pred.shape[0], C, pred.shape[1], target.shape[1], grad_scale), "gn_mse_loss_weighted")
    return loss, dpred


def _assert_loss_close(loss, dpred, loss_ref, dp_ref, pixels, C):
    got = dpred.cpu().numpy().astype(np.float64)
    err, bar = np.abs(got - dp_ref), np.abs(dp_ref) * (2.0 ** -11 + 6 * 2.0 ** -24) + 2.0 ** -25
    print(f"pixels {pixels}: dpred worst err / bar {float((err / bar).max()):.3f}, max |dpred| {float(np.abs(got).max()):.4g}; "
          f"loss {float(loss.item()):.8f} ref {loss_ref:.8f} bar {(pixels * C + 8) * 2.0 ** -24 * loss_ref:.3e}")
    assert np.isfinite(got).all() and (err <= bar).all(), float((err / bar).max())
    assert not _bits(dpred)[:, C:].any()
    assert abs(float(loss.item()) - loss_ref) <= (pixels * C + 8) * 2.0 ** -24 * loss_ref


@pytest.mark.parametrize("ld_t", [4, 8])
@pytest.mark.parametrize("pixels", [70, 2 * 192 * 192])
def test_mse_loss_weighted_against_f64(engine, pixels, ld_t):
    C, gscale = 4, 1024.0
    pred, target, weight, wsum = _loss_case(pixels)
    target = np.ascontiguousarray(target[:, :ld_t])
    loss_ref, dp_ref = R.mse_loss_weighted(pred, target, weight, wsum, C, gscale)
    assert np.abs(dp_ref).max() < 6.0e4 and np.abs(dp_ref).max() > 2.0 ** -14  # clear of f16 overflow, not all subnormal
    p, t, w = _dev(pred), _dev(target), _dev(weight)
    loss, dpred = _run_loss(engine, p, t, w, _dev(np.array([wsum], np.float64)), C, gscale)
    _assert_loss_close(loss, dpred, loss_ref, dp_ref, pixels, C)
    if ld_t == 8:  # the wrapper the trainer calls
        l2, d2 = T.mse_loss_weighted(engine, p, t, w, _dev(np.array([wsum], np.float64)), C, grad_scale=gscale)
        assert torch.equal(l2, loss) and torch.equal(d2, dpred)


@pytest.mark.parametrize("pixels,shape,hw", [(70, (1, 14, 20), (7, 10)), (2 * 192 * 192, (2, 192, 192), (192, 192))])
def test_empty_mask_is_gn_mse_loss(engine, pixels, shape, hw):
    """A mask of zeros pooled with lambda = 4 gives weight 1 and wsum = pixels: the same gs formula times 1.0f, so gn_mse_loss's dpred bits."""
    C, gscale = 4, 1024.0
    pred, target, _, _ = _loss_case(pixels)
    weight, count, wsum = _run_pool(engine, torch.zeros(shape + (8,), dtype=torch.float16, device="cuda"), hw[0], hw[1], 4.0)
    assert int(count.item()) == 0 and float(wsum.item()) == float(pixels) and bool((weight == 1.0).all())
    p, t = _dev(pred), _dev(target)
    loss, dpred = _run_loss(engine, p, t, weight.reshape(-1), wsum, C, gscale)
    loss0, dpred0 = T.mse_loss(engine, p, t, C, grad_scale=gscale)
    assert np.array_equal(_bits(dpred), _bits(dpred0))
    loss_ref, dp_ref = R.mse_loss_weighted(pred, target, np.ones(pixels, np.float32), np.float64(pixels), C, gscale)
    _assert_loss_close(loss, dpred, loss_ref, dp_ref, pixels, C)
    assert abs(float(loss0.item()) - loss_ref) <= (pixels * C + 8) * 2.0 ** -24 * loss_ref


def test_refusals_write_nothing(engine):
    E, lib = engine, engine.lib
    target, cond, mask_ref = _grid_mask((2, 16, 16))
    t, c, m = _dev(target), _dev(cond), _dev(mask_ref)
    inf, nan = float("inf"), float("nan")

    out_mask = torch.full((2, 16, 16, 8), 7.0, dtype=torch.float16, device="cuda")
    good = dict(target=t.data_ptr(), cond=c.data_ptr(), mask=out_mask.data_ptr(), B=2, H=16, W=16, ld_t=8, ld_c=8, t_mul=127.5, t_add=127.5, c_mul=255.0,
                c_add=0.0, threshold=THR)
    bad_mask = [dict(target=None), dict(cond=None), dict(mask=None), dict(B=0), dict(H=0), dict(W=-1), dict(ld_t=2), dict(ld_c=2), dict(threshold=-1),
                dict(t_mul=inf), dict(t_add=nan), dict(c_mul=-inf), dict(c_add=nan)]
    for bad in bad_mask:
        a = dict(good, **bad)
        assert lib.gn_change_mask(E._ctx, *a.values()) != 0, bad
        assert b"gn_change_mask" in lib.gn_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out_mask == 7.0).all())

    weight = torch.full((2, 2, 2), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((2,), 99, dtype=torch.int64, device="cuda")
    ws8 = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    good = dict(mask=m.data_ptr(), ld_m=8, weight=weight.data_ptr(), count=cnt.data_ptr(), wsum=ws8.data_ptr(), B=2, H=16, W=16, h=2, w=2, lam=4.0)
    bad_pool = [dict(lam=-1.0), dict(lam=nan), dict(h=3), dict(w=3), dict(h=4), dict(H=32, W=32, h=1, w=1), dict(mask=None), dict(weight=None), dict(count=None),
                dict(wsum=None), dict(wsum=ws8.data_ptr() + 4), dict(count=cnt.data_ptr() + 4), dict(B=0), dict(h=0)]
    for bad in bad_pool:
        a = dict(good, **bad)
        assert lib.gn_loss_weight_pool(E._ctx, *a.values()) != 0, bad
        assert b"gn_loss_weight_pool" in lib.gn_last_error(), bad
    torch.cuda.synchronize()
    assert bool((weight == -1.0).all()) and bool((cnt == 99).all()) and bool((ws8 == -1.0).all())

    pred, tgt, w70, wsum = _loss_case(70)
    p, g, w = _dev(pred), _dev(tgt), _dev(w70)
    s = torch.tensor([float(wsum), 0.0], dtype=torch.float64, device="cuda")
    dpred, loss, wsp = torch.full_like(p, 9.0), torch.full((1,), -1.0, dtype=torch.float32, device="cuda"), torch.full((1024,), -2.0, dtype=torch.float32, device="cuda")
    good = dict(pred=p.data_ptr(), target=g.data_ptr(), weight=w.data_ptr(), wsum=s.data_ptr(), dpred=dpred.data_ptr(), loss=loss.data_ptr(), ws=wsp.data_ptr(),
                pixels=70, C=4, ldp=8, ldt=8, gscale=1024.0)
    bad_loss = [dict(pred=None), dict(target=None), dict(weight=None), dict(wsum=None), dict(loss=None), dict(ws=None), dict(pixels=0), dict(C=0), dict(ldp=3),
                dict(ldt=3), dict(wsum=s.data_ptr() + 4)]
    for bad in bad_loss:
        a = dict(good, **bad)
        assert lib.gn_mse_loss_weighted(E._ctx, *a.values()) != 0, bad
        assert b"gn_mse_loss_weighted" in lib.gn_last_error(), bad
    torch.cuda.synchronize()
    assert bool((dpred == 9.0).all()) and float(loss.item()) == -1.0 and bool((wsp == -2.0).all())
