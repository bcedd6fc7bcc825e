"""-m gpu: ``gn_openloop_image_metrics`` bit for bit against the int64 restatement (tests/openloop_ref.py; the sums are integers, so there is
no tolerance) and ``gn_openloop_action_metrics`` against the f64 restatement within the derived rounding bound, flags exactly.

Shapes: tiled B = 2, V = 4, 40 x 36 (360 four-pixel threads: the second block of 256 is partial); per-view B = 2, V = 3, 17 x 23 (W * 3 = 69
is no multiple of 4: rows start off the dword grid, and W % 4 = 3 leaves a row tail); 160 x 160 of maximal difference, the smallest square at
which a 32-bit sum wraps; actions B = 3, T = 5, A = 8 at pitch 16 with a sample stride longer than T * 16."""
import ctypes as C

import numpy as np
import pytest
import torch

import openloop_ref as OR

pytestmark = pytest.mark.gpu

MARK = -0x0123456789ABCDEF


def _images(B, V, H, W, seed, tiled):
    rng = np.random.RandomState(seed)
    gen = rng.randint(0, 256, (B, 2 * H, 2 * W, 3) if tiled else (B, V, H, W, 3)).astype(np.uint8)
    gt = rng.randint(0, 256, (B * V, H, W, 3)).astype(np.uint8)
    occ = (rng.randint(0, 3, (B * V, H, W)) == 0).astype(np.uint8) * rng.randint(1, 256, (B * V, H, W)).astype(np.uint8)  # any non-zero byte counts
    occ[1], occ[2] = 0, 1  # one view with nothing occupied, one with everything
    return gen, gt, occ


def _ref(gen, gt, occ, B, V, H, W, tiled):
    views = OR.untile(gen) if tiled else gen
    return OR.image_metrics(views, gt.reshape(B, V, H, W, 3), occ.reshape(B, V, H, W))


def _run_images(engine, gen, gt, occ, rows, **kw):
    out = torch.full((rows, 4 if gen.ndim == 4 else gen.shape[1], 5), MARK, dtype=torch.int64, device="cuda")
    engine.openloop_image_metrics(torch.from_numpy(gen).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(occ).cuda(), out, **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("B,V,H,W,tiled", [(2, 4, 40, 36, True), (2, 3, 17, 23, False)])
def test_image_metrics_equal_the_int64_reference(engine, B, V, H, W, tiled):
    gen, gt, occ = _images(B, V, H, W, 11, tiled)
    want = _ref(gen, gt, occ, B, V, H, W, tiled)
    assert want[0, 1, 1] == 0 and want[0, 2, 3] == 0 and (want[1, :, 1] > 0).all() and (want[1, :, 3] > 0).all()
    got = _run_images(engine, gen, gt, occ, B)
    assert np.array_equal(got, want)
    assert np.array_equal(_run_images(engine, gen, gt, occ, B), got)  # a second run: the same bits
    # rows addressed by row0, n_valid: only sample 0 is scored, into row 3; everything else keeps the marker
    part = _run_images(engine, gen, gt, occ, 6, row0=3, n_valid=1)
    assert np.array_equal(part[3], want[0]) and (np.delete(part, 3, axis=0) == MARK).all()
    assert (_run_images(engine, gen, gt, occ, 2, row0=1, n_valid=0) == MARK).all()


def test_image_sums_are_64_bit(engine):
    H = W = 160
    gen, gt, occ = np.full((1, 1, H, W, 3), 255, np.uint8), np.zeros((1, H, W, 3), np.uint8), np.ones((1, H, W), np.uint8)
    got = _run_images(engine, gen, gt, occ, 1)
    assert got[0, 0].tolist() == [4993920000, 25600, 0, 0, 25600 * 3 * ((255 * 255) & 255)] and 4993920000 > 2 ** 32


def _actions(seed=5, B=3, T=5, A=8, ld=16, extra=7):
    rng = np.random.RandomState(seed)
    buf = rng.randn(B, T * ld + extra).astype(np.float16)
    a_hat = np.lib.stride_tricks.as_strided(buf, (B, T, ld), (buf.strides[0], ld * 2, 2))
    actions = rng.randn(B, T, A).astype(np.float32)
    actions[..., A - 1] = rng.randint(0, 2, (B, T))
    a_hat[0, 0, A - 1], a_hat[0, 1, A - 1] = 0.0, 0.0  # a logit of exactly 0 counts as closed: right for label 0, wrong for label 1
    actions[0, 0, A - 1], actions[0, 1, A - 1] = 0.0, 1.0
    return buf, a_hat[..., :A].copy(), actions, rng.uniform(0.05, 2.0, A - 1).astype(np.float32)


@pytest.mark.parametrize("scaled", [False, True])
def test_action_metrics_within_the_derived_bound(engine, scaled):
    B, T, A, ld = 3, 5, 8, 16
    buf, a_hat, actions, scale = _actions()
    dbuf = torch.from_numpy(buf).cuda()
    view = dbuf.as_strided((B, T, A), (buf.shape[1], ld, 1))
    assert view.stride(0) > T * ld
    out = torch.full((B + 2, T, 2), -7.0, dtype=torch.float32, device="cuda")
    kw = dict(joint_scale=torch.from_numpy(scale).cuda()) if scaled else {}
    engine.openloop_action_metrics(view, torch.from_numpy(actions).cuda(), out, row0=1, **kw)
    got = out.cpu().numpy().astype(np.float64)
    total, flag, bound = OR.action_metrics(a_hat, actions, scale if scaled else None)
    assert (got[0] == -7.0).all() and (got[B + 1] == -7.0).all()
    assert np.array_equal(got[1:B + 1, :, 1], flag) and flag[0, 0] == 1.0 and flag[0, 1] == 0.0 and 0 < flag.mean() < 1
    err = np.abs(got[1:B + 1, :, 0] - total)
    print(f"openloop action sums (scaled={scaled}): max error {err.max():.3e}, max error / bound {(err / bound).max():.3f}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all()
    again = torch.full_like(out, -7.0)
    engine.openloop_action_metrics(view, torch.from_numpy(actions).cuda(), again, row0=1, **kw)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))
    part = torch.full_like(out, -7.0)
    engine.openloop_action_metrics(view, torch.from_numpy(actions).cuda(), part, row0=3, n_valid=1, **kw)
    assert torch.equal(part[3].view(torch.int32), out[1].view(torch.int32)) and bool((part[:3] == -7.0).all()) and bool((part[4:] == -7.0).all())


def test_refused_arguments_leave_the_outputs_untouched(engine):
    from genima_amd._lib import GenimaHipError

    lib, ctx = engine.lib, engine._ctx
    B, V, H, W = 2, 4, 8, 8
    gen, gt, occ = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (B * V * H * W * 3, B * V * H * W * 3, B * V * H * W))
    out = torch.full((B, V, 5), MARK, dtype=torch.int64, device="cuda")
    g, t, o, r = gen.data_ptr(), gt.data_ptr(), occ.data_ptr(), out.data_ptr()
    ok = dict(gen=g, gt=t, occ=o, out=r, B=B, V=V, H=H, W=W, tiled=1, row0=0, n_valid=B, rows=B)
    bad = [dict(gen=None), dict(gt=None), dict(occ=None), dict(out=None), dict(B=0), dict(V=0), dict(H=0), dict(W=-1), dict(n_valid=-1), dict(n_valid=B + 1),
           dict(row0=-1), dict(row0=1), dict(V=3), dict(tiled=1, V=5)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.gn_openloop_image_metrics(ctx, a["gen"], a["gt"], a["occ"], a["out"], a["B"], a["V"], a["H"], a["W"], a["tiled"], a["row0"], a["n_valid"], a["rows"])
        assert rc != 0, change
    torch.cuda.synchronize()
    assert bool((out == MARK).all())
    T, A = 5, 8
    a_hat, act = torch.zeros((B, T, A), dtype=torch.float16, device="cuda"), torch.zeros((B, T, A), dtype=torch.float32, device="cuda")
    aout = torch.full((B, T, 2), -7.0, dtype=torch.float32, device="cuda")
    ok = dict(a=a_hat.data_ptr(), ld=A, bs=T * A, act=act.data_ptr(), out=aout.data_ptr(), B=B, T=T, A=A, row0=0, n_valid=B, rows=B)
    for change in [dict(a=None), dict(act=None), dict(out=None), dict(B=0), dict(T=0), dict(A=1), dict(n_valid=-1), dict(n_valid=B + 1), dict(row0=-1), dict(row0=1),
                   dict(ld=A - 1), dict(bs=T * A - A)]:
        a = dict(ok, **change)
        rc = lib.gn_openloop_action_metrics(ctx, a["a"], a["ld"], a["bs"], a["act"], None, a["out"], a["B"], a["T"], a["A"], a["row0"], a["n_valid"], a["rows"])
        assert rc != 0, change
    torch.cuda.synchronize()
    assert bool((aout == -7.0).all())
    # the wrappers are eager only
    from genima_amd.engine import Engine

    rec = Engine("cuda:0", record=True)
    with pytest.raises(RuntimeError, match="eager"):
        rec.openloop_image_metrics(gen.view(B, 2 * H, 2 * W, 3), gt.view(B * V, H, W, 3), occ.view(B * V, H, W), out)
    with pytest.raises(RuntimeError, match="eager"):
        rec.openloop_action_metrics(a_hat, act, aout)
    assert issubclass(GenimaHipError, RuntimeError)
