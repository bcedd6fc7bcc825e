"""-m gpu: ``gn_openloop_seed_spheres`` / ``gn_openloop_seed_actions`` through the eager engine against the restatements of
tests/seed_spread_ref.py.

The bar is the rounding bound derived there -- (R + A + 8) roundings of the summed magnitudes in the working precision (f64 for the spheres,
f32 for the actions against the f64 rule) -- and the measured worst difference is printed beside it, with whether the bits equal the
restatement that walks the kernel's own order (they do under -ffp-contract=off; DESIGN.md 3.18 says so; the assertion stays the bound).
Column 3 of the action kernel has a stricter bar: bit for bit the f32 seed-order mean of ``gn_openloop_action_metrics``' own column 0 run per
seed on the same chunks.

Shapes.  Spheres: N = 9, V = 4, S = 8 -> 288 rows, more than one 256-thread workgroup; R in {1, 2, 5}; planted rows with k = R, 0 < k < R,
k = 0, gt_m = 0 and a seed exactly at gen_m = min_ratio * gt_m.  Actions: N = 5, T = 20, A = 8, row pitch 8 and 16 with the pad columns at
inf, R in {1, 3}, with and without the joint scale."""
import numpy as np
import pytest
import torch

import seed_spread_ref as SS
from genima_amd._lib import GenimaHipError

pytestmark = pytest.mark.gpu

N, V, S = 9, 4, 8
MIN_RATIO = 0.5


def _sphere_tables(R, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((R, N, V, S, 17), np.int64)
    t[..., 0], t[..., 9:] = 4096, rng.integers(0, 1 << 20, (R, N, V, S, 8))  # columns the kernel never reads
    gt_m = rng.integers(1, 200000, (N, V, S))
    gt_m[rng.random((N, V, S)) < 0.1] = 0
    gen_m = (gt_m[None] * rng.uniform(0.0, 1.6, (R, N, V, S))).astype(np.int64)
    gen_m[rng.random((R, N, V, S)) < 0.1] = 0
    # the planted rows: (n, v, s) = (0, 0, 0) every seed found; (0, 0, 1) seed 0 alone; (0, 0, 2) none; (0, 0, 3) hidden; (8, 3, 7), in
    # the second workgroup, seed 0 exactly at the boundary and the others just below it
    gt_m[0, 0, :4], gt_m[8, 3, 7] = [1000, 1000, 1000, 0], 1000
    gen_m[:, 0, 0, 0], gen_m[:, 0, 0, 1], gen_m[:, 0, 0, 2], gen_m[:, 0, 0, 3] = 900, 0, 499, 700
    gen_m[0, 0, 0, 1] = 800
    gen_m[:, 8, 3, 7] = 499
    gen_m[0, 8, 3, 7] = 500
    t[:, ..., 5] = gt_m
    t[:, ..., 6], t[:, ..., 7] = (gt_m * rng.uniform(0, 255, (N, V, S))).astype(np.int64), (gt_m * rng.uniform(0, 255, (N, V, S))).astype(np.int64)
    t[:, ..., 8] = gt_m * 3000
    t[..., 1] = gen_m
    t[..., 2], t[..., 3] = (gen_m * rng.uniform(0, 255, (R, N, V, S))).astype(np.int64), (gen_m * rng.uniform(0, 255, (R, N, V, S))).astype(np.int64)
    t[..., 4] = gen_m * 3000
    return t


@pytest.mark.parametrize("R", [1, 2, 5])
def test_seed_spheres_against_the_restatement(engine, R):
    t = _sphere_tables(R, seed=40 + R)
    dev = torch.from_numpy(t).cuda()
    got = engine.openloop_seed_spheres(dev, min_ratio=MIN_RATIO).cpu().numpy()
    want, bound = SS.seed_spheres(t, MIN_RATIO)
    assert got.shape == (N, V, S, 8) and got.dtype == np.float64
    k = want[..., 0]
    assert k[0, 0, :4].tolist() == [R, 1, 0, 0] and k[8, 3, 7] == 1, "the planted rows"
    if R > 1:
        assert ((k > 0) & (k < R)).sum() > 4 and (k == R).sum() > 4
    assert np.array_equal(got[..., 0], k)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[k == 0][:, 1:]).all() and np.isfinite(got[k > 0]).all()
    some = k > 0
    err = np.abs(got[some] - want[some])[:, 1:]
    ratio = err / np.maximum(bound[some][:, 1:], 1e-300)
    same = np.array_equal(got[some].view(np.int64), want[some].view(np.int64))
    print(f"seed_spheres R={R}: max |out - restatement| = {err.max():.3e}, max error / bound = {ratio.max():.3e}, bits equal: {same}")
    assert (err <= bound[some][:, 1:]).all()
    if R == 1:
        assert (got[some][:, 3] == 0).all() and (got[some][:, 6] == 0).all()
    again = engine.openloop_seed_spheres(dev, min_ratio=MIN_RATIO).cpu().numpy()
    assert np.array_equal(again.view(np.int64), got.view(np.int64)), "a second run gives other bits"
    # the boundary is the boundary: a hair above min_ratio and the planted seed is not found
    above = engine.openloop_seed_spheres(dev, min_ratio=0.5005).cpu().numpy()
    assert above[8, 3, 7, 0] == 0 and np.array_equal(above[..., 0], SS.seed_spheres(t, 0.5005)[0][..., 0])


def test_seed_spheres_refusals(engine):
    """Argument checks only: every call below is refused before a launch, and out stays as it was; N = 0 is accepted."""
    R = 2
    dev = torch.from_numpy(_sphere_tables(R, seed=1)).cuda()
    out = torch.full((N, V, S, 8), 7.0, dtype=torch.float64, device="cuda")
    for bad in (dict(sph=dev.int()), dict(sph=dev[..., :16].contiguous()), dict(sph=dev[0]), dict(sph=None), dict(out=out.float()), dict(out=out[:-1]),
                dict(min_ratio=-0.5), dict(min_ratio=float("nan")), dict(sph=dev[:, :, :1].contiguous(), out=out[:, :1].contiguous()),
                dict(sph=dev.cpu())):
        a = dict(dict(sph=dev, out=out, min_ratio=MIN_RATIO), **bad)
        with pytest.raises(GenimaHipError):
            engine.openloop_seed_spheres(a["sph"], a["out"], min_ratio=a["min_ratio"])
    lib, ctx, p, o = engine.lib, engine._ctx, dev.data_ptr(), out.data_ptr()
    for args in ((None, o, 0.5, R, N, V, S), (p, None, 0.5, R, N, V, S), (p + 4, o, 0.5, R, N, V, S), (p, o + 4, 0.5, R, N, V, S),
                 (p, o, 0.5, 0, N, V, S), (p, o, 0.5, 65, N, V, S), (p, o, 0.5, R, -1, V, S), (p, o, 0.5, R, N, 1, S), (p, o, 0.5, R, N, 9, S),
                 (p, o, 0.5, R, N, V, 0), (p, o, 0.5, R, N, V, 9), (p, o, -1.0, R, N, V, S), (p, o, float("nan"), R, N, V, S)):
        assert lib.gn_openloop_seed_spheres(ctx, *args) != 0, args
        assert b"gn_openloop_seed_spheres" in lib.gn_last_error()
    assert lib.gn_openloop_seed_spheres(ctx, p, o, 0.5, R, 0, V, S) == 0, "N == 0 is accepted and does nothing"
    engine.synchronize()
    assert (out == 7.0).all(), "a refused call wrote something"


def _chunks(R, T, A, ld, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(R, 5, T, ld, generator=g) * 4.0 - 2.0
    c[..., A:] = 1e30  # inf once it is f16: a pad column that is read shows
    demo = torch.rand(5, T, A, generator=g) * 4.0 - 2.0
    demo[..., A - 1] = (torch.rand(5, T, generator=g) > 0.5).float()
    return c.half(), demo


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("ld", [8, 16])
@pytest.mark.parametrize("R", [1, 3])
def test_seed_actions_against_the_restatement(engine, R, ld, scaled):
    T, A = 20, 8
    chunks, demo = _chunks(R, T, A, ld, seed=R * 100 + ld)
    scale = torch.linspace(0.25, 3.0, A - 1) if scaled else None
    dc, dd, ds = chunks.cuda(), demo.cuda(), None if scale is None else scale.cuda()
    got = engine.openloop_seed_actions(dc, dd, joint_scale=ds).cpu().numpy()
    assert got.shape == (5, T, 4) and got.dtype == np.float32 and np.isfinite(got).all(), "a pad column was read"
    s = None if scale is None else scale.numpy()
    exact, bound = SS.seed_actions(chunks.numpy(), demo.numpy(), s, dtype=np.float64)
    walk, _ = SS.seed_actions(chunks.numpy(), demo.numpy(), s)
    err = np.abs(got.astype(np.float64) - exact)
    for col in (0, 2, 3):
        ratio = float((err[..., col] / np.maximum(bound[..., col], 1e-300)).max())
        print(f"seed_actions R={R} ld={ld} scaled={scaled} column {col}: max error {err[..., col].max():.3e}, max error / bound {ratio:.3f}")
        assert (err[..., col] <= bound[..., col]).all()
    print(f"   bits equal the f32 walk in the kernel's order: {np.array_equal(got.view(np.int32), walk.view(np.int32))}")
    assert np.array_equal(got[..., 1].astype(np.float64), exact[..., 1]) and set(np.unique(got[..., 1])) <= {0.0, 1.0}
    # column 3: the f32 seed-order mean of gn_openloop_action_metrics' own column 0, bit for bit
    total = np.zeros((5, T), np.float32)
    for r in range(R):
        per = torch.zeros((5, T, 2), dtype=torch.float32, device="cuda")
        engine.openloop_action_metrics(dc[r], dd, per, joint_scale=ds)
        total = (total + per.cpu().numpy()[..., 0]).astype(np.float32)
    mean = (total * np.float32(1.0 / R)).astype(np.float32)
    assert np.array_equal(got[..., 3].view(np.int32), mean.view(np.int32)), "column 3 is not the seed-order mean of the action kernel's own sums"
    if R == 1:
        assert np.array_equal(got[..., 0].view(np.int32), got[..., 3].view(np.int32)) and (got[..., 2] == 0).all()
    else:
        assert (got[..., 2] > 0).all()
    again = engine.openloop_seed_actions(dc, dd, joint_scale=ds).cpu().numpy()
    assert np.array_equal(again.view(np.int32), got.view(np.int32)), "a second run gives other bits"


def test_seed_actions_refusals(engine):
    """Argument checks only: every call below is refused before a launch, and out stays as it was."""
    R, T, A, ld, n = 3, 20, 8, 16, 5
    chunks, demo = _chunks(R, T, A, ld, seed=5)
    c, d = chunks.cuda(), demo.cuda()
    out = torch.full((n, T, 4), 7.0, device="cuda")
    for bad in (dict(chunks=c.float()), dict(chunks=c[..., :4].contiguous()), dict(chunks=c[..., :8]), dict(chunks=c[0]), dict(chunks=None), dict(demo=None),
                dict(demo=d[:, :-1].contiguous()), dict(demo=d.double()), dict(out=out.double()), dict(out=out[:-1]), dict(joint_scale=torch.ones(A, device="cuda")),
                dict(chunks=c[:, :0], demo=d[:0], out=out[:0]), dict(chunks=c[:0]), dict(demo=d[..., :1].contiguous())):
        a = dict(dict(chunks=c, demo=d, out=out, joint_scale=None), **bad)
        with pytest.raises(GenimaHipError):
            engine.openloop_seed_actions(a["chunks"], a["demo"], a["out"], joint_scale=a["joint_scale"])
    lib, ctx, pc, pd, po = engine.lib, engine._ctx, c.data_ptr(), d.data_ptr(), out.data_ptr()
    inv = float(np.float32(1.0 / R))
    for args in ((None, ld, pd, None, po, inv, R, n, T, A), (pc, ld, None, None, po, inv, R, n, T, A), (pc, ld, pd, None, None, inv, R, n, T, A),
                 (pc, A - 1, pd, None, po, inv, R, n, T, A), (pc, ld, pd, None, po, inv, R, 0, T, A), (pc, ld, pd, None, po, inv, R, n, 0, A),
                 (pc, ld, pd, None, po, inv, R, n, T, 1), (pc, ld, pd, None, po, 1.0, 0, n, T, A), (pc, ld, pd, None, po, float(np.float32(1.0 / 65)), 65, n, T, A),
                 (pc, ld, pd, None, po, 0.5, R, n, T, A), (pc, ld, pd, None, po, float("nan"), R, n, T, A), (pc + 1, ld, pd, None, po, inv, R, n, T, A),
                 (pc, ld, pd + 2, None, po, inv, R, n, T, A), (pc, ld, pd, pd + 2, po, inv, R, n, T, A), (pc, ld, pd, None, po + 2, inv, R, n, T, A)):
        assert lib.gn_openloop_seed_actions(ctx, *args) != 0, args
        assert b"gn_openloop_seed_actions" in lib.gn_last_error()
    engine.synchronize()
    assert (out == 7.0).all(), "a refused call wrote something"


def test_record_mode_raises():
    from genima_amd.engine import Engine

    rec = Engine("cuda", record=True)
    chunks, demo = _chunks(2, 20, 8, 8, seed=6)
    with pytest.raises(RuntimeError, match="eager"):
        rec.openloop_seed_actions(chunks.cuda(), demo.cuda())
    with pytest.raises(RuntimeError, match="eager"):
        rec.openloop_seed_spheres(torch.zeros((2, 1, 4, 2, 17), dtype=torch.int64, device="cuda"))
    assert rec.num_ops == 0
