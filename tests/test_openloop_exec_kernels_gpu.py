"""-m gpu: ``gn_openloop_exec_actions`` / ``gn_openloop_exec_metrics`` through the eager engine.

The bar of the first is bit equality with the ensemble kernel: ``Engine.action_ensemble`` driven per episode as a rollout would drive it -- a
reset at the episode's start, steps advancing by h, the f16 chunk of the transition at each call's step -- returns, row by row, the bits the
replay kernel writes for the whole table in one launch.  Beside that the f64 rule (tests/openloop_exec_ref.py) within 1e-5 * max|chunk|, the
bound tests/test_ensemble_gpu.py derives for this arithmetic (derived there, not measured).

Shapes: T = 5, A = 3, ld = 8 with the pad columns at 1e30 (inf once it is f16); three episodes of 1, 4 and 11 transitions, N = 16; h in
{1, 2, 3, 5} (h = 3: K = 2 with T no multiple of h), temporal_agg off and on, m in {0, 0.01, 1}; one case at T = 20, A = 8, h = 7."""
import numpy as np
import pytest
import torch

import openloop_exec_ref as XR
from genima_amd._lib import GenimaHipError

pytestmark = pytest.mark.gpu

REL_BOUND = 1e-5
LENGTHS = (1, 4, 11)


def _table(T, A, ld, seed):
    """-> (chunks f16 [N, T, ld] on the host, first_tr int32 [N])."""
    first = XR.first_transitions(LENGTHS)
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(len(first), T, ld, generator=g) * 4.0 - 2.0
    c[..., A:] = 1e30
    return c.half(), first


def _sequential(E, chunks, first, A, h, agg, m):
    """The ensemble kernel as a rollout calls it -> f32 [N, A], the action executed at every transition."""
    N, T, _ = chunks.shape
    K = -(-T // h) if agg else 1
    dev = chunks.cuda()
    want = np.zeros((N, A), np.float32)
    for f, L in zip(np.unique(first), LENGTHS):
        state = E.action_ensemble_state(1, T, A, K)
        for t in range(0, L, h):
            out = E.action_ensemble(dev[f + t: f + t + 1], state, torch.tensor([t], dtype=torch.int32).cuda(),
                                    torch.tensor([1 if t == 0 else 0], dtype=torch.uint8).cuda(), h, K, m, A=A).cpu().numpy()
            n = min(h, L - t)
            want[f + t: f + t + n] = out[0, :n]
    return want


def _replay(E, chunks, first, A, h, agg, m, **kw):
    n_calls = torch.full((len(first),), -1, dtype=torch.int32, device="cuda")
    out = E.openloop_exec_actions(chunks.cuda(), torch.from_numpy(first).cuda(), h, agg, m, A=A, n_calls=n_calls, **kw)
    return out.cpu().numpy(), n_calls.cpu().numpy()


def _check(E, T, A, ld, h, agg, m, seed):
    chunks, first = _table(T, A, ld, seed)
    got, calls = _replay(E, chunks, first, A, h, agg, m)
    assert got.shape == (len(first), A) and got.dtype == np.float32 and np.isfinite(got).all(), "a pad column was read"
    want = _sequential(E, chunks, first, A, h, agg, m)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "the replay differs from the ensemble kernel called step by step"
    ref, ref_calls = XR.exec_actions(chunks.numpy(), first, A, h, agg, m)
    scale = float(np.abs(chunks.numpy()[..., :A].astype(np.float64)).max())
    err = float(np.abs(got.astype(np.float64) - ref).max()) / scale
    print(f"exec_actions T={T} A={A} h={h} agg={agg} m={m}: |out - f64 rule| / max|chunk| = {err:.3e} (bound {REL_BOUND:.0e})")
    assert err <= REL_BOUND
    assert np.array_equal(calls, ref_calls)
    if not agg:
        assert (calls == 1).all()
    again, calls2 = _replay(E, chunks, first, A, h, agg, m)
    assert np.array_equal(again.view(np.int32), got.view(np.int32)) and np.array_equal(calls2, calls), "a second run gives other bits"
    return chunks, first, got


@pytest.mark.parametrize("m", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("agg", [False, True])
@pytest.mark.parametrize("h", [1, 2, 3, 5])
def test_replay_equals_the_ensemble_kernel_bit_for_bit(engine, h, agg, m):
    _check(engine, 5, 3, 8, h, agg, m, seed=100 + h)


def test_replay_at_the_controllers_shape(engine):
    _check(engine, 20, 8, 8, 7, True, 0.01, seed=7)


def test_n_calls_is_optional(engine):
    chunks, first = _table(5, 3, 8, seed=1)
    out = engine.openloop_exec_actions(chunks.cuda(), torch.from_numpy(first).cuda(), 2, True, 0.01, A=3)
    want, _ = _replay(engine, chunks, first, 3, 2, True, 0.01)
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("scaled", [False, True])
def test_metrics_against_the_f64_rule(engine, scaled):
    A = 3
    chunks, first = _table(5, A, 8, seed=11)
    ex, _ = _replay(engine, chunks, first, A, 2, True, 0.01)
    g = torch.Generator().manual_seed(12)
    demo = (torch.rand(len(first), A, generator=g) * 4.0 - 2.0)
    demo[:, A - 1] = (torch.rand(len(first), generator=g) > 0.5).float()
    scale = torch.tensor([0.25, 3.0]) if scaled else None
    dev = dict(first_tr=torch.from_numpy(first).cuda(), joint_scale=None if scale is None else scale.cuda())
    got = engine.openloop_exec_metrics(torch.from_numpy(ex).cuda(), demo.cuda(), dev["first_tr"], joint_scale=dev["joint_scale"]).cpu().numpy()
    want, bound = XR.exec_metrics(ex, demo.numpy(), first, None if scale is None else scale.numpy())
    assert got.shape == (len(first), 4) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    for col in (0, 2, 3):
        ratio = float((err[:, col] / np.maximum(bound[:, col], 1e-300)).max())
        print(f"exec_metrics column {col} scaled={scaled}: max error {err[:, col].max():.3e}, max error / bound {ratio:.3f}")
        assert (err[:, col] <= bound[:, col]).all()
    assert np.array_equal(got[:, 1].astype(np.float64), want[:, 1]) and set(np.unique(got[:, 1])) <= {0.0, 1.0}
    starts = np.unique(first)
    assert (got[starts, 2] == 0).all() and (got[starts, 3] == 0).all(), "no jump at an episode's first step"
    rest = np.setdiff1d(np.arange(len(first)), starts)
    assert (got[rest, 2] > 0).all() and (got[rest, 3] > 0).all()
    again = engine.openloop_exec_metrics(torch.from_numpy(ex).cuda(), demo.cuda(), dev["first_tr"], joint_scale=dev["joint_scale"]).cpu().numpy()
    assert np.array_equal(again.view(np.int32), got.view(np.int32))


def test_refusals(engine):
    """Argument checks only: every call below is refused before a launch, and the outputs stay as they were."""
    T, A, ld = 5, 3, 8
    chunks, first = _table(T, A, ld, seed=2)
    c, f = chunks.cuda(), torch.from_numpy(first).cuda()
    N = len(first)
    out = torch.full((N, A), 7.0, device="cuda")
    ok = dict(h=2, temporal_agg=True, m=0.01, A=A)

    def call(chunks=c, first_tr=f, out=out, **kw):
        a = dict(ok, **kw)
        return engine.openloop_exec_actions(chunks, first_tr, a["h"], a["temporal_agg"], a["m"], A=a["A"], out=out)

    for bad in (dict(h=0), dict(h=T + 1), dict(h=-1), dict(m=-0.5), dict(m=float("nan")), dict(first_tr=None), dict(chunks=c[:, :, :2], A=3), dict(chunks=c[:, :, :2].contiguous(), A=3),
                dict(A=1, out=torch.zeros((N, 1), device="cuda")), dict(A=ld + 1, out=torch.zeros((N, ld + 1), device="cuda")),
                dict(chunks=c[:0], first_tr=f[:0], out=out[:0]), dict(chunks=c[:, :0], out=out), dict(chunks=c.float()), dict(out=out.double())):
        with pytest.raises(GenimaHipError):
            call(**bad)
    assert (out == 7.0).all(), "a refused call wrote something"
    assert engine.lib.gn_openloop_exec_actions(engine._ctx, None, f.data_ptr(), out.data_ptr(), None, N, T, A, ld, 2, 1, 0.01) != 0
    assert engine.lib.gn_openloop_exec_actions(engine._ctx, c.data_ptr(), f.data_ptr(), None, None, N, T, A, ld, 2, 1, 0.01) != 0
    assert engine.lib.gn_openloop_exec_actions(engine._ctx, c.data_ptr(), f.data_ptr(), out.data_ptr(), None, N, T, A, A - 1, 2, 1, 0.01) != 0
    assert engine.lib.gn_openloop_exec_actions(engine._ctx, c.data_ptr(), f.data_ptr(), out.data_ptr(), None, N, 0, A, ld, 2, 1, 0.01) != 0
    assert engine.lib.gn_openloop_exec_actions(engine._ctx, c.data_ptr(), f.data_ptr(), out.data_ptr(), None, 0, T, A, ld, 2, 1, 0.01) != 0
    assert (out == 7.0).all()
    # the metrics entry point
    ex, demo = torch.zeros((N, A), device="cuda"), torch.zeros((N, A), device="cuda")
    res = torch.full((N, 4), 7.0, device="cuda")
    for bad in (dict(exec_actions=ex[:, :1], demo=demo[:, :1].contiguous()), dict(demo=None), dict(first_tr=None), dict(demo=demo[:, :2].contiguous()),
                dict(joint_scale=torch.ones(A, device="cuda")), dict(exec_actions=ex[:0], demo=demo[:0], first_tr=f[:0], out=res[:0])):
        a = dict(dict(exec_actions=ex, demo=demo, first_tr=f, out=res, joint_scale=None), **bad)
        with pytest.raises(GenimaHipError):
            engine.openloop_exec_metrics(a["exec_actions"].contiguous(), a["demo"], a["first_tr"], a["out"], joint_scale=a["joint_scale"])
    lib = engine.lib
    assert lib.gn_openloop_exec_metrics(engine._ctx, ex.data_ptr(), None, f.data_ptr(), None, res.data_ptr(), N, A) != 0
    assert lib.gn_openloop_exec_metrics(engine._ctx, ex.data_ptr(), demo.data_ptr(), f.data_ptr(), None, res.data_ptr(), N, 1) != 0
    assert lib.gn_openloop_exec_metrics(engine._ctx, ex.data_ptr(), demo.data_ptr(), f.data_ptr(), None, res.data_ptr(), 0, A) != 0
    assert (res == 7.0).all()


def test_record_mode_raises():
    from genima_amd.engine import Engine

    R = Engine("cuda", record=True)
    chunks, first = _table(5, 3, 8, seed=3)
    x = torch.zeros((len(first), 3), device="cuda")
    with pytest.raises(RuntimeError, match="eager"):
        R.openloop_exec_actions(chunks.cuda(), torch.from_numpy(first).cuda(), 2, True, 0.01, A=3)
    with pytest.raises(RuntimeError, match="eager"):
        R.openloop_exec_metrics(x, x, torch.from_numpy(first).cuda())
    assert R.num_ops == 0


def test_a_damaged_first_tr_is_refused_with_a_host_copy_and_clamped_without(engine):
    """Entries above n and below 0: with the host copy the wrapper refuses; without it the kernel clamps the entry into [0, n], so the row reads
    inside the table and every other row is what it was."""
    T, A, ld, h = 5, 3, 8, 2
    chunks, first = _table(T, A, ld, seed=4)
    good, good_calls = _replay(engine, chunks, first, A, h, True, 0.01)
    bad = first.copy()
    bad[6], bad[9] = 12, -3  # transition 6: above n; transition 9: negative
    for which in (6, 9):
        one = first.copy()
        one[which] = bad[which]
        with pytest.raises(GenimaHipError, match=r"first_tr\[%d\]" % which):
            _replay(engine, chunks, one, A, h, True, 0.01, first_tr_host=one)
    _replay(engine, chunks, first, A, h, True, 0.01, first_tr_host=first)  # a sound table passes the check
    got, calls = _replay(engine, chunks, bad, A, h, True, 0.01)
    untouched = np.setdiff1d(np.arange(len(first)), [6, 9])
    assert np.array_equal(got[untouched].view(np.int32), good[untouched].view(np.int32)) and np.array_equal(calls[untouched], good_calls[untouched])
    clamped = first.copy()
    clamped[6], clamped[9] = 6, 0
    want, want_calls = XR.exec_actions(chunks.numpy(), clamped, A, h, True, 0.01)
    scale = float(np.abs(chunks.numpy()[..., :A].astype(np.float64)).max())
    assert np.isfinite(got).all() and np.abs(got.astype(np.float64) - want).max() <= REL_BOUND * scale and np.array_equal(calls, want_calls)
    assert np.array_equal(got[6], chunks.numpy()[6, 0, :A].astype(np.float32)), "clamped to n: the row's own chunk, step 0"
    # the metrics kernel: an entry above n reads as an episode's first step (no row n - 1 is needed); the other rows are what they were
    demo = torch.rand(len(first), A, generator=torch.Generator().manual_seed(5))
    ex = torch.from_numpy(good).cuda()
    with pytest.raises(GenimaHipError, match=r"first_tr\[6\]"):
        engine.openloop_exec_metrics(ex, demo.cuda(), torch.from_numpy(bad).cuda(), first_tr_host=bad)
    sound = engine.openloop_exec_metrics(ex, demo.cuda(), torch.from_numpy(first).cuda(), first_tr_host=first).cpu().numpy()
    hurt = engine.openloop_exec_metrics(ex, demo.cuda(), torch.from_numpy(bad).cuda()).cpu().numpy()
    keep = np.setdiff1d(np.arange(len(first)), [6])
    assert np.array_equal(hurt[keep].view(np.int32), sound[keep].view(np.int32)) and hurt[6, 2] == 0 and hurt[6, 3] == 0
    assert np.array_equal(hurt[6, :2], sound[6, :2])
