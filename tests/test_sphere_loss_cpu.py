"""-m "not gpu": the sphere-weighted loss (ControlNetTrainer.attach_frozen(sphere_loss_weight=), csrc/loss_weight.hip) without a device: the
three entry points are declared, bound and built without fma contraction; the numpy restatement the GPU tests compare against has the
properties the design rests on; the trainer refuses bad values before it touches a device."""
import os
import re

import numpy as np
import pytest

from genima_amd import _lib, build
from genima_amd.training import ControlNetTrainer
import sphere_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gn_change_mask", "gn_loss_weight_pool", "gn_mse_loss_weighted")


def test_entry_points_are_declared_bound_and_built_without_contraction():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", header), n
    assert len(_lib.SIGNATURES["gn_change_mask"][1]) == 14
    assert len(_lib.SIGNATURES["gn_loss_weight_pool"][1]) == 12
    assert len(_lib.SIGNATURES["gn_mse_loss_weighted"][1]) == 13
    assert "loss_weight.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["loss_weight.hip"]


@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 8, 24), (1, 32, 32)])
def test_byte_grid_inputs_mark_a_real_share(shape):
    """The GPU tests' byte-grid inputs: neither an empty nor a full mask, and untouched pixels come back as their own bytes (d == 0)."""
    target, cond = R.byte_grid_pair(*shape, seed=3)
    share = R.marked_share(R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30))
    assert 0.01 <= share <= 0.5, share
    assert R.marked_share(R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 765)) == 0.0
    same = R.image_bytes(target[..., :3], 127.5, 127.5) == R.image_bytes(cond[..., :3], 255.0, 0.0)
    assert 0.5 <= same.all(axis=-1).mean() < 1.0


def test_threshold_is_strict():
    """d == threshold is unmarked, d == threshold + 1 is marked; ties round to even; the clamp holds at both ends."""
    cond = np.zeros((1, 1, 4, 8), np.float16)
    target = np.zeros((1, 1, 4, 8), np.float16)
    for x, (r, g, b) in enumerate([(10, 10, 10), (10, 10, 11), (0, 0, 30), (31, 0, 0)]):
        target[0, 0, x, :3] = (np.array([r, g, b]) / 127.5 - 1.0).astype(np.float16)
    cond[..., :3] = 0.0
    m = R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30)
    assert m[0, 0, :, 0].tolist() == [0.0, 1.0, 0.0, 1.0] and not m[..., 1:].any()
    ties = np.array([0.0, 1.0, 2.0, 3.0, 127.0, 128.0, 400.0, -7.0], np.float16)
    assert R.image_bytes(ties, 1.0, 0.5).tolist() == [0.0, 2.0, 2.0, 4.0, 128.0, 128.0, 255.0, 0.0]


def test_lambda_zero_is_the_plain_mean():
    target, cond = R.byte_grid_pair(2, 16, 16, seed=3)
    mask = R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30)
    weight, count, wsum = R.loss_weight_pool(mask, 2, 2, 0.0)
    assert (weight == 1.0).all() and wsum == 2 * 2 * 2 and count == int((mask[..., 0] != 0).sum()) > 0
    w4, c4, s4 = R.loss_weight_pool(mask, 2, 2, 4.0)
    assert c4 == count and abs(float(w4.astype(np.float64).sum()) - s4) <= 1e-6 * s4 and w4.max() > 1.0


def test_all_marked_mask_gives_the_unweighted_mean():
    rng = np.random.default_rng(0)
    pred, tgt = rng.standard_normal((70, 8)).astype(np.float16), rng.standard_normal((70, 4)).astype(np.float16)
    ones, lam = np.ones((1, 56, 80, 8), np.float16), 4.0
    weight, count, wsum = R.loss_weight_pool(ones, 7, 10, lam)
    assert (weight == 1.0 + lam).all() and count == 56 * 80 and wsum == 70 * (1.0 + lam)
    loss_w, dp_w = R.mse_loss_weighted(pred, tgt, weight.reshape(-1), wsum, 4, 8.0)
    loss_1, dp_1 = R.mse_loss_weighted(pred, tgt, np.ones(70, np.float32), np.float64(70), 4, 8.0)
    d = pred[:, :4].astype(np.float64) - tgt.astype(np.float64)
    assert abs(loss_1 - float((d * d).mean())) <= 1e-12
    assert abs(loss_w - loss_1) <= 1e-12 * loss_1 and np.allclose(dp_w, dp_1, rtol=1e-12, atol=0) and not dp_w[:, 4:].any()
    assert R.gs_f32(np.float64(70), 4, 8.0) == np.float32(np.float32(16.0) / np.float32(280.0))


class _Sched:
    config = {"prediction_type": "epsilon", "num_train_timesteps": 1000}


@pytest.mark.parametrize("kw", [dict(sphere_loss_weight=-1.0), dict(sphere_loss_weight=float("nan")), dict(sphere_change_threshold=-1),
                                dict(sphere_loss_weight=1.0, sphere_change_threshold=-3)])
def test_attach_frozen_refuses_negative_values(kw):
    tr = ControlNetTrainer.__new__(ControlNetTrainer)  # attach_frozen checks its arguments before it touches the device
    tr._use_graph = False
    with pytest.raises(ValueError):
        tr.attach_frozen(None, None, None, None, _Sched(), **kw)


def test_attach_frozen_refuses_the_replayed_step_and_keeps_the_default():
    tr = ControlNetTrainer.__new__(ControlNetTrainer)
    tr._use_graph = True
    with pytest.raises(ValueError):
        tr.attach_frozen(None, None, None, None, _Sched(), sphere_loss_weight=4.0)
    import inspect
    p = inspect.signature(ControlNetTrainer.attach_frozen).parameters
    assert p["sphere_loss_weight"].default == 0.0 and p["sphere_change_threshold"].default == 30
    assert inspect.signature(ControlNetTrainer.step).parameters["loss_weight"].default is None
    assert inspect.signature(ControlNetTrainer.forward_backward).parameters["loss_weight"].default is None
