"""-m "not gpu": the loss read-outs (ControlNetTrainer.attach_frozen(loss_parts=), eval_loss, train_loop.loss_validator; gn_mse_loss_parts in
csrc/loss_weight.hip) without a device: the entry points are declared, bound and exported; the numpy restatement the GPU tests compare
against has the properties the split rests on; the pure summariser; the trainer's refusals before it touches a device; the validator's
default timestep grid against the sampler's own."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from genima_amd import _lib, build, scheduler, train_loop
from genima_amd import train_ops as T
from genima_amd.pix2pix import InstructPix2PixTrainer
from genima_amd.training import ControlNetTrainer
import loss_parts_ref as P
import sphere_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gn_mse_loss_parts", "gn_mse_loss_parts_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert hasattr(lib, n), n
    assert len(_lib.SIGNATURES["gn_mse_loss_parts"][1]) == 17
    assert len(_lib.SIGNATURES["gn_mse_loss_parts_workspace_bytes"][1]) == 3
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["loss_weight.hip"]
    # the workspace query touches no device: three f64 partials per range of 256 latent pixels and sample
    fn = lib.gn_mse_loss_parts_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int32] * 3
    assert fn(3, 5, 7) == 3 * 1 * 24 and fn(2, 33, 33) == 2 * 5 * 24 and fn(8, 64, 64) == 8 * 16 * 24 and fn(0, 4, 4) == 0


def _case(B=3, h=5, w=7, F=8, seed=2):
    target, cond = R.byte_grid_pair(B, h * F, w * F, seed=3)
    mask = R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30)
    assert 0.01 <= R.marked_share(mask) <= 0.5
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, h, w, 8)).astype(np.float16), rng.standard_normal((B, h, w, 8)).astype(np.float16), mask


def test_reference_parts_add_up():
    pred, tgt, mask = _case()
    S, G, A, Pn = P.sample_parts(pred, tgt, mask, 4)
    total = P.total_sq_error(pred, tgt, 4)
    assert (S > 0).all() and (G > 0).all() and (A > 0).all() and (A < Pn).all()
    assert abs(float(S.sum() + G.sum()) - total) <= 1e-12 * total
    assert float(A.sum()) == float((mask[..., 0] != 0).sum()) / 64.0  # the marked area is an integer count over F^2: exact
    # all marked: nothing is background, exactly; empty (and no mask at all): nothing is sphere
    S1, G1, A1, P1 = P.sample_parts(pred, tgt, np.ones_like(mask), 4)
    assert (G1 == 0.0).all() and (A1 == P1).all() and abs(float(S1.sum()) - total) <= 1e-12 * total
    for empty in (np.zeros_like(mask), None):
        S0, G0, A0, _ = P.sample_parts(pred, tgt, empty, 4)
        assert (S0 == 0.0).all() and (A0 == 0.0).all() and abs(float(G0.sum()) - total) <= 1e-12 * total
    # rows: a repeated bucket adds, an out-of-range bucket lands in the extra row
    tab = P.table_add(np.zeros((4, 5)), pred, tgt, mask, [2, 0, 7], 4)
    assert tab[:, 4].tolist() == [1.0, 0.0, 1.0, 1.0] and tab[:, 3].tolist() == [35.0, 0.0, 35.0, 35.0]
    assert tab[3, 0] == S[2] and tab[2, 1] == G[0]


def test_summarize_parts_on_a_hand_written_table():
    #               S     G     A     P    n
    tab = np.array([[2.0, 6.0, 4.0, 20.0, 2.0],    # t 0 .. 499
                    [0.0, 8.0, 0.0, 10.0, 1.0],    # t 500 .. 999: nothing marked -> no sphere loss
                    [5.0, 5.0, 5.0, 10.0, 1.0]])   # the extra row: one dropped sample, in none of the sums
    s = T.summarize_parts(tab, 2, [0, 500, 1000])
    assert s["n"] == 3 and s["dropped"] == 1
    assert s["loss"] == 16.0 / (2 * 30.0) and s["loss_sphere"] == 2.0 / (2 * 4.0) and s["loss_background"] == 14.0 / (2 * 26.0)
    assert s["sphere_area"] == 4.0 / 30.0
    a, b = s["by_t"]
    assert (a["t_lo"], a["t_hi"], a["n"]) == (0, 499, 2) and (b["t_lo"], b["t_hi"], b["n"]) == (500, 999, 1)
    assert a["loss"] == 8.0 / 40.0 and a["loss_sphere"] == 2.0 / 8.0 and a["loss_background"] == 6.0 / 32.0
    assert b["loss"] == 8.0 / 20.0 and b["loss_sphere"] is None and b["loss_background"] == 8.0 / 20.0
    # single timesteps name the rows with ``t``; an all-marked row has no background; an empty table has no loss at all: None, never 0
    full = np.array([[3.0, 0.0, 10.0, 10.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    s = T.summarize_parts(full, 1, [999, 199])
    assert [r["t"] for r in s["by_t"]] == [999, 199] and "t_lo" not in s["by_t"][0]
    assert s["by_t"][0]["loss_background"] is None and s["by_t"][0]["loss_sphere"] == 0.3 and s["loss_background"] is None
    assert s["by_t"][1] == dict(t=199, n=0, loss=None, loss_sphere=None, loss_background=None)
    z = T.summarize_parts(np.zeros((3, 5)), 4, [0, 500, 1000])
    assert z["n"] == 0 and z["dropped"] == 0 and z["loss"] is None and z["loss_sphere"] is None and z["loss_background"] is None and z["sphere_area"] is None
    with pytest.raises(ValueError):
        T.summarize_parts(tab, 2, [0, 250, 500, 1000])  # two rows take two timesteps or three bounds
    with pytest.raises(ValueError):
        T.summarize_parts(np.zeros((3, 4)), 2, [0, 500, 1000])


class _Sched:
    config = {"prediction_type": "epsilon", "num_train_timesteps": 1000}


@pytest.mark.parametrize("value", [-1, 2.5, float("nan"), "4", None, True])
def test_attach_frozen_refuses_a_bad_bucket_count(value):
    tr = ControlNetTrainer.__new__(ControlNetTrainer)  # attach_frozen checks its arguments before it touches the device
    tr._use_graph = False
    with pytest.raises(ValueError):
        tr.attach_frozen(None, None, None, None, _Sched(), loss_parts=value)


def test_attach_frozen_refuses_the_replayed_step_and_other_trainers_and_keeps_the_defaults():
    tr = ControlNetTrainer.__new__(ControlNetTrainer)
    tr._use_graph = True
    with pytest.raises(ValueError, match="eager-only"):
        tr.attach_frozen(None, None, None, None, _Sched(), loss_parts=4)
    p2p = InstructPix2PixTrainer.__new__(InstructPix2PixTrainer)
    p2p._use_graph = False
    with pytest.raises(ValueError, match="ControlNet trainers only"):
        p2p.attach_frozen(None, None, None, None, _Sched(), loss_parts=4)
    with pytest.raises(ValueError, match="ControlNet trainers only"):
        p2p.eval_loss({}, [999])
    with pytest.raises(ValueError, match="eager-only"):
        tr.eval_loss({}, [999])
    with pytest.raises(ValueError, match="eager-only"):
        tr.step(*([None] * 7), loss_parts=(None, None))
    assert inspect.signature(ControlNetTrainer.attach_frozen).parameters["loss_parts"].default == 0
    assert inspect.signature(ControlNetTrainer.step).parameters["loss_parts"].default is None
    assert inspect.signature(ControlNetTrainer.forward_backward).parameters["loss_parts"].default is None
    assert inspect.signature(ControlNetTrainer.loss_parts_summary).parameters["reset"].default is True
    assert inspect.signature(train_loop.TrainLoop.__init__).parameters["loss_parts_steps"].default is None


def test_the_table_is_refused_with_the_option_off():
    tr = ControlNetTrainer.__new__(ControlNetTrainer)
    tr.loss_parts = 0
    with pytest.raises(ValueError, match="loss_parts"):
        tr.loss_parts_summary()
    with pytest.raises(ValueError, match="loss_parts"):
        tr._loss_parts_table()


def test_default_grid_is_the_samplers_five_trailing_steps():
    s = scheduler.EulerAncestralDiscreteScheduler()
    s.set_timesteps(5)
    assert tuple(int(t) for t in s.timesteps) == train_loop.LOSS_VALIDATOR_TIMESTEPS
    assert inspect.signature(train_loop.loss_validator).parameters["timesteps"].default == train_loop.LOSS_VALIDATOR_TIMESTEPS
