"""-m "not gpu": temporal ensembling of action chunks -- known answers worked by hand on the float64 restatement (tests/ensemble_ref.py), the
ABI names (header, loader, library), and the argument checks of the library and of the Python wrappers that need no device."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ensemble_ref import EnsembleRef
from genima_amd import _lib, build, configs
from genima_amd._lib import GenimaHipError
from genima_amd.act import GenimaACT, execution_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_action_ensemble", "gn_action_ensemble_f16", "gn_action_ensemble_state_bytes", "gn_program_add_action_ensemble")


def _const_chunks(n, T):
    """Call c predicts the value 10 c + j for its j-th step: every prediction names who made it and for which offset."""
    return [(10.0 * c + np.arange(T, dtype=np.float64)).reshape(1, T, 1) for c in range(n)]


def test_plain_means_of_overlapping_predictions():
    """T = 4, h = 1, m = 0, five calls at steps 0 .. 4: step t is predicted by the calls max(0, t - 3) .. t, call c at offset t - c."""
    ref = EnsembleRef(B=1, T=4, A=1, K=4, h=1, m=0.0)
    got = [ref(c, [t])[0, 0, 0] for t, c in enumerate(_const_chunks(5, 4))]
    want = [0.0,                                # step 0: call 0 offset 0
            (1 + 10) / 2,                       # step 1: call 0 offset 1, call 1 offset 0
            (2 + 11 + 20) / 3,
            (3 + 12 + 21 + 30) / 4,
            (13 + 22 + 31 + 40) / 4]            # step 4: call 0 no longer covers it
    assert got == pytest.approx(want, rel=0, abs=1e-12)


def test_exponential_weights_favour_the_oldest():
    m = 0.01
    ref = EnsembleRef(B=1, T=4, A=1, K=4, h=1, m=m)
    got = [ref(c, [t])[0, 0, 0] for t, c in enumerate(_const_chunks(3, 4))]
    w = [1.0, math.exp(-0.01), math.exp(-0.02)]
    want = [0.0, (w[0] * 1 + w[1] * 10) / (w[0] + w[1]), (w[0] * 2 + w[1] * 11 + w[2] * 20) / sum(w)]
    assert got == pytest.approx(want, rel=0, abs=1e-12)
    assert got[2] < (2 + 11 + 20) / 3, "the oldest prediction (the smallest value here) weighs most"


def test_whole_chunk_with_one_slot_is_the_identity():
    rng = np.random.default_rng(0)
    ref = EnsembleRef(B=2, T=4, A=3, K=1, h=4)
    for t in (0, 4, 8):
        c = rng.uniform(-2, 2, (2, 4, 5))
        assert np.array_equal(ref(c, [t, t]), c[:, :, :3])


def test_a_reset_forgets_history_of_that_row_only():
    chunks = _const_chunks(3, 4)
    two = [np.concatenate([c, c], axis=0) for c in chunks]
    ref = EnsembleRef(B=2, T=4, A=1, K=4, h=1, m=0.0)
    ref(two[0], [0, 0])
    ref(two[1], [1, 1])
    out = ref(two[2], [2, 2], reset=[False, True])
    assert out[0, 0, 0] == pytest.approx((2 + 11 + 20) / 3) and out[1, 0, 0] == 20.0


def test_uneven_horizon_evicts_and_covers_partly():
    """T = 3, h = 2, K = 2: the call at step 2 finds step 2 covered by both chunks and step 3 by the new one alone; the call at step 4 has
    dropped the first chunk."""
    ref = EnsembleRef(B=1, T=3, A=1, K=2, h=2, m=0.0)
    c = _const_chunks(3, 3)
    assert ref(c[0], [0])[0, :, 0].tolist() == [0.0, 1.0]
    assert ref(c[1], [2])[0, :, 0].tolist() == [(2 + 10) / 2, 11.0]
    assert ref(c[2], [4])[0, :, 0].tolist() == [(12 + 20) / 2, 21.0]
    assert [s for s, _ in ref.rows[0]] == [2, 4]


def test_new_exports_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/genima_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound by genima_amd/_lib.py"
        assert hasattr(lib, n), f"libgenima_hip.so does not export {n}"
    assert _lib.ABI_VERSION == 101  # exports were appended, no struct changed
    assert "ensemble.hip" in build.SOURCES


def test_library_argument_checks_without_a_device():
    """Size query and record-time refusal are host code; the launcher refuses bad arguments before it touches the device."""
    lib = _lib.load()
    row = lambda T, A, K: (4 * (K * T * A + K + 2) + 15) // 16 * 16  # ring + starts + head + one word of the library's own
    assert lib.gn_action_ensemble_state_bytes(2, 20, 8, 4) == 2 * row(20, 8, 4)
    assert lib.gn_action_ensemble_state_bytes(1, 3, 1, 2) == row(3, 1, 2)
    assert lib.gn_action_ensemble_state_bytes(0, 20, 8, 4) < 0 and lib.gn_action_ensemble_state_bytes(1, 20, 8, 0) < 0
    prog = ctypes.c_void_p()
    mem = ctypes.create_string_buffer(4096)  # real host memory behind every pointer handed over: recording stores pointers, it reads none
    base = (ctypes.addressof(mem) + 63) // 64 * 64
    ctx, buf = ctypes.c_void_p(base), ctypes.c_void_p(base + 1024)  # a zeroed stand-in for the context a program keeps a pointer to
    assert lib.gn_program_create(ctx, ctypes.byref(prog)) == 0
    ok = dict(B=2, T=20, A=8, ld=16, K=4, h=5, m=0.01)

    def add(**kw):
        a = dict(ok, **kw)
        return lib.gn_program_add_action_ensemble(prog, buf, 0, buf, buf, buf, buf, a["B"], a["T"], a["A"], a["ld"], a["K"], a["h"], a["m"])

    assert add() == 0 and lib.gn_program_num_ops(prog) == 1
    for bad in (dict(h=0), dict(h=21), dict(K=3), dict(ld=7), dict(m=-1.0), dict(B=0)):
        assert add(**bad) != 0, bad
        assert b"gn_program_add_action_ensemble" in lib.gn_last_error()
    assert add(K=1, h=20) == 0 and add(h=7, K=3) == 0 and add(h=7, K=2) != 0 and add(h=5, K=1) == 0
    assert lib.gn_program_num_ops(prog) == 4, "a refused op is not recorded"
    assert lib.gn_program_destroy(prog) == 0
    # the launch entry points: without a context nothing can be launched, whatever else is passed (the refusals of h / K / ld by a live
    # context are in tests/test_ensemble_gpu.py)
    for name in ("gn_action_ensemble", "gn_action_ensemble_f16"):
        fn = getattr(lib, name)
        assert fn(None, buf, buf, buf, buf, buf, 2, 20, 8, 16, 4, 5, 0.01) != 0, "null context"
        assert name.encode() in lib.gn_last_error()
        assert fn(None, buf, None, buf, buf, buf, 2, 20, 8, 16, 4, 5, 0.01) != 0 and fn(None, None, buf, buf, buf, None, 2, 20, 8, 16, 4, 0, 0.01) != 0


def test_execution_slots():
    assert execution_slots(20, None, False) == (20, 1) and execution_slots(20, None, True) == (20, 1)
    assert execution_slots(20, 5, True) == (5, 4) and execution_slots(20, 7, True) == (7, 3) and execution_slots(20, 1, True) == (1, 20)
    assert execution_slots(20, 5, False) == (5, 1) and execution_slots(3, 2, True) == (2, 2)
    for bad in (0, -1, 21, 2.5, True):
        with pytest.raises(GenimaHipError, match="execution_horizon"):
            execution_slots(20, bad, True)


def _host_agent():
    fam = configs.family("tiny")
    agent = GenimaACT(fam["act"], None, fam["act_text"], None, device="cpu")  # no device: weights stay on the host, nothing is packed
    return agent, int(fam["act"]["num_queries"])


def test_set_execution_validates_and_keys_the_program():
    agent, T = _host_agent()
    assert agent._exec is None
    agent.set_execution(min(5, T), True)
    assert agent._exec == (min(5, T), -(-T // min(5, T)), 0.01)
    e0 = agent._exec_epoch
    agent.reset_execution()
    assert agent._exec_epoch == e0 + 1, "a full reset reaches every recorded program"
    agent.reset_execution([1])
    assert agent._exec_pending == {1} and agent._exec_epoch == e0 + 1
    for kw in (dict(execution_horizon=0), dict(execution_horizon=T + 1), dict(execution_horizon=1, m=-0.5), dict(execution_horizon=1, m=float("nan"))):
        with pytest.raises(GenimaHipError):
            agent.set_execution(temporal_agg=True, **kw)
    with pytest.raises(GenimaHipError):
        agent.reset_execution([-1])
    agent.set_execution()
    assert agent._exec is None and not agent._exec_pending
    with pytest.raises(GenimaHipError):  # no CPU fallback, with or without an execution mode
        agent.set_execution(1, True)._program(1, 4, 64, 64, False)


def test_per_call_inputs_of_the_op():
    """steps | reset are written as one buffer; the first call of a program, a full reset and listed rows raise the reset flags once."""
    agent, T = _host_agent()
    agent.set_execution(1, True)
    B = 3
    ctl = torch.zeros(5 * B, dtype=torch.uint8)
    io = SimpleNamespace(ens_ctl=ctl, ens_steps=ctl[: 4 * B].view(torch.int32), ens_reset=ctl[4 * B:], ens_epoch=None)
    agent._fill_execution(io, 7, B)
    assert io.ens_steps.tolist() == [7, 7, 7] and io.ens_reset.tolist() == [1, 1, 1]
    agent._fill_execution(io, torch.tensor([8, 1, 300]), B)
    assert io.ens_steps.tolist() == [8, 1, 300] and io.ens_reset.tolist() == [0, 0, 0]
    agent.reset_execution([2])
    agent._fill_execution(io, 9, B)
    assert io.ens_reset.tolist() == [0, 0, 1]
    agent._fill_execution(io, 10, B)
    assert io.ens_reset.tolist() == [0, 0, 0]
    agent.reset_execution()
    agent._fill_execution(io, np.int64(0), B)
    assert io.ens_steps.tolist() == [0, 0, 0] and io.ens_reset.tolist() == [1, 1, 1]
    for bad in (-1, torch.tensor([1, 2]), 2 ** 31 - 1):
        with pytest.raises(GenimaHipError, match="step"):
            agent._fill_execution(io, bad, B)
    agent.reset_execution([B])
    with pytest.raises(GenimaHipError, match="row"):
        agent._fill_execution(io, 0, B)
