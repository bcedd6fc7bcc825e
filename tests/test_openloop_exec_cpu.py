"""-m "not gpu": the host side of the open-loop scores of an execution mode -- the closed form of gn_openloop_exec_actions against the ensemble
rule driven call by call (tests/ensemble_ref.py), the ABI names, ``OpenLoopResult.execution_summary`` on hand-made tables, ``summary()``
untouched by executions, and the command lines' ``--execution`` syntax."""
import ctypes
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest

import openloop_exec_ref as XR
from ensemble_ref import EnsembleRef
from genima_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_openloop_exec_actions", "gn_openloop_exec_metrics")


def _chunks(N, T, A, ld, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-2, 2, (N, T, ld)).astype(np.float16)  # the controller's chunks are f16
    c[..., A:] = np.inf
    return c


def _ring_f32(chunk, T, A, h, K, m):
    """One episode through the ensemble rule as the ring applies it, call by call, in f32 rounded operation by operation: a list of the last K
    (start, chunk) pairs, the covering ones oldest first.  chunk [L, T, >= A] -> f32 [L, A], the action executed at every step."""
    L = chunk.shape[0]
    kept, out = [], np.zeros((L, A), np.float32)
    for t in range(0, L, h):
        kept = (kept + [(t, chunk[t, :, :A].astype(np.float32))])[-K:]
        for s in range(t, min(t + h, L)):
            num, den, i = np.zeros(A, np.float32), np.float32(0), 0
            for start, c in kept:
                if not 0 <= s - start < T:
                    continue
                w = np.float32(1) if i == 0 else np.exp(np.float32(-np.float32(m) * np.float32(i)))
                num = (num + (w * c[s - start]).astype(np.float32)).astype(np.float32)
                den = np.float32(den + w)
                i += 1
            assert i <= K
            out[s] = num / den
    return out


@pytest.mark.parametrize("T", [5, 20])
def test_closed_form_is_the_ensemble_rule_driven_call_by_call(T):
    """Every h in 1 .. T, temporal_agg off and on, m in {0, 0.01, 1}, episodes of 1, 4, 11 and 47 transitions.  The f32 closed form equals the
    ring's loop in f32 bit for bit (the same calls in the same order), and the f64 one equals EnsembleRef's f64 up to the order in which
    numpy adds (1e-12 of the largest value)."""
    A, ld, lengths = 3, 4, (1, 4, 11, 47)
    first = XR.first_transitions(lengths)
    chunks = _chunks(len(first), T, A, ld, seed=T)
    scale = float(np.abs(chunks[..., :A].astype(np.float64)).max())
    for h in range(1, T + 1):
        for agg in (False, True):
            K = -(-T // h) if agg else 1
            for m in (0.0, 0.01, 1.0):
                got32, calls = XR.exec_actions(chunks, first, A, h, agg, m, np.float32)
                got64, _ = XR.exec_actions(chunks, first, A, h, agg, m, np.float64)
                assert calls.max() <= K and calls.min() >= 1
                for f, L in zip(np.unique(first), lengths):
                    ep = chunks[f: f + L]
                    assert np.array_equal(got32[f: f + L].view(np.int32), _ring_f32(ep, T, A, h, K, m).view(np.int32)), (h, agg, m, L)
                    ref = EnsembleRef(1, T, A, K, h, m)
                    for t in range(0, L, h):
                        want = ref(ep[t][None].astype(np.float64), [t], reset=[t == 0])[0]
                        n = min(h, L - t)
                        assert np.abs(got64[f + t: f + t + n] - want[:n]).max() <= 1e-12 * scale, (h, agg, m, L, t)
                        for s in range(t, t + n):  # the taking-part calls are the starts the reference keeps and that cover s
                            assert XR.taking_part(s, T, h, agg) == [st for st, _ in ref.rows[0] if 0 <= s - st < T]
    # without temporal_agg: the executing call's own prediction, exactly
    for h in (1, 2, T):
        got, calls = XR.exec_actions(chunks, first, A, h, False, 0.01, np.float32)
        for n in range(len(first)):
            s = n - first[n]
            assert np.array_equal(got[n], chunks[first[n] + s - s % h, s % h, :A].astype(np.float32)) and calls[n] == 1


def test_known_answers_worked_by_hand():
    """T = 4, one episode of 6 transitions, call c predicts 10 c + j for its j-th step (A = 2: the second column negated)."""
    T, L = 4, 6
    c = np.zeros((L, T, 2))
    c[..., 0] = 10.0 * np.arange(L)[:, None] + np.arange(T)[None]
    c[..., 1] = -c[..., 0]
    first = np.zeros(L, np.int32)
    got, calls = XR.exec_actions(c, first, 2, 2, True, 0.0)
    # h = 2: calls at 0, 2, 4.  step 2: call 0 offset 2, call 2 offset 0; step 3: call 0 offset 3, call 2 offset 1; step 4: calls 2, 4; ...
    assert got[:, 0].tolist() == [0.0, 1.0, (2 + 20) / 2, (3 + 21) / 2, (22 + 40) / 2, (23 + 41) / 2] and calls.tolist() == [1, 1, 2, 2, 2, 2]
    assert np.array_equal(got[:, 1], -got[:, 0])
    w = math.exp(-0.5)
    got, _ = XR.exec_actions(c, first, 2, 2, True, 0.5)
    assert got[2, 0] == pytest.approx((2 + w * 20) / (1 + w), abs=1e-12), "the older call weighs 1, the newer exp(-m)"
    got, calls = XR.exec_actions(c, first, 2, 3, True, 0.0)  # h = 3, K = 2: step 3 <- call 0 offset 3 and call 3 offset 0; steps 4, 5 <- call 3 alone
    assert got[:, 0].tolist() == [0.0, 1.0, 2.0, (3 + 30) / 2, 31.0, 32.0] and calls.tolist() == [1, 1, 1, 2, 1, 1]
    # a second episode starts afresh
    first2 = np.array([0, 0, 0, 3, 3, 3], np.int32)
    got, calls = XR.exec_actions(c, first2, 2, 1, True, 0.0)
    assert got[3, 0] == 30.0 and got[4, 0] == (31 + 40) / 2 and calls.tolist() == [1, 2, 3, 1, 2, 3]


def test_new_exports_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/genima_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound by genima_amd/_lib.py"
        assert hasattr(lib, n), f"libgenima_hip.so does not export {n}"
    assert _lib.ABI_VERSION == 101 and len(_lib.DESC_CLASSES) == 11  # exports were appended, no struct changed or added
    # the replay kernel is compiled beside the ensemble kernel, under its flags, and not under openloop.hip's
    assert "ensemble.hip" in build.SOURCES and "ensemble.hip" not in build.EXTRA_FLAGS and "-ffp-contract=off" in build.EXTRA_FLAGS["openloop.hip"]
    src = open(os.path.join(build.CSRC, "ensemble.hip")).read()
    assert "gn_openloop_exec_actions" in src and src.count("ens_weighted_mean(") == 2, "both kernels take the weighted sum from the shared header"


def test_library_refuses_without_a_context():
    lib = _lib.load()
    mem = ctypes.create_string_buffer(4096)
    buf = ctypes.c_void_p((ctypes.addressof(mem) + 63) // 64 * 64)
    assert lib.gn_openloop_exec_actions(None, buf, buf, buf, None, 16, 5, 3, 8, 2, 1, 0.01) != 0
    assert b"gn_openloop_exec_actions" in lib.gn_last_error()
    assert lib.gn_openloop_exec_metrics(None, buf, buf, buf, None, buf, 16, 3) != 0
    assert b"gn_openloop_exec_metrics" in lib.gn_last_error()


# ---- OpenLoopResult ---------------------------------------------------------------------------------------------------------------------------
def _result(executions=None, chunks=None):
    from genima_amd.openloop import OpenLoopResult

    # 5 transitions: episode 0 (task a) has steps 0 .. 2, episode 1 (task b) steps 0, 1; T = 2, 2 joints
    norm = np.array([[[2.0, 1], [4.0, 0]], [[6.0, 1], [8.0, 1]], [[1.0, 0], [3.0, 1]], [[5.0, 1], [7.0, 0]], [[9.0, 1], [2.0, 1]]], np.float32)
    acts = {"oracle": {"norm": norm, "rad": norm * np.array([0.5, 1], np.float32)}}
    return OpenLoopResult(None, acts, [0, 0, 0, 1, 1], [0, 1, 2, 0, 1], [0, 0, 0, 1, 1], ["a", "b"], ["front"], 2, 4, 4, executions=executions, chunks=chunks)


def _executions():
    # h = 2: positions 0, 1, 0 | 0, 1; the one boundary step is transition 2 (step 2 of episode 0)
    sc = np.array([[2.0, 1, 0.0, 0.0], [4.0, 0, 1.0, 0.5], [6.0, 1, 8.0, 2.0], [8.0, 1, 0.0, 0.0], [10.0, 0, 3.0, 1.0]], np.float32)
    tabs = {"actions": np.zeros((5, 3), np.float32), "n_calls": np.array([1, 1, 2, 1, 1], np.int32), "scores": {"norm": sc, "rad": sc * np.array([0.5, 1, 0.5, 0.5], np.float32)}}
    return [{"h": 2, "temporal_agg": True, "m": 0.01, "K": 1, "oracle": tabs}]


def test_execution_summary_on_hand_made_tables(tmp_path):
    res = _result(_executions(), {"oracle": np.zeros((5, 2, 3), np.float16)})
    (x,) = res.execution_summary()
    assert (x["h"], x["temporal_agg"], x["m"], x["K"], x["calls_per_step"]) == (2, True, 0.01, 1, 0.5) and "generated" not in x
    o = x["oracle"]
    assert o["joint_l1_norm"] == (2 + 4 + 6 + 8 + 10) / 5 / 2 and o["joint_l1_rad"] == o["joint_l1_norm"] / 2 and o["gripper_acc"] == 3 / 5
    assert o["mean_calls"] == 6 / 5
    assert o["by_position"] == {"n": [3, 2], "joint_l1_norm": [(2 + 6 + 8) / 3 / 2, (4 + 10) / 2 / 2], "joint_l1_rad": [(2 + 6 + 8) / 3 / 4, (4 + 10) / 2 / 4],
                                "gripper_acc": [1.0, 0.0]}
    assert o["jump_boundary_norm"] == 8.0 / 2 and o["demo_jump_boundary_norm"] == 2.0 / 2  # transition 2 alone; the first steps are no boundary
    assert o["jump_inside_norm"] == (1.0 + 3.0) / 2 / 2 and o["demo_jump_inside_norm"] == (0.5 + 1.0) / 2 / 2
    assert o["jump_boundary_rad"] == 2.0 and o["jump_inside_rad"] == 0.5
    assert set(x["per_task"]) == {"a", "b"}
    b = x["per_task"]["b"]["oracle"]
    assert b["joint_l1_norm"] == (8 + 10) / 2 / 2 and b["jump_boundary_norm"] is None and b["jump_inside_norm"] == 3.0 / 2, "task b never reaches a second call"
    assert b["by_position"]["n"] == [1, 1]
    # a horizon longer than every episode: positions nobody reaches are None, not NaN
    ex = _executions()
    ex[0]["h"] = 4
    far = _result(ex, res.chunks).execution_summary()[0]["oracle"]
    assert far["by_position"]["n"] == [2, 2, 1, 0] and far["by_position"]["joint_l1_norm"][3] is None and far["jump_boundary_norm"] is None
    # to_json: a key of its own beside the summary
    path = str(tmp_path / "x.json")
    s = res.to_json(path)
    assert s["executions"] == res.execution_summary() and {k: v for k, v in s.items() if k != "executions"} == res.summary()
    with open(path) as f:
        assert json.load(f) == json.loads(json.dumps(s))


def test_summary_ignores_executions(tmp_path):
    plain, with_ex = _result(), _result(_executions(), {"oracle": np.zeros((5, 2, 3), np.float16)})
    assert plain.executions is None and plain.chunks is None and plain.execution_summary() is None
    assert with_ex.summary() == plain.summary()
    assert "executions" not in plain.to_json(str(tmp_path / "p.json"))
    assert set(with_ex.actions) == {"oracle"}


# ---- command lines ------------------------------------------------------------------------------------------------------------------------------
def test_parse_execution():
    from genima_amd.openloop import parse_execution

    assert parse_execution("5") == (5, False, 0.01) and parse_execution("5,agg") == (5, True, 0.01) and parse_execution(" 7 , on , 0.1 ") == (7, True, 0.1)
    assert parse_execution("20,off") == (20, False, 0.01) and parse_execution("1,agg,0") == (1, True, 0.0)
    for bad in ("", "x", "5,maybe", "5,agg,much", "5,agg,0.1,2", "2.5"):
        with pytest.raises(ValueError, match="execution setting"):
            parse_execution(bad)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_openloop_takes_repeated_execution_flags(capsys):
    tool = _tool("eval_openloop")
    base = ["--dataset_root", "d", "--sd_ckpt", "s"]
    a = tool.parse(base + ["--controller_snapshot", "c", "--stats_dir", "t", "--execution", "5,agg", "--execution", "20", "--execution", "1,agg,0.1"])
    assert a.execution == [(5, True, 0.01), (20, False, 0.01), (1, True, 0.1)]
    assert tool.parse(base + ["--controller_snapshot", "c", "--stats_dir", "t"]).execution is None
    for bad in (["--controller_snapshot", "c", "--stats_dir", "t", "--execution", "5,maybe"], ["--no_controller", "--execution", "5"]):
        with pytest.raises(SystemExit):
            tool.parse(base + bad)
    capsys.readouterr()
