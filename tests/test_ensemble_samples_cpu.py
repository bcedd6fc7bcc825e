"""-m "not gpu": sample-combined action ensembling -- the float64 restatement (tests/ensemble_samples_ref.py) against brute force and known
answers, the medoid margin of every generated test input, the ABI names, and the argument checks that need no device (the library's at
record time, ``GenimaACT.set_execution``, ``harness.control_step``, ``OpenLoopEval(combine=)``)."""
import ctypes
import os
import re

import numpy as np
import pytest

import ensemble_samples_ref as SR
from ensemble_ref import EnsembleRef
from genima_amd import _lib, build, configs, harness
from genima_amd._lib import GenimaHipError
from genima_amd.act import GenimaACT, check_samples
from genima_amd.openloop import OpenLoopEval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_action_ensemble_samples_f16", "gn_openloop_exec_actions_samples", "gn_program_record_action_ensemble_samples")
SHAPES = ((2, 3, 20, 8, 16), (1, 5, 7, 3, 5), (2, 1, 20, 8, 16), (1, 2, 20, 8, 16))  # (B, R, T, A, ld): tests/test_ensemble_samples_gpu.py's
MARGIN = 1e-3


def test_combination_against_brute_force():
    rng = np.random.default_rng(0)
    for R, T, A in ((1, 4, 2), (2, 3, 3), (3, 5, 2), (6, 4, 4)):
        x = rng.uniform(-2, 2, (R, T, A))
        mean, pick, spread = SR.combine(x, "mean")
        brute = np.zeros((T, A))
        for r in range(R):
            brute += x[r]
        assert pick == -1 and np.allclose(mean, brute / R, rtol=0, atol=1e-15)
        assert spread == pytest.approx(sum(abs(x[r, t, a] - mean[t, a]) for r in range(R) for t in range(T) for a in range(A)) / (R * T * A), rel=1e-12)
        D = [sum(abs(x[r, t, a] - x[q, t, a]) for q in range(R) for t in range(T) for a in range(A)) for r in range(R)]
        med, pick, spread = SR.combine(x, "medoid")
        assert pick == int(np.argmin(D)) and np.array_equal(med, x[pick]) and SR.medoid_distances(x) == pytest.approx(D, rel=1e-12)
        assert spread == pytest.approx(D[pick] / (R * T * A), rel=1e-12), "under medoid the spread is the pick's own D over R T A"


def test_known_answers():
    x = np.array([[[0.0, 0.0]], [[1.0, 1.0]], [[10.0, 10.0]]])  # three samples on a line: the middle one is the medoid, the mean is none of them
    med, pick, spread = SR.combine(x, "medoid")
    assert pick == 1 and np.array_equal(med, [[1.0, 1.0]]) and spread == pytest.approx((1 + 0 + 9) / 3)
    mean, _, _ = SR.combine(x, "mean")
    assert mean.tolist() == [[11 / 3, 11 / 3]]
    assert SR.combine(np.stack([x[2], x[0], x[0]]), "medoid")[1] == 1, "two identical samples: the lower index"
    assert SR.combine(x[:2], "medoid")[1] == 0 and SR.medoid_margin(x[:2]) == ([0, 1], np.inf), "R = 2 is a tie by symmetry"
    assert SR.medoid_margin(x) == ([1], pytest.approx(0.1))  # D = (22, 20, 38): the runner-up is sample 0
    assert SR.medoid_margin(x[:1]) == ([0], np.inf)


def test_restatement_delegates_to_the_ensemble_rule():
    rng = np.random.default_rng(1)
    B, R, T, A, h, K = 2, 3, 6, 2, 2, 3
    for rule in SR.RULES:
        ref, plain = SR.EnsembleSamplesRef(B, R, T, A, K, h, 0.01, rule), EnsembleRef(B, T, A, K, h, 0.01)
        for c in range(5):
            x = rng.uniform(-2, 2, (B, R, T, A + 1))
            reset = [c == 3, False]
            got, picks, spreads = ref(x, [c * h] * B, reset)
            comb = np.stack([SR.combine(x[b, :, :, :A], rule)[0] for b in range(B)])
            assert np.array_equal(got, plain(comb, [c * h] * B, reset)) and picks.shape == spreads.shape == (B,)
    # the table replay: one episode, h = 2, no aggregation = the head of the combined chunk of the call that covers the step
    chunks = rng.uniform(-2, 2, (R, 5, T, A))
    out, picks = SR.replay_table(chunks, [0] * 5, 2, False, 0.01, "mean")
    assert np.allclose(out[3], chunks[:, 2, 1].sum(0) / R, rtol=0, atol=1e-15) and (picks == -1).all()


def test_generated_inputs_keep_the_medoid_margin():
    """EVERY (call, row) of every shape the GPU tests use: either the smallest D is shared exactly (a tie by construction: R = 2, or the two
    identical samples of the tie case -- the pick is then the lowest index) or the runner-up lies at least 1e-3 of D above it, twenty times the
    5e-5 that R * T * A f32 additions can move a D."""
    worst, ties = np.inf, 0
    for B, R, T, A, ld in SHAPES:
        x = SR.sample_chunks(B, R, T, A, ld, seed=7)
        assert x.shape == (30, B, R, T, ld) and np.array_equal(x, x.astype(np.float16).astype(np.float32)) and (x[..., A:] == 60000.0).all()
        for c in range(x.shape[0]):
            for b in range(B):
                group, margin = SR.medoid_margin(x[c, b, :, :, :A])
                assert margin >= MARGIN, (B, R, c, b, margin)
                worst = min(worst, margin)
                if R == 2:
                    assert group == [0, 1]
                elif R >= 3 and c == SR.TIE_CALL and b == 0:
                    assert group == [1, 2], "the exact tie: samples 1 and 2 are identical and the best"
                    ties += 1
                else:
                    assert len(group) == 1
    print(f"smallest medoid margin over all cases: {worst:.3e}")
    assert ties == 2


def test_new_exports_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/genima_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound by genima_amd/_lib.py"
        assert hasattr(lib, n), f"libgenima_hip.so does not export {n}"


def test_library_refusals_without_a_device():
    """Record-time refusals are host code: the sample arguments, and an open guarded segment."""
    lib = _lib.load()
    prog, sid = ctypes.c_void_p(), ctypes.c_int32(-1)
    mem = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(mem) + 63) // 64 * 64
    ctx, buf = ctypes.c_void_p(base), base + 1024
    assert lib.gn_program_create(ctx, ctypes.byref(prog)) == 0
    B, T, A, ld = 2, 20, 8, 16
    f32 = lambda v: float(np.float32(v))
    ok = dict(chunk=buf, bs=3 * T * ld, ss=T * ld, R=3, inv_R=f32(1.0 / 3), combine=1, state=buf, out=buf, pick=buf, spread=buf, B=B, T=T, A=A, ld=ld, K=4, h=5,
              m=0.01)

    def add(**kw):
        a = dict(ok, **kw)
        return lib.gn_program_record_action_ensemble_samples(prog, a["chunk"], a["bs"], a["ss"], a["R"], a["inv_R"], a["combine"], a["state"], buf, buf, a["out"],
                                                          a["pick"], a["spread"], a["B"], a["T"], a["A"], a["ld"], a["K"], a["h"], a["m"])

    assert add() == 0 and add(pick=None, spread=None, combine=0) == 0 and lib.gn_program_num_ops(prog) == 2
    assert add(bs=T * ld, ss=B * T * ld) == 0, "the [R][B] layout"
    assert add(R=1, inv_R=1.0, bs=T * ld, ss=0) == 0, "one sample: its stride is not read"
    bad = (dict(h=0), dict(h=21), dict(K=3), dict(ld=7), dict(m=-1.0), dict(B=0), dict(chunk=None), dict(state=buf + 4),   # the sibling's refusals
           dict(R=0), dict(R=65, inv_R=f32(1.0 / 65)), dict(R=64, inv_R=f32(1.0 / 64), T=25, K=1, h=1, bs=64 * 25 * ld, ss=25 * ld),  # 64 * 25 * 8 > 12288 staged
           dict(inv_R=float(np.nextafter(np.float32(1.0 / 3), np.float32(1)))), dict(inv_R=0.33333), dict(combine=2), dict(combine=-1),
           dict(chunk=buf + 1), dict(pick=buf + 2), dict(spread=buf + 2), dict(out=buf + 2),
           dict(ss=(T - 1) * ld + A - 1), dict(bs=2 * T * ld + (T - 1) * ld + A - 1), dict(ss=-T * ld), dict(bs=-3 * T * ld), dict(bs=T * ld, ss=T * ld))
    for kw in bad:
        assert add(**kw) != 0, kw
        assert b"gn_program_record_action_ensemble_samples" in lib.gn_last_error(), kw
    assert lib.gn_program_num_ops(prog) == 4, "a refused op is not recorded"
    assert lib.gn_program_begin_segment(prog, ctypes.byref(sid)) == 0
    assert add() != 0 and b"guarded segment" in lib.gn_last_error() and lib.gn_program_num_ops(prog) == 4
    assert lib.gn_program_end_segment(prog) == 0 and add() == 0 and lib.gn_program_num_ops(prog) == 5, "exactly one op per accepted call"
    assert lib.gn_program_record_action_ensemble_samples(None, buf, 3 * T * ld, T * ld, 3, f32(1.0 / 3), 1, buf, buf, buf, buf, buf, buf, B, T, A, ld, 4, 5, 0.01) != 0
    assert b"gn_program_record_action_ensemble_samples" in lib.gn_last_error(), "a NULL program is refused by name"
    assert lib.gn_program_destroy(prog) == 0
    # the launch entry points refuse without a context, whatever else is passed
    assert lib.gn_action_ensemble_samples_f16(None, buf, 3 * T * ld, T * ld, 3, f32(1.0 / 3), 0, buf, buf, buf, buf, None, None, B, T, A, ld, 4, 5, 0.01) != 0
    assert b"gn_action_ensemble_samples_f16" in lib.gn_last_error()
    assert lib.gn_openloop_exec_actions_samples(None, buf, T * ld, 9 * T * ld, 3, f32(1.0 / 3), 0, buf, buf, None, None, 9, T, A, ld, 5, 1, 0.01) != 0
    assert b"gn_openloop_exec_actions_samples" in lib.gn_last_error()


def _host_agent():
    fam = configs.family("tiny")
    return GenimaACT(fam["act"], None, fam["act_text"], None, device="cpu"), int(fam["act"]["num_queries"])


def test_set_execution_takes_the_sample_mode():
    agent, T = _host_agent()
    assert agent.execution is None and agent.execution_samples is None and agent.last_samples is None
    agent.set_execution(samples=3)
    assert agent.execution == (T, 1, 0.01) and agent.execution_samples == (3, "mean"), "samples alone: the whole combined chunk, one slot"
    agent.set_execution(min(5, T), True, samples=2, combine="medoid")
    assert agent.execution == (min(5, T), -(-T // min(5, T)), 0.01) and agent.execution_samples == (2, "medoid")
    agent.set_execution(min(5, T), True)
    assert agent.execution_samples is None and agent.execution is not None, "the 3-tuple is what it was without samples"
    for kw in (dict(samples=0), dict(samples=65), dict(samples=2.0), dict(samples=True), dict(samples=2, combine="median"), dict(combine="medoid")):
        with pytest.raises(GenimaHipError):
            agent.set_execution(**kw)
    agent.set_execution()
    assert agent.execution is None and agent.execution_samples is None
    assert check_samples(None, "mean") is None and check_samples(4, "medoid") == (4, "medoid")
    with pytest.raises(GenimaHipError):  # no CPU fallback in the sample mode either
        agent.set_execution(samples=2)._program(2, 4, 64, 64, False)


def test_control_step_checks_its_sample_arguments():
    agent, _ = _host_agent()
    obs = {"front_rgb": np.zeros((2, 3, 8, 8), np.uint8)}
    for kw, err in ((dict(samples=0), GenimaHipError), (dict(samples=2, combine="median"), GenimaHipError), (dict(combine="medoid"), ValueError)):
        with pytest.raises(err):
            harness.control_step(None, agent, obs, "goal", ["front"], 1, [None], 1, 0.0, "cpu", **kw)
    with pytest.raises(ValueError, match="one frame per call"):
        harness.control_step(None, agent, obs, "goal", ["front"], 2, [None], 1, 0.0, "cpu", samples=2)


def test_openloop_combine_needs_seeds_and_executions():
    agent, _ = _host_agent()
    dagent = object()  # the options are checked before any agent is touched
    ev = OpenLoopEval.__new__(OpenLoopEval)
    check = lambda **kw: ev._check_options(dagent, agent, ("a", "b", "c", "d"), ((), ()), object(), 30, None, kw.pop("executions", None), False, 0.5, 1e-6, None,
                                           kw.pop("seeds", None), 0.5, kw.pop("combine", None))
    check(seeds=3, executions=[(5, True)], combine=("mean", "medoid"))
    assert ev.combine == ("mean", "medoid")
    check(seeds=3, executions=[(5, True)], combine="medoid")
    assert ev.combine == ("medoid",)
    check(seeds=3, executions=[(5, True)])
    assert ev.combine is None
    for kw in (dict(seeds=3, combine=("mean",)), dict(executions=[(5, True)], combine=("mean",)), dict(combine=("mean",))):
        with pytest.raises(ValueError, match="needs seeds=R and executions"):
            check(**kw)
    for bad in ((), ("median",), ("mean", "mean"), "both"):
        with pytest.raises(ValueError, match="combine is None or distinct rules"):
            check(seeds=3, executions=[(5, True)], combine=bad)
