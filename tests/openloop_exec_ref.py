"""The rule of ``gn_openloop_exec_actions`` / ``gn_openloop_exec_metrics`` (include/genima_hip.h states it) in plain numpy, for
tests/test_openloop_exec_cpu.py, tests/test_openloop_exec_kernels_gpu.py and tests/test_openloop_exec_gpu.py.

TEST INFRASTRUCTURE ONLY; nothing of genima_amd is imported.  ``exec_actions(..., dtype=np.float32)`` mirrors the kernel's order operation by
operation (every product, sum and quotient rounded to f32; the device may fuse a product into its sum and its expf may differ by an ulp, so this
form is close to the device, not equal); ``dtype=np.float64`` is the reference.
"""
from __future__ import annotations

import numpy as np

import openloop_ref as OR


def first_transitions(lengths) -> np.ndarray:
    """Episodes of ``lengths`` transitions laid end to end -> int32 [N]: the first transition of each one's episode."""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.repeat(starts, lengths).astype(np.int32)


def taking_part(s: int, T: int, h: int, temporal_agg: bool):
    """The starts of the calls whose chunks are averaged for step ``s`` of an episode, oldest first."""
    t = s - s % h
    if not temporal_agg:
        return [t]
    jmax = (T - 1 - (s - t)) // h
    return [t - j * h for j in range(jmax, -1, -1) if t - j * h >= 0]


def exec_actions(chunks, first_tr, A: int, h: int, temporal_agg: bool, m: float, dtype=np.float64):
    """chunks [N, T, >= A] (any float dtype; taken at its own values), first_tr int [N] -> (exec ``dtype`` [N, A], n_calls int32 [N])."""
    N, T = chunks.shape[:2]
    c = np.asarray(chunks)[:, :, :A].astype(dtype)
    out, n_calls = np.zeros((N, A), dtype), np.zeros(N, np.int32)
    for n in range(N):
        f = min(max(int(first_tr[n]), 0), n)  # the kernel's clamp
        s = n - f
        us = taking_part(s, T, h, temporal_agg)
        num, den = np.zeros(A, dtype), dtype(0)
        for i, u in enumerate(us):
            w = dtype(1) if i == 0 else np.exp(dtype(-dtype(m) * dtype(i)))
            num = (num + (w * c[f + u, s - u]).astype(dtype)).astype(dtype)
            den = dtype(den + w)
        out[n] = num / den
        n_calls[n] = len(us)
    return out, n_calls


def exec_metrics(ex, demo, first_tr, scale=None):
    """ex, demo f32 [N, A], first_tr int [N], scale f32 [A - 1] or None -> (out f64 [N, 4], bound f64 [N, 4]): the four columns of
    ``gn_openloop_exec_metrics`` in f64, and per column the bound of tests/openloop_ref.py ``action_metrics`` -- (A + 2) 2^-24 times the sum:
    each device term is one f32 subtraction (relative error 2^-24), one f32 multiplication and at most A - 2 f32 additions -- for the three
    sums; the flag is exact (bound 0)."""
    ex, demo = np.asarray(ex, np.float32), np.asarray(demo, np.float32)
    N = ex.shape[0]
    first = np.asarray(first_tr)[:N] >= np.arange(N)
    out, bound = np.zeros((N, 4)), np.zeros((N, 4))
    total, flag, b = OR.action_metrics(ex[:, None, :], demo[:, None, :], scale)
    out[:, 0], out[:, 1], bound[:, 0] = total[:, 0], flag[:, 0], b[:, 0]
    for col, x in ((2, ex), (3, demo)):
        prev = np.concatenate([x[:1], x[:-1]])
        total, _, b = OR.action_metrics(x[:, None, :], prev[:, None, :], scale)
        out[:, col], bound[:, col] = np.where(first, 0.0, total[:, 0]), np.where(first, 0.0, b[:, 0])
    return out, bound
