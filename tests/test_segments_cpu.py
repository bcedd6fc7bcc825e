"""-m "not gpu": guarded segments -- the ABI names (header, loader, library), and the host-side policy of the pipeline and of the engine's
liveness check, driven through a stand-in engine (no device)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from genima_amd import _lib, build
from genima_amd._lib import GenimaHipError
from genima_amd.engine import Engine
from genima_amd.pipeline import StableDiffusionControlNetPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_program_begin_segment", "gn_program_end_segment", "gn_program_set_segment_enabled", "gn_program_last_run_ops", "gn_bytes_changed")


def test_new_exports_are_declared_bound_and_exported():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genima_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/genima_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not bound by genima_amd/_lib.py"
        assert hasattr(lib, n), f"libgenima_hip.so does not export {n}"
    assert _lib.ABI_VERSION == 101  # exports were appended, no struct changed


def test_segment_calls_without_a_device():
    """The segment bookkeeping of the library is host code: record-time marking and the flags work on a program without a single op."""
    lib = _lib.load()
    prog, seg = ctypes.c_void_p(), ctypes.c_int32(-1)
    ctx = ctypes.c_void_p(1)  # never dereferenced by the calls below
    assert lib.gn_program_create(ctx, ctypes.byref(prog)) == 0
    assert lib.gn_program_end_segment(prog) != 0, "no open segment"
    assert lib.gn_program_begin_segment(prog, ctypes.byref(seg)) == 0 and seg.value == 0
    assert lib.gn_program_begin_segment(prog, ctypes.byref(seg)) != 0, "segments do not nest"
    assert lib.gn_program_end_segment(prog) == 0
    assert lib.gn_program_begin_segment(prog, ctypes.byref(seg)) == 0 and seg.value == 1
    assert lib.gn_program_end_segment(prog) == 0
    assert lib.gn_program_set_segment_enabled(prog, 1, 0) == 0
    assert lib.gn_program_set_segment_enabled(prog, 2, 0) != 0, "no such segment"
    assert lib.gn_program_last_run_ops(prog) == 0
    assert lib.gn_program_destroy(prog) == 0


class _FakeEngine:
    """What pipeline._replay / _ids_changed use of an Engine."""

    def __init__(self, hoist=True, segments=("prompt", "constants")):
        self.hoist = hoist
        self.segments = {n: dict(enabled=True) for n in segments}
        self.replays = []   # per replay: the names of the segments that ran
        self.device_state = {}
        self.fail_next = False

    def set_segment(self, name, on):
        self.segments[name]["enabled"] = bool(on)

    def _replay(self):
        if self.fail_next:
            self.fail_next = False
            raise RuntimeError("replay failed")
        self.replays.append(tuple(n for n, s in self.segments.items() if s["enabled"]))

    run = launch = _replay

    def changed(self, live, key, stream=None):  # the device comparison, on CPU tensors here
        last = self.device_state.get(key)
        self.device_state[key] = live.clone()
        return last is None or not torch.equal(last, live)

    def forget(self, key=None):
        self.device_state.pop(key, None)


class _DeviceIds:
    """Ids that claim to live on the device (the comparison then goes through Engine.changed on the program's own buffer)."""

    def __init__(self, t):
        self.t, self.device = t, SimpleNamespace(type="cuda")


def _call(pipe, io, ids, on_device=False):
    io.ids.copy_(ids)
    src = _DeviceIds(ids) if on_device else ids
    changed = pipe._ids_changed(io, [(io.ids, src, "ids")], None)
    pipe._replay(io, changed, None)


def _program(**kw):
    pipe = StableDiffusionControlNetPipeline.__new__(StableDiffusionControlNetPipeline)
    io = SimpleNamespace(engine=_FakeEngine(**kw), prompt_valid=False, const_done=False, ids_host={}, ids=torch.zeros(2, 77, dtype=torch.int32))
    pipe._progs = {"k": io}
    return pipe, io


def test_policy_runs_each_segment_only_when_needed():
    pipe, io = _program()
    a = torch.zeros(2, 77, dtype=torch.int32)
    b = a.clone()
    b[1, 3] = 9  # one row of the batch
    for ids in (a, a, a, b, a, a):
        _call(pipe, io, ids)
    both, prompt = ("prompt", "constants"), ("prompt",)
    assert io.engine.replays == [both, (), (), prompt, prompt, ()]
    assert all(s["enabled"] for s in io.engine.segments.values()), "direct replays of the engine always run everything"
    # host ids, then the same ids from the device: the device snapshot is not trusted across the switch -- and back
    _call(pipe, io, a, on_device=True)
    _call(pipe, io, a, on_device=True)
    _call(pipe, io, a)
    _call(pipe, io, a)
    assert io.engine.replays[6:] == [prompt, (), prompt, ()]


def test_policy_reruns_after_a_failed_replay_and_after_weights_changed():
    pipe, io = _program()
    a = torch.zeros(2, 77, dtype=torch.int32)
    b = a + 1
    _call(pipe, io, a)
    io.engine.fail_next = True
    with pytest.raises(RuntimeError):
        _call(pipe, io, b)  # the ids were taken in, the segment's outputs were not produced
    assert all(s["enabled"] for s in io.engine.segments.values())
    _call(pipe, io, b)
    assert io.engine.replays[-1] == ("prompt",), "an unchanged prompt after a failed replay still runs the segment"
    _call(pipe, io, b)
    assert io.engine.replays[-1] == ()
    pipe.weights_changed()
    _call(pipe, io, b)
    assert io.engine.replays[-1] == ("prompt", "constants")


def test_gn_hoist_0_keeps_every_segment_enabled():
    pipe, io = _program(hoist=False)
    a = torch.zeros(2, 77, dtype=torch.int32)
    for _ in range(3):
        pipe._replay(io, False, None)
    assert io.engine.replays == [("prompt", "constants")] * 3


def test_liveness_check_on_host_tensors():
    """Engine._check_segment_writes is address arithmetic: it can be driven with host tensors on an engine that was never initialised."""
    E = Engine.__new__(Engine)
    E._seg_open, E._seg_writes, E._plain_writes = None, [], []
    big = torch.zeros(64, 32, dtype=torch.float16)
    E._check_segment_writes([big[:8]])           # an op in front of the segment
    E._seg_open = "s"
    E._check_segment_writes([big[16:24, :16]])   # a strided view written inside it
    with pytest.raises(GenimaHipError, match="outside it writes"):
        E._check_segment_writes([big[4:12]])     # overlaps what the earlier op writes on every replay
    E._seg_open = None
    E._check_segment_writes([big[24:32], None])  # next to the segment's bytes: fine
    with pytest.raises(GenimaHipError, match="segment 's'"):
        E._check_segment_writes([big[23:25]])    # row 23 belongs to the segment's view
    E._seg_open = "t"
    with pytest.raises(GenimaHipError, match="segment 's'"):
        E._check_segment_writes([big[16:17]])    # another segment is "outside" too
