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


def test_recording_without_a_device():
    """Recording is host code too: every ``gn_program_add_*`` appends exactly one op (stream markers included), and what it refuses at
    record time it refuses by name and appends nothing.  Pointers are stored, never read, so zeroed host memory stands in for the context
    and the tensors; nothing here replays the program."""
    lib = _lib.load()
    mem = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(mem) + 63) // 64 * 64
    ctx, buf = ctypes.c_void_p(base), ctypes.c_void_p(base + 1024)
    prog = ctypes.c_void_p()
    assert lib.gn_program_create(ctx, ctypes.byref(prog)) == 0
    three = (ctypes.c_void_p * 3)(buf, buf, buf)
    four = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    ptrs, lens = (ctypes.c_void_p * 2)(buf, buf), (ctypes.c_int64 * 2)(8, 16)
    gemm = _lib.GemmDesc(M=123, N=40, K=64)
    byref = ctypes.byref
    ops = {  # entry point -> arguments behind the program
        "gemm": (byref(gemm),), "attention": (byref(_lib.AttnDesc()),), "groupnorm": (byref(_lib.GroupNormDesc()),),
        "tblock": (byref(_lib.TBlockDesc()),), "conv3x3_gn": (byref(_lib.ConvGnDesc()),), "conv3x3_patch": (byref(_lib.ConvPatchDesc()),),
        "tiny_block": (buf, three, three, buf, 1, 5, 7, 64), "layernorm": (buf, buf, buf, buf, 5, 24, 1e-5),
        "timestep_embedding": (buf, buf, 3, 16, 1, 0.5), "scale_pad": (buf, buf, 5, 6, 16, 0.5),
        "scale_cat_pad": (buf, buf, buf, 7, 5, 12, 3, 20, 16, 0.5, 2.0), "euler_step": (buf, buf, 9, 4, 8, 2.5, 1.25),
        "image_f16_to_u8": (buf, buf, 30, 8), "image_u8_to_f16": (buf, buf, 30, 8, 2.0, -1.0),
        "image_normalize_u8": (buf, buf, 30, 8, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0), "add": (buf, buf, buf, 104),
        "add_multi": (ptrs, ptrs, ptrs, lens, 2), "add_noise": (buf, buf, buf, buf, buf, 3, 40), "act": (buf, buf, 48, 2),
        "film": (buf, buf, buf, buf, 48, 3, 6, 16, 1), "embedding": (buf, buf, buf, buf, 2, 3, 8), "softmax_rows": (buf, 5, 16, 24, 0.7),
        "maxpool3x3s2": (buf, buf, 2, 5, 7, 8), "gather_rows": (buf, buf, buf, 2, 3, 8), "copy4d": (buf, buf, four, four, four, 8),
        "argmax_rows_i32": (buf, buf, 5, 7), "action_ensemble": (buf, 1, buf, buf, buf, buf, 2, 6, 5, 8, 4, 3, 0.02),
        "memset": (buf, 256), "fork": (), "main": (), "join": (),
    }
    assert {"gn_program_add_" + n for n in ops} == {n for n in _lib.SIGNATURES if n.startswith("gn_program_add_")}, "one of each kind"
    index = {}
    for n, (name, args) in enumerate(ops.items()):
        fn = getattr(lib, "gn_program_add_" + name)
        assert fn(prog, *args) == 0, (name, lib.gn_last_error())
        assert lib.gn_program_num_ops(prog) == n + 1, name
        index[name] = n
    count = len(ops)

    def refused(name, *args, program=prog):
        assert getattr(lib, "gn_program_add_" + name)(program, *args) != 0, (name, args)
        assert ("gn_program_add_" + name).encode() in lib.gn_last_error(), (name, lib.gn_last_error())
        assert lib.gn_program_num_ops(prog) == count, f"{name}: a refused op is not recorded"

    for name, args in ops.items():
        refused(name, *args, program=None)
    for name in ("gemm", "attention", "groupnorm", "tblock", "conv3x3_gn", "conv3x3_patch"):
        refused(name, None)
    refused("tiny_block", buf, None, three, buf, 1, 5, 7, 64)
    refused("tiny_block", buf, three, None, buf, 1, 5, 7, 64)
    refused("tiny_block", buf, three, three, buf, 1, 5, 7, 32)   # unsupported channel count
    refused("tiny_block", buf, three, three, buf, 0, 5, 7, 64)
    refused("tiny_block", None, three, three, buf, 1, 5, 7, 64)
    for bad in (dict(h=0), dict(h=7), dict(K=0), dict(ld=4), dict(m=-1.0), dict(B=0), dict(state=None)):  # h > T, K < ceil(T / h), ld < A
        a = dict(dict(state=buf, B=2, T=6, A=5, ld=8, K=4, h=3, m=0.02), **bad)
        refused("action_ensemble", buf, 0, a["state"], buf, buf, buf, a["B"], a["T"], a["A"], a["ld"], a["K"], a["h"], a["m"])
    for arrays in ((None, four, four), (four, None, four), (four, four, None)):
        refused("copy4d", buf, buf, *arrays, 8)
    refused("add_multi", ptrs, ptrs, ptrs, lens, 0)
    refused("add_multi", ptrs, ptrs, ptrs, lens, 17)
    refused("add_multi", None, ptrs, ptrs, lens, 2)
    refused("memset", None, 256)
    refused("memset", buf, 0)

    # the payloads that are read and rewritten after recording are where they were put
    back = _lib.GemmDesc()
    assert lib.gn_program_get_gemm(prog, index["gemm"], byref(back)) == 0 and (back.M, back.N, back.K) == (123, 40, 64)
    assert all(lib.gn_program_get_gemm(prog, i, byref(back)) != 0 for name, i in index.items() if name != "gemm")
    assert lib.gn_program_set_memset_bytes(prog, index["memset"], 128) == 0
    assert lib.gn_program_set_memset_bytes(prog, index["memset"], 256) != 0, "a memset only shrinks"
    assert lib.gn_program_set_memset_bytes(prog, index["add"], 8) != 0 and b"gn_program_set_memset_bytes" in lib.gn_last_error()
    assert lib.gn_program_num_ops(prog) == count
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
