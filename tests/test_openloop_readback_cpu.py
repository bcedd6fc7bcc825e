"""The evaluator's named readback (``openloop.read_back``) and the argument checks the eager engine ops share, without a device."""
import numpy as np
import pytest
import torch

from genima_amd import engine as EG
from genima_amd._lib import GenimaHipError
from genima_amd.openloop import read_back, readback_layout


def _tables():
    """Narrow before wide, odd element counts, a None among them: name -> CPU tensor."""
    def ramp(shape, dtype):
        n = int(np.prod(shape))
        return ((torch.arange(n, dtype=torch.float64) * 3 - n) / 4).to(dtype).reshape(shape)

    return {"chunks/oracle": ramp((1,), torch.float16), "exec/0/oracle/n_calls": ramp((3,), torch.int32), "missing": None,
            "actions/oracle/norm": ramp((5, 1), torch.float32), "points": ramp((1, 7), torch.float64), "image": ramp((3, 1, 3), torch.int64),
            "chunks/generated": ramp((11,), torch.float16), "exec/0/oracle/actions": ramp((13,), torch.float32), "spheres": ramp((1,), torch.int64)}


def test_every_table_comes_back_under_its_name_bit_for_bit():
    tabs = _tables()
    got = read_back(tabs)
    assert list(got) == [k for k, t in tabs.items() if t is not None]
    for k, a in got.items():
        want = tabs[k].numpy()
        assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), k
        assert a.base is None and a.flags.writeable, k  # a copy of its own, not a view of the packed buffer
    assert read_back({}) == {} and read_back({"a": None}) == {}


def test_every_table_starts_on_a_multiple_of_its_element_size():
    tabs = _tables()
    lay = readback_layout(tabs)
    assert set(lay) == {k for k, t in tabs.items() if t is not None}
    sizes = [tabs[k].element_size() for k in lay]  # in packing order
    assert sizes == sorted(sizes, reverse=True), "widest first"
    assert [k for k in lay if tabs[k].element_size() == 2] == ["chunks/oracle", "chunks/generated"], "a stable sort keeps the order given"
    end = 0
    for k, o in lay.items():
        assert o == end and o % tabs[k].element_size() == 0, k  # packed without gaps, each on its own grid
        end = o + tabs[k].numel() * tabs[k].element_size()
    # the order given would not do: its first table is one f16 element, which throws the int32 table behind it off its grid
    given = [t for t in tabs.values() if t is not None]
    assert given[0].numel() * given[0].element_size() % given[1].element_size() != 0


def test_one_concatenation_and_one_host_copy(monkeypatch):
    calls = {"cat": 0, "cpu": 0}
    cat, cpu = torch.cat, torch.Tensor.cpu

    def counted_cat(*a, **kw):
        calls["cat"] += 1
        return cat(*a, **kw)

    def counted_cpu(self, *a, **kw):
        calls["cpu"] += 1
        return cpu(self, *a, **kw)

    monkeypatch.setattr(torch, "cat", counted_cat)
    monkeypatch.setattr(torch.Tensor, "cpu", counted_cpu)
    read_back(_tables())
    assert calls == {"cat": 1, "cpu": 1}


# ---- the eager ops' shared argument checks (genima_amd/engine.py): every refusal is a GenimaHipError that names the caller
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the device, so that each clause of the contract can fail on its own here."""
    is_cuda = property(lambda self: True)


def test_expect_refuses_what_is_not_a_contiguous_device_tensor_of_the_shape():
    good = torch.zeros((2, 3)).as_subclass(_OnDevice)
    assert good.is_cuda and good.t().is_cuda and not good.t().is_contiguous()
    EG._expect("some_op", good, torch.float32, (2, 3))
    EG._expect_each("some_op", ((good, torch.float32, (2, 3)), (None, torch.int32, (1,))), optional=True)
    for t, dtype, shape in ((torch.zeros((2, 3)), torch.float32, (2, 3)),  # a CPU tensor
                            (good, torch.float16, (2, 3)), (good.half(), torch.float32, (2, 3)),  # a wrong dtype
                            (good, torch.float32, (3, 2)), (good, torch.float32, (2, 3, 1)), (good, torch.float32, (6,)),  # a wrong shape
                            (good.t(), torch.float32, (3, 2)), (good[:, ::2], torch.float32, (2, 2)),  # views that are not contiguous
                            (None, torch.float32, (2, 3)), (np.zeros((2, 3), np.float32), torch.float32, (2, 3))):
        with pytest.raises(GenimaHipError, match="contiguous device tensor") as ei:
            EG._expect("some_op", t, dtype, shape)
        assert "some_op" in str(ei.value) and str(dtype) in str(ei.value) and str(shape) in str(ei.value)
    assert issubclass(GenimaHipError, RuntimeError)
    EG._expect("some_op", None, torch.float32, (2, 3), optional=True)  # None passes only where the argument is optional
    with pytest.raises(GenimaHipError, match="contiguous device tensor"):
        EG._expect("some_op", torch.zeros((2, 3)), torch.float32, (2, 3), optional=True)
    with pytest.raises(GenimaHipError, match="some_op"):
        EG._expect_each("some_op", ((good, torch.float32, (2, 3)), (None, torch.int32, (1,))))


def test_host_copy_check():
    good = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert EG._host_int32("some_op", None, (2, 3)) is None and EG._host_int32("some_op", good, (2, 3)) == good.ctypes.data
    for bad in (good.astype(np.float64), good.astype(np.int64), good.T, good[:, :2], np.asfortranarray(good)):
        with pytest.raises(GenimaHipError, match="host copy") as ei:
            EG._host_int32("some_op", bad, (2, 3))
        assert "some_op" in str(ei.value)
    with pytest.raises(GenimaHipError, match="host copy"):
        EG.Engine._first_tr_host("some_op", np.zeros(4, np.float64), 4)
    with pytest.raises(GenimaHipError, match=r"first_tr\[2\] = 3 must lie in 0 \.\. 2"):
        EG.Engine._first_tr_host("some_op", np.array([0, 0, 3, 3], np.int32), 4)
    EG.Engine._first_tr_host("some_op", np.array([0, 0, 2, 2], np.int32), 4)


def test_the_eager_guard_keeps_the_name_and_the_reason():
    import types

    EG._eager_only(types.SimpleNamespace(record=False), "some_op", "the rows change")
    with pytest.raises(RuntimeError, match="some_op is an eager op: the rows change"):
        EG._eager_only(types.SimpleNamespace(record=True), "some_op", "the rows change")


def test_replay_index_refuses_host_indices_outside_the_table():
    for idx in ([0, 5], [-1], [], np.array([2, 7])):
        with pytest.raises(GenimaHipError, match=r"some_op: transition indices must lie in \[0, 5\)"):
            EG._replay_index("some_op", idx, 5, "cpu")
