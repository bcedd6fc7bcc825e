"""LossScaler (genima_amd/loss_scaler.py) without a device: the bookkeeping against a trace recorded from the trainers' own code before
the scaler was factored out of them (tests/golden/loss_scaler_trace.json names the commit), the deferred read-back with a stand-in for
the event, and the checkpoint vector."""
import json
import os

import pytest
import torch

from genima_amd.loss_scaler import LossScaler

with open(os.path.join(os.path.dirname(__file__), "golden", "loss_scaler_trace.json")) as _f:
    GOLDEN = json.load(_f)
SCRIPT = [tuple(t) for t in GOLDEN["script"]]


def _state(s: LossScaler, applied: bool) -> dict:
    return dict(applied=applied, loss_scale=s.scale, clean=s.clean, opt_step=s.opt_step, sched_step=s.sched_step, grad_norm=s.grad_norm)


def test_the_script_covers_the_cases():
    bad = [bool(t[2]) for t in SCRIPT]
    grew = [i for i in range(1, len(SCRIPT)) if GOLDEN["growth_interval_3"][i]["loss_scale"] > GOLDEN["growth_interval_3"][i - 1]["loss_scale"]]
    short = [i for i in range(1, len(SCRIPT)) if bad[i] and GOLDEN["growth_interval_3"][i - 1]["clean"] == GOLDEN["growth_interval"] - 1]
    assert bad[0], "a bad step first"
    assert any(a and b for a, b in zip(bad, bad[1:])), "two bad steps in a row"
    assert short, "a bad step one short of growth"
    assert grew, "a growth"
    assert any(i + 1 < len(bad) and bad[i + 1] for i in grew), "a bad step directly after a growth"
    assert len(GOLDEN["produced_by_commit"]) == 40


def test_golden_trace_with_growth():
    s = LossScaler(GOLDEN["initial_scale"], GOLDEN["growth_interval"])
    for i, (triple, want) in enumerate(zip(SCRIPT, GOLDEN["growth_interval_3"])):
        s.opt_step += 1  # the trainer advances it before AdamW runs
        assert _state(s, s.apply(*triple)) == want, i


def test_golden_trace_without_growth_only_halves():
    s = LossScaler(GOLDEN["initial_scale"], None)
    scales = [s.scale]
    for i, (triple, want) in enumerate(zip(SCRIPT, GOLDEN["growth_interval_none"])):
        s.opt_step += 1
        got = _state(s, s.apply(*triple))
        assert {k: got[k] for k in want} == want, i
        scales.append(s.scale)
    assert all(b in (a, 0.5 * a) for a, b in zip(scales, scales[1:])) and s.sched_step == sum(1 for t in SCRIPT if not t[2])


def test_synchronous_update_reads_the_three_scalars():
    s = LossScaler(1024.0, 2)
    s.opt_step += 1
    assert s.update(torch.tensor([0.0, float("inf"), 1.0])) is False
    assert (s.scale, s.clean, s.opt_step, s.sched_step, s.grad_norm) == (512.0, 0, 0, 0, float("inf"))
    s.opt_step += 1
    assert s.update(torch.tensor([0.5, 2.0, 0.0])) is True
    assert (s.scale, s.clean, s.opt_step, s.sched_step, s.grad_norm) == (512.0, 1, 1, 1, 2.0)


class _Event:
    """What the scaler needs of a torch.cuda.Event: the scalars are in the host tensor once synchronize() returns."""

    def __init__(self, host, values):
        self.host, self.values, self.waits = host, values, 0

    def synchronize(self):
        self.waits += 1
        self.host.copy_(torch.tensor(self.values))


@pytest.mark.parametrize("field", ["scale", "clean", "opt_step", "sched_step", "grad_norm"])
def test_a_read_of_any_field_applies_the_deferred_update_once(field):
    s = LossScaler(1024.0, 2000)
    s.opt_step += 1
    host = torch.zeros(3)
    ev = _Event(host, [0.0, 7.0, 1.0])
    s.defer(host, ev)
    assert s.pending and ev.waits == 0, "queuing does not wait"
    getattr(s, field)
    assert not s.pending and ev.waits == 1
    assert (s.scale, s.clean, s.opt_step, s.sched_step, s.grad_norm) == (512.0, 0, 0, 0, 7.0)
    assert ev.waits == 1, "applied exactly once"


def test_a_second_deferred_update_settles_the_first_before_queuing():
    s = LossScaler(1024.0, 2000)
    host = torch.zeros(3)  # ONE reused buffer: the first update must be applied before the second lands in it
    first, second = _Event(host, [0.0, 7.0, 1.0]), _Event(host, [1.0, 0.5, 0.0])
    s.opt_step += 1
    s.defer(host, first)
    s._opt_step += 1  # (the next step's advance, without a look at the state)
    s.defer(host, second)
    assert first.waits == 1 and second.waits == 0 and s.pending
    assert (s._scale, s._opt_step, s._sched_step) == (512.0, 1, 0), "the first is applied, the second is not yet"
    assert (s.scale, s.clean, s.opt_step, s.sched_step, s.grad_norm) == (512.0, 1, 1, 1, 0.5)
    assert second.waits == 1 and not s.pending


@pytest.mark.parametrize("field,value", [("scale", 2.0 ** 30), ("clean", 5), ("opt_step", 9), ("sched_step", 9)])
def test_assigning_a_field_settles_first(field, value):
    s = LossScaler(1024.0, 2000)
    s.opt_step += 1
    host = torch.zeros(3)
    ev = _Event(host, [0.0, 7.0, 1.0])
    s.defer(host, ev)
    setattr(s, field, value)
    assert ev.waits == 1 and not s.pending
    want = dict(scale=512.0, clean=0, opt_step=0, sched_step=0)
    want[field] = value  # the assignment lands on top of the applied update, not under it
    assert dict(scale=s.scale, clean=s.clean, opt_step=s.opt_step, sched_step=s.sched_step) == want


def test_checkpoint_vector_round_trips_and_reads_the_four_entry_form():
    s = LossScaler(65536.0, 3)
    for triple in SCRIPT[:9]:
        s.opt_step += 1
        s.apply(*triple)
    vec = s.state_vector(41)
    assert vec.dtype == torch.float64 and vec.tolist() == [s.opt_step, s.scale, s.clean, 41, s.sched_step]
    r = LossScaler(1.0, 3)
    assert r.load_state_vector(vec) == 41
    assert (r.opt_step, r.scale, r.clean, r.sched_step) == (s.opt_step, s.scale, s.clean, s.sched_step)
    assert all(isinstance(v, int) for v in (r.opt_step, r.clean, r.sched_step))
    old = LossScaler(1.0, 3)  # written before sched_step was saved: the schedule resumes at the global step
    assert old.load_state_vector(vec[:4]) == 41
    assert (old.opt_step, old.scale, old.clean, old.sched_step) == (s.opt_step, s.scale, s.clean, 41)
