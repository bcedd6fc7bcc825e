"""Host side of the open-loop evaluation: the wrapped-uint8 score against ``validation.normalized_error`` (already pinned to the reference),
``OpenLoopResult.summary`` on hand-made tables, and ``ControllerTrainLoop``'s ``validate`` hook -- ``validation.jsonl``, ``best.pt``, pruning,
resume -- with a stub agent and replay."""
import json
import os

import numpy as np
import torch

import openloop_ref as OR
from genima_amd import validation
from genima_amd.act_train_loop import ControllerTrainLoop
from genima_amd.openloop import OpenLoopResult


def test_wrap_sq_is_the_reference_validation_mse():
    rng = np.random.RandomState(3)
    for H, W in ((9, 7), (32, 32)):
        gen, gt = (rng.randint(0, 256, (2, 3, H, W, 3)).astype(np.uint8) for _ in range(2))
        m = OR.image_metrics(gen, gt, rng.randint(0, 2, (2, 3, H, W)).astype(np.uint8))
        for b in range(2):
            for v in range(3):
                assert m[b, v, 4] / (H * W * 3) == validation.normalized_error(gen[b, v], gt[b, v])[1]
        assert (m[..., 1] + m[..., 3] == H * W).all()
        d = gen.astype(np.int64) - gt.astype(np.int64)
        assert np.array_equal(m[..., 0] + m[..., 2], (d * d).sum(axis=(-1, -2, -3)))


def _result():
    # 3 transitions, 2 cameras, T = 2, 2 joints; transition 2 draws no sphere (n_in = 0) in either view; two tasks
    image = np.zeros((3, 2, 5), np.int64)
    image[0, 0], image[0, 1] = [3 * 4 * 4, 4, 3 * 12 * 1, 12, 48], [3 * 2 * 9, 2, 0, 14, 96]
    image[1, 0], image[1, 1] = [3 * 8 * 16, 8, 3 * 8 * 4, 8, 0], [0, 0, 3 * 16 * 25, 16, 48]
    image[2, 0], image[2, 1] = [0, 0, 3 * 16 * 9, 16, 96], [0, 0, 3 * 16 * 1, 16, 0]
    norm = np.array([[[2.0, 1], [4.0, 0]], [[6.0, 1], [8.0, 1]], [[1.0, 0], [3.0, 1]]], np.float32)
    acts = {"generated": {"norm": norm, "rad": norm * np.array([0.5, 1], np.float32)}, "oracle": {"norm": norm * np.array([0.25, 1], np.float32), "rad": norm * np.array([0.125, 1], np.float32)}}
    return OpenLoopResult(image, acts, [0, 0, 1], [0, 1, 0], [0, 0, 1], ["a", "b"], ["front", "wrist"], 2, 4, 4)


def test_summary_aggregation_with_missing_sphere_rows(tmp_path):
    res = _result()
    s = res.summary()
    g, o = s["generated"], s["oracle"]
    assert s["n"] == 3 and g["joint_l1_norm"] == (2 + 4 + 6 + 8 + 1 + 3) / 6 / 2 and g["joint_l1_rad"] == g["joint_l1_norm"] / 2
    assert o["joint_l1_norm"] == g["joint_l1_norm"] / 4 and o["joint_l1_rad"] == g["joint_l1_norm"] / 8
    assert g["gripper_acc"] == 4 / 6 and g["per_t"]["gripper_acc"] == [2 / 3, 2 / 3]
    assert g["per_t"]["joint_l1_norm"] == [(2 + 6 + 1) / 3 / 2, (4 + 8 + 3) / 3 / 2]
    im = s["image"]
    assert im["sphere_rmse"] == {"front": (2.0 + 4.0) / 2, "wrist": 3.0} and im["sphere_missing"] == {"front": 1, "wrist": 2}
    assert im["background_rmse"] == {"front": (1.0 + 2.0 + 3.0) / 3, "wrist": (0.0 + 5.0 + 1.0) / 3}
    assert im["wrapped_mse"] == ((48 + 96) + 48 + 96) / 3 / (2 * 4 * 4 * 3)
    assert np.isnan(res.sphere_rmse()[2]).all() and res.sphere_rmse()[1, 0] == 4.0
    # per task: task b is the one transition without spheres -> reported as missing (None), not as 0 and not as NaN
    assert set(s["per_task"]) == {"a", "b"} and s["per_task"]["b"]["n"] == 1
    assert s["per_task"]["b"]["image"]["sphere_rmse"] == {"front": None, "wrist": None} and s["per_task"]["b"]["generated"]["joint_l1_norm"] == 1.0
    assert s["per_task"]["a"]["image"]["sphere_rmse"]["front"] == 3.0
    path = str(tmp_path / "out" / "openloop.json")
    assert res.to_json(path) == s
    with open(path) as f:
        assert json.load(f) == json.loads(json.dumps(s))


class _StubAgent:
    def __init__(self):
        self.w = torch.zeros(3)

    def state_dict(self):
        return {"actor.w": self.w.clone()}

    def load_state_dict(self, sd, strict=False):
        self.w = sd["actor.w"].clone()

    def update_device(self, batch, step=0):
        self.w += 1
        return {"actor_loss": float(self.w[0])}


class _StubReplay:
    action_stats = {"mean": np.zeros(3), "std": np.ones(3)}
    proprio_stats = {"mean": np.zeros(3), "std": np.ones(3)}

    def __iter__(self):
        return iter([{"n": 0}, {"n": 1}])


def _w(path):
    return float(torch.load(path, weights_only=False)["agent"]["actor.w"][0])


def test_validate_hook_ranks_snapshots(tmp_path):
    scores = {1: 5.0, 2: 3.0, 3: 4.0, 4: 6.0, 5: 2.5, 6: 9.0}  # by epochs done
    calls = []

    def validate(agent, epochs_done):
        calls.append((epochs_done, float(agent.w[0])))
        return {"select": scores[epochs_done], "gripper_acc": 0.5}

    loop = ControllerTrainLoop(_StubAgent(), _StubReplay(), str(tmp_path), num_train_epochs=4, checkpoint_every=1, num_checkpoints=1, validate=validate)
    loop.train()
    d = loop.ckpt_dir
    assert calls == [(1, 2.0), (2, 4.0), (3, 6.0), (4, 8.0)]  # right after each snapshot, on the weights it holds
    lines = [json.loads(l) for l in open(os.path.join(d, "validation.jsonl"))]
    assert [l["_epoch"] for l in lines] == [1, 2, 3, 4] and [l["_num_iters"] for l in lines] == [2, 4, 6, 8] and [l["select"] for l in lines] == [5.0, 3.0, 4.0, 6.0]
    assert all(l["gripper_acc"] == 0.5 for l in lines)
    # num_checkpoints = 1: one numbered file survives beside latest.pt -- and best.pt, which is never pruned
    assert sorted(n for n in os.listdir(d) if n.endswith(".pt")) == ["2.pt", "best.pt", "latest.pt"]
    assert _w(os.path.join(d, "best.pt")) == 4.0 and loop.best_select == 3.0  # the snapshot of epochs_done = 2
    # resume: the minimum so far is read back, so 4.0-like scores do not displace it, 2.5 does
    loop2 = ControllerTrainLoop(_StubAgent(), _StubReplay(), str(tmp_path), num_train_epochs=6, checkpoint_every=1, num_checkpoints=1, validate=validate)
    assert loop2.best_select == 3.0 and loop2._epoch == 4
    loop2.train()
    assert len(open(os.path.join(d, "validation.jsonl")).readlines()) == 6
    assert _w(os.path.join(d, "best.pt")) == 10.0 and loop2.best_select == 2.5
    assert sorted(n for n in os.listdir(d) if n.endswith(".pt")) == ["4.pt", "best.pt", "latest.pt"]
    # a dict without `select` is logged and ranks nothing
    loop3 = ControllerTrainLoop(_StubAgent(), _StubReplay(), str(tmp_path / "plain"), num_train_epochs=2, checkpoint_every=1, validate=lambda a, e: {"x": 1.0})
    loop3.train()
    assert not os.path.exists(os.path.join(loop3.ckpt_dir, "best.pt")) and len(open(os.path.join(loop3.ckpt_dir, "validation.jsonl")).readlines()) == 2


def test_without_validate_nothing_changes(tmp_path):
    loop = ControllerTrainLoop(_StubAgent(), _StubReplay(), str(tmp_path), num_train_epochs=21, checkpoint_every=10, num_checkpoints=3)
    loop.train()
    assert sorted(os.listdir(loop.ckpt_dir)) == ["0.pt", "10.pt", "action_stats.json", "latest.pt", "proprio_stats.json"]
    ck = torch.load(os.path.join(loop.ckpt_dir, "latest.pt"), weights_only=False)
    assert set(ck) == {"cfg", "_epoch", "_num_iters", "agent"} and ck["_epoch"] == 21 and ck["_num_iters"] == 42
