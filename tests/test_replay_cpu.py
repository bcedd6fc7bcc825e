"""-m "not gpu": the host side of the ACT controller training from a demo tree -- demo -> transitions, statistics and their JSON files, the
normalisation transforms, the epoch sampler, the loop's checkpoint logic (stub agent, stub replay) and the index rules of replay_ref."""
import json
import os

import numpy as np
import pytest
import torch

import replay_ref as R
from genima_amd import replay as P
from genima_amd.act_train_loop import ControllerTrainLoop


def _demo4():
    jp = np.array([[0.0, 1.0], [0.5, 1.5], [1.0, 3.0], [2.0, 2.0]])
    go = np.array([1.0, 1.0, 0.5, 0.0])
    return {"joint_positions": jp, "gripper_open": go}


def test_transitions_of_a_hand_written_demo():
    d = _demo4()
    a, s = P.demo_actions(d), P.demo_low_dim_state(d)
    assert a.dtype == s.dtype == np.float32 and a.shape == (3, 3) and s.shape == (4, 3)
    assert np.array_equal(a, np.array([[0.5, 1.5, 1.0], [1.0, 3.0, 0.0], [2.0, 2.0, 0.0]], np.float32))
    assert np.array_equal(s, np.array([[1.0, 0.0, 1.0], [1.0, 0.5, 1.5], [0.5, 1.0, 3.0], [0.0, 2.0, 2.0]], np.float32))
    assert np.array_equal(a, R.actions_of(d["joint_positions"], d["gripper_open"]))
    assert np.array_equal(s, R.low_dim_state_of(d["joint_positions"], d["gripper_open"]))


def test_joint_position_action_is_preferred():
    d = _demo4()
    d["joint_position_action"] = np.array([[9.0, 9.0, 1.0], [7.0, 8.0, 1.0], [5.0, 6.0, 1.0], [3.0, 4.0, 1.0]])
    a = P.demo_actions(d)
    assert np.array_equal(a[:, :2], np.array([[7.0, 8.0], [5.0, 6.0], [3.0, 4.0]], np.float32))  # the NEXT observation's, without its last element
    assert np.array_equal(a[:, 2], np.array([1.0, 0.0, 0.0], np.float32))  # the gripper still comes from gripper_open
    assert np.array_equal(a, R.actions_of(d["joint_positions"], d["gripper_open"], d["joint_position_action"]))


def test_gripper_one_hot():
    d = {"joint_positions": np.zeros((4, 1)), "gripper_open": np.array([0.0, 1.0, 0.5, 0.0])}
    assert P.demo_actions(d)[:, -1].tolist() == [1.0, 0.0, 0.0]


def test_demo_npz_round_trip(tmp_path):
    d, frames = P.synthetic_demo(5, seed=3, size=8, cameras=("front",))
    P.write_episode(str(tmp_path / "ep0"), d, frames, "open the box")
    with np.load(tmp_path / "ep0" / "demo.npz") as z:
        assert sorted(z.files) == ["gripper_open", "joint_positions"] and z["joint_positions"].dtype == np.float64
    back = P.load_demo(str(tmp_path / "ep0"))
    assert np.array_equal(back["joint_positions"], d["joint_positions"]) and np.array_equal(back["gripper_open"], d["gripper_open"])
    assert sorted(os.listdir(tmp_path / "ep0" / "front_rgb")) == [f"{i}.png" for i in range(5)]
    d2, f2 = P.synthetic_demo(5, seed=3, size=8, cameras=("front",))
    assert np.array_equal(d2["joint_positions"], d["joint_positions"]) and np.array_equal(f2["front"], frames["front"])


def test_list_episodes_takes_the_first_demos_in_natural_order(tmp_path):
    for task, n in (("open_box", 12), ("close_jar", 2)):
        for i in range(n):
            os.makedirs(tmp_path / task / "variation0" / "episodes" / f"episode{i}")
    got = P.list_episodes(str(tmp_path), ["open_box", "close_jar"], 11)
    assert [os.path.basename(p) for p in got] == [f"episode{i}" for i in range(11)] + ["episode0", "episode1"]  # episode10 after episode9
    assert got[0] == os.path.join(str(tmp_path), "open_box", "variation0", "episodes", "episode0")


def _demos():
    return [P.synthetic_demo(L, seed=s, size=4, cameras=("front",))[0] for L, s in ((6, 1), (9, 2))]


def test_stats_match_direct_numpy_calls():
    demos = _demos()
    acts = np.concatenate([R.actions_of(d["joint_positions"], d["gripper_open"]) for d in demos]).astype(np.float64)
    a, p = P.action_stats(demos), P.proprio_stats(demos)
    assert np.array_equal(a["mean"], np.mean(acts, 0)) and np.array_equal(a["std"], np.std(acts, 0))
    assert np.array_equal(a["max"], np.max(acts, 0)) and np.array_equal(a["min"], np.min(acts, 0))
    assert p["mean"][0] == 1 / 2 and p["std"][0] == 1 / 6 and p["max"][0] == 1 and p["min"][0] == 0
    assert np.array_equal(p["mean"][1:], np.mean(acts, 0)[:-1]) and np.array_equal(p["std"][1:], np.std(acts, 0)[:-1])
    assert np.array_equal(p["max"][1:], np.max(acts, 0)[:-1]) and np.array_equal(p["min"][1:], np.min(acts, 0)[:-1])
    for k in ("mean", "std", "max", "min"):
        assert np.array_equal(a[k], R.action_stats_of(acts)[k]) and np.array_equal(p[k], R.proprio_stats_of(acts)[k])


def test_stats_json_round_trip(tmp_path):
    demos = _demos()
    a, p = P.action_stats(demos), P.proprio_stats(demos)
    P.save_stats(str(tmp_path), a, p)
    assert sorted(os.listdir(tmp_path)) == ["action_stats.json", "proprio_stats.json"]
    for name, st in (("action_stats.json", a), ("proprio_stats.json", p)):
        with open(tmp_path / name) as f:
            js = json.load(f)
        assert sorted(js) == ["mean", "std"] and js["mean"] == st["mean"].tolist() and js["std"] == st["std"].tolist()
    a2, p2 = P.load_stats(str(tmp_path))
    assert np.array_equal(a2["mean"], a["mean"]) and np.array_equal(a2["std"], a["std"])
    assert np.array_equal(p2["mean"], p["mean"]) and np.array_equal(p2["std"], p["std"])


def test_transforms_invert_and_leave_the_gripper_alone():
    demos = _demos()
    a, p = P.action_stats(demos), P.proprio_stats(demos)
    acts = P.demo_actions(demos[0]).astype(np.float64)
    acts[:, -1] = np.linspace(0.1, 0.9, len(acts))  # a gripper value that any arithmetic would disturb
    n = P.action_to_norm(acts, a["mean"], a["std"])
    assert np.array_equal(n[:, :-1], (acts[:, :-1] - a["mean"][:-1]) / a["std"][:-1])
    back = P.action_from_norm(n, a["mean"], a["std"])
    # one subtract, divide, multiply, add in f64: a few ulps of the larger of |a| and |mean|
    bound = 4 * np.finfo(np.float64).eps * (np.abs(acts[:, :-1]) + np.abs(a["mean"][:-1]))
    assert np.all(np.abs(back[:, :-1] - acts[:, :-1]) <= bound)
    assert np.array_equal(n[:, -1], acts[:, -1]) and np.array_equal(back[:, -1], acts[:, -1])
    s = P.demo_low_dim_state(demos[0]).astype(np.float64)
    s[:, 0] = 0.3
    sn = P.proprio_to_norm(s, p["mean"], p["std"])
    assert np.array_equal(sn[:, 0], s[:, 0]) and np.array_equal(sn[:, 1:], (s[:, 1:] - p["mean"][1:]) / (p["std"][1:] + 1e-10))
    assert np.array_equal(acts[:, -1], np.linspace(0.1, 0.9, len(acts)))  # the transforms work on copies


def test_zero_std_is_refused_by_name():
    d = _demo4()
    d["joint_positions"][:, 1] = 2.0
    with pytest.raises(ValueError, match="joint 1"):
        P.action_stats([d])


def test_sampler_per_batch_restates_the_reference():
    g, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    s = P.EpochSampler(10, 4, generator=g)
    for _ in range(2):  # two epochs; the draw that precedes StopIteration consumes the generator too
        got = list(iter(s))
        assert len(got) == 2
        want = [torch.randperm(10, generator=g2)[k * 4: k * 4 + 4] for k in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        torch.randperm(10, generator=g2)
    it = iter(s)
    next(it), next(it)
    with pytest.raises(StopIteration):
        next(it)
    assert len(list(iter(s))) == 2  # a fresh epoch on iter()


def test_sampler_per_epoch_visits_distinct_transitions():
    s = P.EpochSampler(10, 4, shuffle="per_epoch", generator=torch.Generator().manual_seed(3))
    got = torch.cat(list(iter(s)))
    assert got.numel() == 8 and len(set(got.tolist())) == 8
    again = torch.cat(list(iter(s)))
    assert again.numel() == 8 and len(set(again.tolist())) == 8 and not torch.equal(again, got)
    with pytest.raises(ValueError):
        P.EpochSampler(10, 4, shuffle="never")


def test_sampler_uses_the_global_generator_by_default():
    torch.manual_seed(5)
    got = next(iter(P.EpochSampler(10, 4)))
    torch.manual_seed(5)
    assert torch.equal(got, torch.randperm(10)[:4])


class _StubAgent:
    def __init__(self):
        self.w = torch.zeros(3)
        self.steps = []

    def state_dict(self):
        return {"actor.w": self.w.clone(), "clip_model.x": torch.ones(1)}

    def load_state_dict(self, sd, strict=False):
        self.w = sd["actor.w"].clone()

    def update_device(self, batch, step=0):
        self.steps.append(step)
        self.w += 1
        return {"actor_loss": float(self.w[0])}


class _StubReplay:
    action_stats = {"mean": np.zeros(3), "std": np.ones(3)}
    proprio_stats = {"mean": np.zeros(3), "std": np.ones(3)}

    def __iter__(self):
        return iter([{"n": 0}, {"n": 1}])


def _names(loop):
    return sorted(n for n in os.listdir(loop.ckpt_dir) if n.endswith(".pt"))


def test_loop_rotation_pruning_payload_and_resume(tmp_path):
    agent, logged = _StubAgent(), []
    loop = ControllerTrainLoop(agent, _StubReplay(), str(tmp_path), num_train_epochs=21, checkpoint_every=10, num_checkpoints=3,
                               log=lambda m, i: logged.append(i))
    loop.train()
    assert loop.ckpt_dir == os.path.join(str(tmp_path), "snapshots", "genima_controller")
    assert _names(loop) == ["0.pt", "10.pt", "latest.pt"]  # epochs 0, 10 and 20 wrote; 10 and 20 renamed their predecessor
    assert agent.steps == list(range(42)) == logged
    assert {"action_stats.json", "proprio_stats.json"} <= set(os.listdir(loop.ckpt_dir))
    ck = torch.load(os.path.join(loop.ckpt_dir, "latest.pt"), weights_only=False)
    assert set(ck) == {"cfg", "_epoch", "_num_iters", "agent"} and set(ck["agent"]) == {"actor.w"}
    assert ck["_epoch"] == 21 and ck["_num_iters"] == 42 and float(ck["agent"]["actor.w"][0]) == 42.0
    assert float(torch.load(os.path.join(loop.ckpt_dir, "10.pt"), weights_only=False)["agent"]["actor.w"][0]) == 22.0  # written after epoch 10
    # resume: a fresh agent takes the weights, the counters continue
    agent2 = _StubAgent()
    loop2 = ControllerTrainLoop(agent2, _StubReplay(), str(tmp_path), num_train_epochs=61, checkpoint_every=10, num_checkpoints=3)
    assert loop2._epoch == 21 and loop2._num_iters == 42 and float(agent2.w[0]) == 42.0
    loop2.train()
    assert agent2.steps == list(range(42, 122))
    assert _names(loop2) == ["30.pt", "40.pt", "50.pt", "latest.pt"]  # pruned to three, oldest first in natural order
    assert torch.load(os.path.join(loop2.ckpt_dir, "latest.pt"), weights_only=False)["_epoch"] == 61


def test_frame_and_action_indices_stay_inside_their_episode():
    lengths, fs, T = (3, 6), 3, 4
    obs_index, first_obs, last_tr, episode = R.tables(lengths)
    assert len(obs_index) == 7 and episode.tolist() == [0, 0, 1, 1, 1, 1, 1]
    obs_range = {0: range(0, 3), 1: range(3, 9)}
    tr_range = {0: range(0, 2), 1: range(2, 7)}
    for n in range(7):
        e = int(episode[n])
        assert all(o in obs_range[e] for o in R.frame_indices(n, fs, obs_index, first_obs))
        assert all(r in tr_range[e] for r in R.action_rows(n, T, last_tr))
    assert R.frame_indices(2, fs, obs_index, first_obs) == [3, 3, 3]  # first transition of episode 2: its first observation repeated
    assert R.action_rows(2, T, last_tr) == [2, 3, 4, 5]
    assert R.frame_indices(1, fs, obs_index, first_obs) == [0, 0, 1]  # last transition of episode 1
    assert R.action_rows(1, T, last_tr) == [1, 1, 1, 1]  # its chunk repeats the episode's last action
    assert R.frame_indices(6, fs, obs_index, first_obs) == [5, 6, 7] and R.action_rows(6, T, last_tr) == [6, 6, 6, 6]
    # a tree whose last frame per episode is missing (render_episode writes L - 1) stores L - 1 observations per episode
    oi, fo, _, _ = R.tables(lengths, obs_counts=(2, 5))
    assert oi.tolist() == [0, 1, 2, 3, 4, 5, 6] and fo.tolist() == [0, 0, 2, 2, 2, 2, 2]
