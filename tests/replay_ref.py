"""Numpy restatement of the ACT replay, written from the reference's text and the kernel's contract in include/genima_hip.h, not from
genima_amd/replay.py: the demo -> transition rules, the statistics formulas, the frame / action index rules and the batch layouts.

  * controller/env/rlbench_utils.py:66-75   action = next observation's joint_position_action[:-1] (or joint_positions) ++ gripper one-hot
  * controller/env/rlbench_utils.py:119-137 low_dim_state = [gripper_open] ++ joint_positions
  * controller/env/rlbench_utils.py:236-250 an episode of L observations is stored as L - 1 transitions
  * controller/env/rlbench.py:373-376       proprioception statistics: the actions', gripper constants 1/2, 1/6, 1, 0 in front
  * controller/utils/dataloader.py:42-45    the frame stack ends at the transition and clips at the episode's first observation
"""
import numpy as np


def actions_of(joint_positions, gripper_open, joint_position_action=None):
    L = len(gripper_open)
    out = []
    for t in range(L - 1):
        arm = joint_position_action[t + 1][:-1] if joint_position_action is not None else joint_positions[t + 1]
        out.append(np.concatenate([arm, [1.0 if gripper_open[t + 1] == 1 else 0.0]]).astype(np.float32))
    return np.stack(out)


def low_dim_state_of(joint_positions, gripper_open):
    return np.stack([np.concatenate([[gripper_open[t]], joint_positions[t]]).astype(np.float32) for t in range(len(gripper_open))])


def action_stats_of(actions):
    a = np.asarray(actions, np.float64)
    return {"mean": np.mean(a, 0), "std": np.std(a, 0), "max": np.max(a, 0), "min": np.min(a, 0)}


def proprio_stats_of(actions):
    a = np.asarray(actions, np.float64)
    return {"mean": np.hstack([1 / 2, np.mean(a, 0)[:-1]]), "std": np.hstack([1 / 6, np.std(a, 0)[:-1]]),
            "max": np.hstack([1, np.max(a, 0)[:-1]]), "min": np.hstack([0, np.min(a, 0)[:-1]])}


def tables(lengths, obs_counts=None):
    """Episode lengths (observations) -> per-transition int32 tables: obs_index, first_obs, last_tr, episode.  ``obs_counts``: observations
    stored per episode (L, or L - 1 when the last frame is missing); default L."""
    obs_counts = list(lengths) if obs_counts is None else list(obs_counts)
    obs_index, first_obs, last_tr, episode = [], [], [], []
    o0 = t0 = 0
    for e, L in enumerate(lengths):
        for t in range(L - 1):
            obs_index.append(o0 + t)
            first_obs.append(o0)
            last_tr.append(t0 + L - 2)
            episode.append(e)
        o0 += obs_counts[e]
        t0 += L - 1
    return tuple(np.asarray(x, np.int32) for x in (obs_index, first_obs, last_tr, episode))


def frame_indices(n, fs, obs_index, first_obs):
    """The observations of the frame stack of transition n, oldest first."""
    return [max(int(obs_index[n]) - (fs - 1) + k, int(first_obs[n])) for k in range(fs)]


def action_rows(n, T, last_tr):
    """The action rows of the chunk of transition n."""
    return [min(n + j, int(last_tr[n])) for j in range(T)]


def u8_to_f16(frames_u8):
    """gn_image_u8_to_f16 with mul 1, add 0: (float)v / 255.0f in f32 (correctly rounded division), rounded to f16; channels 3..7 zero."""
    v = (np.asarray(frames_u8, np.float32) / np.float32(255.0)).astype(np.float16)
    out = np.zeros(v.shape[:-1] + (8,), np.float16)
    out[..., :3] = v
    return out


def gather(idx, frames, qpos, action, obs_index, first_obs, last_tr, V, fs, T):
    """frames uint8 [N_obs * V, H, W, 3] (observation-major, camera-minor), qpos f32 [N_obs, S], action f32 [N, A]; idx clamped into [0, N)
    -> (images f16 [B, V * fs, H, W, 8], images_u8 [B, V * fs, H, W, 3], low_dim_state f32 [B, fs, S], action f32 [B, T, A])."""
    N = len(obs_index)
    img8, low, act = [], [], []
    for n in idx:
        n = min(max(int(n), 0), N - 1)
        obs = frame_indices(n, fs, obs_index, first_obs)
        img8.append(np.stack([frames[o * V + v] for v in range(V) for o in obs]))  # slot v * fs + k
        low.append(np.stack([qpos[o] for o in obs]))
        act.append(np.stack([action[r] for r in action_rows(n, T, last_tr)]))
    img8 = np.stack(img8)
    return u8_to_f16(img8), img8, np.stack(low).astype(np.float32), np.stack(act).astype(np.float32)
