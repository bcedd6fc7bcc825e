"""Step 4 of the reference's workflow -- train the ACT controller -- from a demo tree, without RoboBase or RLBench: the demo format, the
action / proprioception statistics, and a replay whose frames, proprioception and actions stay on the device for the whole run.

Reference: ``controller/env/rlbench_utils.py:50-81`` (the action linking two observations, gripper as one-hot), ``:119-137`` (``low_dim_state``
= ``[gripper_open] ++ joint_positions``), ``:220-254`` (L observations -> L - 1 transitions), ``controller/env/rlbench.py:353-383`` (proprioception
statistics made from the ACTIONS, gripper constants hard-coded), ``controller/env/wrappers/action_normalization_wrapper.py`` /
``proprio_norm_wrapper.py`` (the transforms and the two JSON files) and ``controller/utils/dataloader.py:75-97`` (the epoch sampler).

Demo tree: an episode directory holds ``<camera>_rgb/<ts>.png`` (as ``render.render_episode`` and the reference's renderer write it) and a
plain-array ``demo.npz`` with ``joint_positions`` f64 [L, J], ``gripper_open`` f64 [L] and optionally ``joint_position_action`` f64
[L, J + 1]; an optional ``description.txt`` carries the task string in its first line.  A transition t < L - 1 reads observation t, so
the last observation's frame may be missing (``render_episode`` writes L - 1 frames).

Render mode (``DeviceReplay(..., render=RenderTargets(cfg, textures))``): the controller's own training distribution is the reference's
``rlbench_data_rnd_bg`` -- the joint-target spheres alpha-blended over a random texture, no scene (``render/render_data.py:296-311``).  Such a
frame depends on nothing but the trajectory, a texture and a blend factor, so the batch is DRAWN by ``gn_replay_render`` from per-observation
view tables and a texture bank on the device: an episode is then ``demo.npz`` + ``traj.npz`` (``render.save_traj``), no camera PNG is read,
and every frame of every batch gets a fresh texture and blend (``draw_backgrounds`` states the picks).

Two things here are NOT pinned to reference text, because ``_compute_action_stats`` and the sequence sampling live in RoboBase: the action
statistics (taken here as mean / population std / max / min over axis 0 of all transitions' actions) and the end-of-episode rule of the
action chunk (the chunk repeats the episode's last action and never crosses into the next episode).  Statistics are computed in numpy f64
from the f32 actions (the reference's ``np.mean`` of an f32 stack accumulates in f32).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .data import _natural_key, resize_center_crop_u8

DEFAULT_CAMERAS = ("left_shoulder", "right_shoulder", "front", "wrist")  # RoboBase's camera enumeration (rlbench_utils.py:107-113): the view order a checkpoint was trained with
ACTION_STATS_JSON, PROPRIO_STATS_JSON = "action_stats.json", "proprio_stats.json"


# ---------------------------------------------------------------------------------------------------------------- the demo format
def save_demo(path: str, demo: Dict[str, np.ndarray]):
    """Write ``demo.npz``: exactly ``joint_positions``, ``gripper_open`` and, when the demo has it, ``joint_position_action``."""
    arrays = {"joint_positions": np.asarray(demo["joint_positions"], np.float64), "gripper_open": np.asarray(demo["gripper_open"], np.float64)}
    if demo.get("joint_position_action") is not None:
        arrays["joint_position_action"] = np.asarray(demo["joint_position_action"], np.float64)
    np.savez(path, **arrays)


def load_demo(path: str) -> Dict[str, np.ndarray]:
    """``demo.npz`` (or the episode directory that holds it) -> the demo dict, checked."""
    if os.path.isdir(path):
        path = os.path.join(path, "demo.npz")
    with np.load(path) as z:
        demo = {k: np.asarray(z[k], np.float64) for k in z.files}
    return check_demo(demo)


def check_demo(demo: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    jp, go = np.asarray(demo["joint_positions"], np.float64), np.asarray(demo["gripper_open"], np.float64)
    if jp.ndim != 2 or go.shape != (jp.shape[0],) or jp.shape[0] < 2:
        raise ValueError(f"demo: joint_positions [L >= 2, J] and gripper_open [L] expected, got {jp.shape} and {go.shape}")
    out = {"joint_positions": jp, "gripper_open": go}
    jpa = demo.get("joint_position_action")
    if jpa is not None:
        jpa = np.asarray(jpa, np.float64)
        if jpa.shape != (jp.shape[0], jp.shape[1] + 1):
            raise ValueError(f"demo: joint_position_action must be [L, J + 1] = {(jp.shape[0], jp.shape[1] + 1)}, got {jpa.shape}")
        out["joint_position_action"] = jpa
    return out


def demo_from_low_dim_obs(pkl_path: str) -> Dict[str, np.ndarray]:
    """RLBench's ``low_dim_obs.pkl`` (a pickled ``Demo`` of ``Observation``s) -> the demo dict ``save_demo`` writes.  Unpickling imports
    ``rlbench``, which must be installed for this call and for nothing else here (as ``render.traj_from_low_dim_obs``); it is not installed
    where this package is tested, so this function is NOT covered by the test suite."""
    import pickle

    with open(pkl_path, "rb") as f:
        obs = list(pickle.load(f))
    demo = {"joint_positions": np.array([o.joint_positions for o in obs], dtype=np.float64),
            "gripper_open": np.array([o.gripper_open for o in obs], dtype=np.float64)}
    if all("joint_position_action" in o.misc for o in obs):
        demo["joint_position_action"] = np.array([o.misc["joint_position_action"] for o in obs], dtype=np.float64)
    return check_demo(demo)


def synthetic_demo(L: int, seed: int = 0, size: int = 64, cameras: Sequence[str] = DEFAULT_CAMERAS, joints: int = 7):
    """A made-up demo for tests and benchmarks -> ``(demo, frames)``: smooth joint paths with noise, a gripper that closes half-way, and
    ``frames = {camera: uint8 [L, size, size, 3]}`` of random bytes.  Deterministic in ``seed``."""
    rng = np.random.RandomState(seed)
    t = np.linspace(0.0, 1.0, L)[:, None]
    jp = np.sin(2.0 * np.pi * (t * rng.uniform(0.5, 1.5, joints) + rng.uniform(0, 1, joints))) * rng.uniform(0.3, 1.2, joints) + 0.01 * rng.randn(L, joints)
    go = (np.arange(L) < (L + 1) // 2).astype(np.float64)
    frames = {c: rng.randint(0, 256, (L, size, size, 3)).astype(np.uint8) for c in cameras}
    return {"joint_positions": jp.astype(np.float64), "gripper_open": go}, frames


def write_episode(ep_dir: str, demo: Dict[str, np.ndarray], frames: Dict[str, np.ndarray], description: Optional[str] = None):
    """Write one episode of the demo tree: ``<camera>_rgb/<ts>.png``, ``demo.npz`` and, with ``description``, ``description.txt``."""
    from PIL import Image

    for cam, fr in frames.items():
        d = os.path.join(ep_dir, f"{cam}_rgb")
        os.makedirs(d, exist_ok=True)
        for ts in range(len(fr)):
            Image.fromarray(np.asarray(fr[ts], np.uint8)).save(os.path.join(d, f"{ts}.png"))
    os.makedirs(ep_dir, exist_ok=True)
    save_demo(os.path.join(ep_dir, "demo.npz"), demo)
    if description is not None:
        with open(os.path.join(ep_dir, "description.txt"), "w") as f:
            f.write(description + "\n")


def demo_actions(demo: Dict[str, np.ndarray]) -> np.ndarray:
    """f32 [L - 1, J + 1]: ``action[t]`` links observation t to t + 1 (``observations_to_action_with_onehot_gripper``): the NEXT
    observation's ``joint_position_action[:-1]`` when the demo has it, else its ``joint_positions``, then 1.0 where its ``gripper_open == 1``
    and 0.0 otherwise."""
    demo = check_demo(demo)
    jpa = demo.get("joint_position_action")
    arm = jpa[1:, :-1] if jpa is not None else demo["joint_positions"][1:]
    grip = np.where(demo["gripper_open"][1:] == 1, 1.0, 0.0)
    return np.concatenate([arm, grip[:, None]], axis=1).astype(np.float32)


def demo_low_dim_state(demo: Dict[str, np.ndarray]) -> np.ndarray:
    """f32 [L, 1 + J]: ``[gripper_open[t]] ++ joint_positions[t]`` (``Observation.get_low_dim_data`` with these two fields on)."""
    demo = check_demo(demo)
    return np.concatenate([demo["gripper_open"][:, None], demo["joint_positions"]], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ statistics and transforms
def _all_actions(demos) -> np.ndarray:
    return np.concatenate([demo_actions(d) for d in demos], axis=0).astype(np.float64)


def action_stats(demos) -> Dict[str, np.ndarray]:
    """mean / std (population) / max / min over axis 0 of every transition's action, f64 [A].  A joint whose std is 0 is refused: the
    reference would divide by zero when it normalises."""
    a = _all_actions(demos)
    st = {"mean": np.mean(a, 0), "std": np.std(a, 0), "max": np.max(a, 0), "min": np.min(a, 0)}
    for j in range(a.shape[1] - 1):
        if st["std"][j] == 0:
            raise ValueError(f"action_stats: joint {j} never moves in the demos (action std 0): its actions cannot be normalised")
    return st


def proprio_stats(demos) -> Dict[str, np.ndarray]:
    """``_compute_proprio_stats`` (controller/env/rlbench.py:353-383), literally: the statistics of the ACTIONS with the gripper element moved
    to the front, where ``low_dim_state`` has it, and hard-coded: mean 1/2, std 1/6, max 1, min 0."""
    a = _all_actions(demos)
    return {"mean": np.hstack([1 / 2, np.mean(a, 0)[:-1]]), "std": np.hstack([1 / 6, np.std(a, 0)[:-1]]),
            "max": np.hstack([1, np.max(a, 0)[:-1]]), "min": np.hstack([0, np.min(a, 0)[:-1]])}


def action_to_norm(action: np.ndarray, mean, std) -> np.ndarray:
    """``ActionNormalization.transform_to_norm`` over the last axis, on a copy: the arm elements standardised, the gripper untouched."""
    a = np.array(action, copy=True)
    a[..., :-1] = (a[..., :-1] - np.asarray(mean)[:-1]) / np.asarray(std)[:-1]
    return a


def action_from_norm(action: np.ndarray, mean, std) -> np.ndarray:
    """``ActionNormalization.transform_from_norm``: the inverse."""
    a = np.array(action, copy=True)
    a[..., :-1] = a[..., :-1] * np.asarray(std)[:-1] + np.asarray(mean)[:-1]
    return a


def proprio_to_norm(state: np.ndarray, mean, std) -> np.ndarray:
    """``ProprioNorm.transform_to_norm``: elements 1.. standardised with epsilon 1e-10 on the std, element 0 (the gripper) untouched."""
    s = np.array(state, copy=True)
    s[..., 1:] = (s[..., 1:] - np.asarray(mean)[1:]) / (np.asarray(std)[1:] + 1e-10)
    return s


def save_stats(directory: str, action: Dict[str, np.ndarray], proprio: Dict[str, np.ndarray]):
    """``action_stats.json`` / ``proprio_stats.json`` as ``{"mean": [...], "std": [...]}``: what the reference's evaluation wrappers load from
    the snapshot directory."""
    os.makedirs(directory, exist_ok=True)
    for name, st in ((ACTION_STATS_JSON, action), (PROPRIO_STATS_JSON, proprio)):
        with open(os.path.join(directory, name), "w") as f:
            json.dump({"mean": np.asarray(st["mean"]).tolist(), "std": np.asarray(st["std"]).tolist()}, f)


def load_stats(directory: str):
    """-> ``(action, proprio)``, each ``{"mean": f64 [..], "std": f64 [..]}``."""
    out = []
    for name in (ACTION_STATS_JSON, PROPRIO_STATS_JSON):
        with open(os.path.join(directory, name)) as f:
            st = json.load(f)
        out.append({"mean": np.array(st["mean"], np.float64), "std": np.array(st["std"], np.float64)})
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------- sampler
class EpochSampler:
    """The batch order of ``EpochReplayBuffer`` (controller/utils/dataloader.py:75-97).  ``per_batch`` (the reference): every batch draws a
    fresh ``torch.randperm(N)`` and takes ``[start : start + bs]`` of it, so an epoch may repeat a transition; ``per_epoch``: one permutation
    per epoch.  Either way an epoch ends when ``start + bs - 1 >= N``: floor(N / bs) batches.  Draws come from ``generator``, or from torch's
    global generator as in the reference."""

    def __init__(self, N: int, batch_size: int, shuffle: str = "per_batch", generator: Optional[torch.Generator] = None):
        if shuffle not in ("per_batch", "per_epoch"):
            raise ValueError(f"shuffle must be 'per_batch' or 'per_epoch', got {shuffle!r}")
        if N <= 0 or batch_size <= 0:
            raise ValueError(f"EpochSampler: N ({N}) and batch_size ({batch_size}) must be positive")
        self.N, self.batch_size, self.shuffle, self.generator = int(N), int(batch_size), shuffle, generator
        self.batch_start, self._perm = 0, None

    def __iter__(self):
        self.batch_start, self._perm = 0, None
        return self

    def __next__(self) -> torch.Tensor:
        if self.shuffle == "per_batch":
            perm = torch.randperm(self.N, generator=self.generator)  # drawn before the end-of-epoch test, as the reference does
        else:
            if self._perm is None:
                self._perm = torch.randperm(self.N, generator=self.generator)
            perm = self._perm
        if self.batch_start + self.batch_size - 1 >= self.N:
            raise StopIteration
        idx = perm[self.batch_start: self.batch_start + self.batch_size]
        self.batch_start += self.batch_size
        return idx


# ------------------------------------------------------------------------------------------------------------- the device replay
def _episode_frames(ep, cameras):
    """-> (demo, description, frame source): ``ep`` is an episode directory or an in-memory ``(demo, frames[, description])`` tuple."""
    if isinstance(ep, (str, os.PathLike)):
        ep = os.fspath(ep)
        demo, desc = load_demo(ep), ""
        p = os.path.join(ep, "description.txt")
        if os.path.exists(p):
            with open(p) as f:
                desc = f.readline().rstrip("\n")
        files = {}
        for cam in cameras:
            d = os.path.join(ep, f"{cam}_rgb")
            files[cam] = [os.path.join(d, n) for n in sorted((n for n in os.listdir(d) if n.endswith(".png")), key=_natural_key)]
        return demo, desc, files
    demo, frames = check_demo(ep[0]), ep[1]
    return demo, (ep[2] if len(ep) > 2 else ""), {cam: frames[cam] for cam in cameras}


def _read_frame(src, size: Optional[int]) -> np.ndarray:
    if isinstance(src, str):
        from PIL import Image

        with open(src, "rb") as f:
            raw = f.read()
        if size is not None:
            return resize_center_crop_u8(raw, size)
        import io

        return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(src, dtype=np.uint8)


def list_episodes(dataset_root: str, tasks: Sequence[str], demos: int, variation: int = 0) -> List[str]:
    """The first ``demos`` episode directories (natural order) of every task: ``<root>/<task>/variation<k>/episodes/<episode>``."""
    out = []
    for task in tasks:
        eps = os.path.join(dataset_root, task, f"variation{variation}", "episodes")
        names = sorted((n for n in os.listdir(eps) if os.path.isdir(os.path.join(eps, n))), key=_natural_key)
        out += [os.path.join(eps, n) for n in names[:demos]]
    return out


# ------------------------------------------------------------------------------------------------------------------ render mode
@dataclass
class RenderTargets:
    """What ``DeviceReplay(render=...)`` draws its frames from.  ``cfg``: a ``render.RenderConfig`` (image size, samples, sphere textures,
    horizon window, per-camera joints); ``textures``: a directory of background images or a uint8 [NB, H, W, 3] array; ``seed``: 64 bits
    of the background draws; ``alpha_blend``: the lower end of the blend factor (default: ``cfg.alpha_blend``)."""
    cfg: Any
    textures: Any
    seed: int = 0
    alpha_blend: Optional[float] = None

    def __post_init__(self):
        if self.alpha_blend is None:
            self.alpha_blend = float(self.cfg.alpha_blend)
        if not 0.0 <= float(self.alpha_blend) <= 1.0:
            raise ValueError(f"RenderTargets: alpha_blend must lie in [0, 1], got {self.alpha_blend}")


def load_texture_bank(textures, H: int, W: int) -> np.ndarray:
    """-> uint8 [NB, H, W, 3].  A directory: every file in natural-sorted order (so a layer index names a file), loaded as the reference
    does per frame (render_data.py:299-301, and ``render.render_episode``): ``Image.open(f).resize((W, H))``, then ``.convert("RGB")``.
    An array is checked and taken as it is."""
    if isinstance(textures, (str, os.PathLike)):
        from PIL import Image

        d = os.fspath(textures)
        names = sorted((n for n in os.listdir(d) if os.path.isfile(os.path.join(d, n))), key=_natural_key)
        if not names:
            raise ValueError(f"load_texture_bank: no texture files in {d}")
        return np.ascontiguousarray(np.stack([np.asarray(Image.open(os.path.join(d, n)).resize((W, H)).convert("RGB"), dtype=np.uint8) for n in names]))
    bank = np.asarray(textures)
    if bank.dtype != np.uint8 or bank.ndim != 4 or bank.shape[0] < 1 or tuple(bank.shape[1:]) != (H, W, 3):
        raise ValueError(f"load_texture_bank: a uint8 [NB >= 1, {H}, {W}, 3] array expected, got {bank.dtype} {bank.shape}")
    return np.ascontiguousarray(bank)


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)  # a copy
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def draw_backgrounds(seed: int, draw: int, B: int, V: int, fs: int, NB: int, alpha: float):
    """The texture layer and blend factor of every frame of one ``gn_replay_render`` batch (include/genima_hip.h states the formula), in
    numpy on the host -> ``(layer int32 [B, V * fs], blend f64 [B, V * fs])``; frame ``[b, v * fs + k]`` is slot ``(b * V + v) * fs + k``.
    A pure function of its arguments: uint32 arithmetic that wraps, then ``blend = alpha + (1 - alpha) * (u * 2^-24)`` in f64."""
    seed = int(seed)
    lo, hi, dr = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF), np.uint32(int(draw) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        base = _mix32(np.array([lo ^ np.uint32(0x6A09E667) ^ (dr * np.uint32(0x9E3779B9))], np.uint32))[0] ^ hi
        slot = np.arange(B * V * fs, dtype=np.uint32)
        s = _mix32(base + slot * np.uint32(0x85EBCA6B))
        layer = (_mix32(s ^ np.uint32(0xC2B2AE35)).astype(np.uint64) * np.uint64(NB)) >> np.uint64(32)
        u = _mix32(s ^ np.uint32(0x27D4EB2F)) >> np.uint32(8)
    a = np.float64(alpha)
    blend = a + (np.float64(1.0) - a) * (u.astype(np.float64) * np.float64(2.0 ** -24))
    return layer.astype(np.int32).reshape(B, V * fs), blend.reshape(B, V * fs)


def _episode_traj(ep, index: int):
    """-> (demo, description, traj) of a render-mode episode: a directory holding ``demo.npz`` + ``traj.npz`` (camera PNGs are neither
    needed nor read), or an in-memory ``(demo, traj[, description])`` tuple."""
    from .render import TRAJ_KEYS, load_traj

    if isinstance(ep, (str, os.PathLike)):
        ep = os.fspath(ep)
        p = os.path.join(ep, "traj.npz")
        if not os.path.exists(p):
            raise ValueError(f"DeviceReplay: render mode needs a traj.npz (render.save_traj) in every episode; episode {index} ({ep}) has none")
        demo, desc, traj = load_demo(ep), "", load_traj(p)
        p = os.path.join(ep, "description.txt")
        if os.path.exists(p):
            with open(p) as f:
                desc = f.readline().rstrip("\n")
    else:
        demo, traj, desc = check_demo(ep[0]), ep[1], (ep[2] if len(ep) > 2 else "")
        if not all(k in traj for k in TRAJ_KEYS):
            raise ValueError(f"DeviceReplay: render mode takes (demo, traj[, description]) tuples; episode {index} lacks one of {TRAJ_KEYS}")
    L = demo["joint_positions"].shape[0]
    if len(traj["gripper_open"]) != L:
        raise ValueError(f"DeviceReplay: episode {index} has {L} observations in its demo and {len(traj['gripper_open'])} steps in its trajectory")
    return demo, desc, traj


def view_tables(trajs, cfg, cameras: Sequence[str]) -> Dict[str, np.ndarray]:
    """``gn_replay_render``'s per-observation view tables: for every step ``ts`` of every trajectory, ``render.pack_views(render.pack_step(
    traj, cfg, ts, cameras))``, concatenated -- row ``obs * V + v``.  A step whose horizon window is empty (``render.window_step``: the last two of a trajectory) has
    count 0: its frame is the texture alone."""
    from .render import pack_step, pack_views

    parts = [pack_views(pack_step(traj, cfg, ts, cameras)) for traj in trajs for ts in range(len(traj["gripper_open"]))]
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in ("cams", "spheres", "tex_index", "count")}


class DeviceReplay:
    """Every frame of the given episodes and cameras, decoded once into device chunks of at most ``chunk_bytes``, beside persistent device
    tables: ``frame_ptr`` int64 [N_obs * V], ``qpos`` f32 [N_obs, S] and ``action`` f32 [N, A] (both normalised on the host at load, so the
    device path is a pure gather), ``lang_tokens`` int32 [N_ep, 77] (with a ``tokenizer``) and per transition ``obs_index``, ``first_obs``,
    ``last_tr``, ``episode`` int32 [N].  ``sample(indices)`` assembles a batch with ONE ``gn_replay_gather`` launch and a B x 4-byte index
    upload; ``host_batch(indices)`` is the same sample as the RoboBase-shaped numpy dict ``GenimaACT.update`` takes.  Iterating yields
    ``sample`` batches in ``EpochSampler``'s order.

    ``episodes``: episode directories, or in-memory ``(demo, {camera: uint8 [n, H, W, 3]}[, description])`` tuples.  An episode of L
    observations needs L or L - 1 frames per camera.  ``image_size``: resize + centre-crop PNGs to it (None: the files' own size).
    ``tokenizer``: a ``tokenizer.CLIPTokenizer`` (its ``tokenize``) or any callable ``[str] -> int [1, 77]``.  ``stats``:
    ``(action_stats, proprio_stats)`` to normalise with; by default they are computed from these episodes.  ``capacity_bytes``: refuse, before
    anything is allocated, a set whose frames need more device memory than this.

    ``render``: a ``RenderTargets`` turns on render mode.  Episodes are then directories holding ``demo.npz`` + ``traj.npz`` or
    ``(demo, traj[, description])`` tuples; instead of frames the device holds the view tables of every observation (``view_tables``), the
    sphere atlas and the texture bank (``device_bytes`` counts these three), and ``sample`` draws the batch with ONE ``gn_replay_render``
    launch.  ``H``, ``W``, ``samples`` and the atlas come from ``render.cfg``; the cameras must be among ``render.cfg.cameras``.  The
    backgrounds of a batch are picked by ``(render.seed, draw)``; ``self.draw`` counts the batches drawn so far."""

    def __init__(self, episodes, cameras: Sequence[str] = DEFAULT_CAMERAS, *, engine=None, device="cuda", frame_stack: int = 1,
                 action_sequence: int = 20, batch_size: int = 8, tokenizer=None, image_size: Optional[int] = None, chunk_bytes: int = 256 << 20,
                 capacity_bytes: Optional[int] = None, shuffle: str = "per_batch", generator: Optional[torch.Generator] = None, stats=None,
                 render: Optional[RenderTargets] = None):
        from .engine import Engine

        self.cameras, self.V = tuple(cameras), len(cameras)
        self.fs, self.T, self.batch_size = int(frame_stack), int(action_sequence), int(batch_size)
        if not episodes or self.V == 0 or self.fs < 1 or self.T < 1:
            raise ValueError("DeviceReplay: needs episodes, cameras, frame_stack >= 1 and action_sequence >= 1")
        self.render = render
        if render is not None:
            cfg = render.cfg
            missing = [c for c in self.cameras if c not in cfg.cameras]
            if missing:
                raise ValueError(f"DeviceReplay: cameras {missing} are not among the render config's {list(cfg.cameras)}")
            if image_size is not None and (int(image_size) != cfg.image_height or int(image_size) != cfg.image_width):
                raise ValueError(f"DeviceReplay: image_size = {image_size} contradicts the render config's {cfg.image_height} x {cfg.image_width} frames")
            eps = [_episode_traj(ep, i) for i, ep in enumerate(episodes)]
        else:
            eps = [_episode_frames(ep, self.cameras) for ep in episodes]
        demos = [e[0] for e in eps]
        self.action_stats, self.proprio_stats = stats if stats is not None else (action_stats(demos), proprio_stats(demos))
        # ---- host tables
        if render is not None:
            from .render import load_atlas

            n_obs = [e[0]["joint_positions"].shape[0] for e in eps]  # every observation can be drawn: the last one's window is empty
            self.H, self.W, self.samples = int(render.cfg.image_height), int(render.cfg.image_width), int(render.cfg.samples)
            self.host_views = view_tables([e[2] for e in eps], render.cfg, self.cameras)
            self.host_bank = load_texture_bank(render.textures, self.H, self.W)
            self.host_atlas = load_atlas(render.cfg.texture_dir)
            self.NB = int(self.host_bank.shape[0])
            self.device_bytes = sum(int(t.nbytes) for t in self.host_views.values()) + int(self.host_bank.nbytes) + int(self.host_atlas.nbytes)
            if capacity_bytes is not None and self.device_bytes > int(capacity_bytes):
                raise ValueError(f"DeviceReplay: the view tables, {self.NB} textures of {self.H}x{self.W} and the sphere atlas need {self.device_bytes} "
                                 f"bytes on the device, over capacity_bytes = {int(capacity_bytes)}")
        else:
            n_obs = []
            for i, (demo, _, src) in enumerate(eps):
                L = demo["joint_positions"].shape[0]
                counts = {len(src[c]) for c in self.cameras}
                if len(counts) != 1 or min(counts) < L - 1:
                    raise ValueError(f"DeviceReplay: episode {i} has {L} observations and needs {L - 1} or {L} frames per camera, found {sorted(counts)}")
                n_obs.append(min(L, min(counts)))
            first = _read_frame(eps[0][2][self.cameras[0]][0], image_size)
            self.H, self.W = int(first.shape[0]), int(first.shape[1])
            self.frame_bytes = self.H * self.W * 3
            self.frame_stride = (self.frame_bytes + 3) // 4 * 4  # frames start on the dword grid: the kernel's three-dword loads
            n_frames = sum(n_obs) * self.V
            self.frames_per_chunk = max(1, int(chunk_bytes) // self.frame_stride)
            self.device_bytes = n_frames * self.frame_stride
            if capacity_bytes is not None and self.device_bytes > int(capacity_bytes):
                raise ValueError(f"DeviceReplay: {n_frames} frames of {self.H}x{self.W} need {self.device_bytes} bytes on the device, over "
                                 f"capacity_bytes = {int(capacity_bytes)}")
        qpos, action, obs_index, first_obs, last_tr, episode = [], [], [], [], [], []
        o0 = t0 = 0
        for e, (demo, _, _) in enumerate(eps):
            L = demo["joint_positions"].shape[0]
            a = action_to_norm(demo_actions(demo).astype(np.float64), self.action_stats["mean"], self.action_stats["std"]).astype(np.float32)
            s = proprio_to_norm(demo_low_dim_state(demo).astype(np.float64), self.proprio_stats["mean"], self.proprio_stats["std"]).astype(np.float32)
            action.append(a)
            qpos.append(s[: n_obs[e]])
            obs_index += [o0 + t for t in range(L - 1)]
            first_obs += [o0] * (L - 1)
            last_tr += [t0 + L - 2] * (L - 1)
            episode += [e] * (L - 1)
            o0, t0 = o0 + n_obs[e], t0 + L - 1
        self.N, self.N_obs, self.N_ep = t0, o0, len(eps)
        self.descriptions = [e[1] for e in eps]
        self.host = {"qpos": np.concatenate(qpos), "action": np.concatenate(action), "obs_index": np.asarray(obs_index, np.int32),
                     "first_obs": np.asarray(first_obs, np.int32), "last_tr": np.asarray(last_tr, np.int32), "episode": np.asarray(episode, np.int32)}
        self.S, self.A = int(self.host["qpos"].shape[1]), int(self.host["action"].shape[1])
        if tokenizer is not None:
            fn = getattr(tokenizer, "tokenize", tokenizer)
            toks = [np.asarray(fn([d])).reshape(-1)[:77] for d in self.descriptions]
            if any(t.shape != (77,) for t in toks):
                raise ValueError("DeviceReplay: the tokenizer must give 77 tokens per description")
            self.host["lang_tokens"] = np.stack(toks).astype(np.int32)
        # ---- device: frames into chunks, then the tables
        self.E = engine if engine is not None else Engine(device)
        dev = self.E.device
        if render is not None:
            self.host_frames, self.chunks, self.frame_ptr = None, [], None
            self.cams, self.spheres, self.tex_index, self.count = (torch.from_numpy(self.host_views[k]).to(dev) for k in ("cams", "spheres", "tex_index", "count"))
            self.bank, self.atlas = torch.from_numpy(self.host_bank).to(dev), torch.from_numpy(self.host_atlas).to(dev)
            self.draw = 0  # the batches drawn so far: the default ``draw`` of the next ``sample``
        else:
            self.host_frames = np.empty((self.N_obs * self.V, self.H, self.W, 3), np.uint8)  # host_batch's source (and the tests')
            i = 0
            for e, (_, _, src) in enumerate(eps):
                for t in range(n_obs[e]):
                    for c in self.cameras:
                        fr = _read_frame(src[c][t], image_size)
                        if fr.shape != (self.H, self.W, 3):
                            raise ValueError(f"DeviceReplay: frame {t} of camera {c!r}, episode {e}, is {fr.shape}, expected {(self.H, self.W, 3)}")
                        self.host_frames[i] = fr
                        i += 1
            self.chunks, addr = [], np.empty(n_frames, np.int64)
            for c0 in range(0, n_frames, self.frames_per_chunk):
                n = min(self.frames_per_chunk, n_frames - c0)
                stage = np.zeros((n, self.frame_stride), np.uint8)
                stage[:, : self.frame_bytes] = self.host_frames[c0: c0 + n].reshape(n, self.frame_bytes)
                chunk = torch.from_numpy(stage).to(dev)
                self.chunks.append(chunk)
                addr[c0: c0 + n] = chunk.data_ptr() + np.arange(n, dtype=np.int64) * self.frame_stride
            self.frame_ptr = torch.from_numpy(addr).to(dev)
        for k in ("qpos", "action", "obs_index", "first_obs", "last_tr", "episode", "lang_tokens"):
            setattr(self, k, torch.from_numpy(self.host[k]).to(dev).contiguous() if k in self.host else None)
        self._ones = {}
        self.sampler = EpochSampler(self.N, self.batch_size, shuffle, generator)

    def __len__(self):
        return self.N

    # ---- the two routes to a batch
    def sample(self, indices, want_u8: bool = False, want_draws: bool = False, draw: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``indices``: transition indices -- host integers (checked, uploaded) or a device int32 [B] tensor -> ``{"images": f16 [B, V * fs,
        H, W, 8] on the 0..1 scale, "low_dim_state": f32 [B, fs, S], "action": f32 [B, T, A], "lang_tokens": int32 [B, 1, 77] (with a
        tokenizer), "reward": ones f32 [B]}`` (+ ``"images_u8"`` uint8 [B, V * fs, H, W, 3] with ``want_u8``), all on the device.

        Render mode: the images are drawn; ``draw`` (32 bits) picks the batch's backgrounds together with ``render.seed`` and defaults to
        the counter ``self.draw``, which then advances by one (an explicit ``draw`` leaves the counter alone); ``want_draws`` adds
        ``"bg_layer"`` int32 and ``"blend"`` f64 [B, V * fs], what ``draw_backgrounds`` states."""
        layer = blend = None
        if self.render is not None:
            if draw is None:
                draw, self.draw = self.draw, self.draw + 1
            img, img8, low, act, tok, layer, blend = self.E.replay_render(
                self.cams, self.spheres, self.tex_index, self.count, self.atlas, self.bank, self.qpos, self.action, self.obs_index, self.first_obs,
                self.last_tr, indices, self.V, self.fs, self.T, samples=self.samples, seed=self.render.seed, draw=draw,
                alpha_blend=self.render.alpha_blend, want_u8=want_u8, want_draws=want_draws, lang_tokens=self.lang_tokens,
                episode=self.episode if self.lang_tokens is not None else None)
        else:
            if want_draws or draw is not None:
                raise ValueError("DeviceReplay.sample: want_draws / draw belong to render mode (render=RenderTargets(...)); this replay gathers stored frames")
            img, img8, low, act, tok = self.E.replay_gather(self.frame_ptr, self.qpos, self.action, self.obs_index, self.first_obs, self.last_tr, indices,
                                                            (self.H, self.W), self.V, self.fs, self.T, want_u8=want_u8, lang_tokens=self.lang_tokens,
                                                            episode=self.episode if self.lang_tokens is not None else None)
        B = img.shape[0]
        if B not in self._ones:
            self._ones[B] = torch.ones(B, dtype=torch.float32, device=self.E.device)
        out = {"images": img, "low_dim_state": low, "action": act, "reward": self._ones[B]}
        if tok is not None:
            out["lang_tokens"] = tok.view(B, 1, 77)
        if img8 is not None:
            out["images_u8"] = img8
        if layer is not None:
            out["bg_layer"], out["blend"] = layer, blend
        return out

    def host_batch(self, indices) -> Dict[str, np.ndarray]:
        """The same sample as the numpy dict a RoboBase replay hands to ``GenimaACT.update``: ``<camera>_rgb`` uint8 [B, fs, 3, H, W] in camera
        order, ``low_dim_state`` f32 [B, fs, S], ``action`` f32 [B, T, A], ``lang_tokens`` int32 [B, fs, 77] (with a tokenizer), ``reward``
        f32 [B].  Assembled on the host, per batch: the route ``sample`` replaces.  Not in render mode: there are no stored frames."""
        if self.render is not None:
            raise ValueError("DeviceReplay.host_batch: this replay is in render mode -- its frames are drawn on the device by sample(), none are stored")
        idx = np.asarray(torch.as_tensor(indices).cpu()).reshape(-1).astype(np.int64)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= self.N:
            raise ValueError(f"host_batch: transition indices must lie in [0, {self.N}), got {idx.tolist()}")
        h = self.host
        k = np.arange(self.fs)
        obs = np.maximum(h["obs_index"][idx][:, None] - (self.fs - 1) + k[None], h["first_obs"][idx][:, None])  # [B, fs]
        rows = np.minimum(idx[:, None] + np.arange(self.T)[None], h["last_tr"][idx][:, None])  # [B, T]
        out = {}
        for v, cam in enumerate(self.cameras):
            out[f"{cam}_rgb"] = np.ascontiguousarray(self.host_frames[obs * self.V + v].transpose(0, 1, 4, 2, 3))
        out["low_dim_state"] = h["qpos"][obs]
        out["action"] = h["action"][rows]
        if "lang_tokens" in h:
            out["lang_tokens"] = np.repeat(h["lang_tokens"][h["episode"][idx]][:, None], self.fs, axis=1)
        out["reward"] = np.ones(len(idx), np.float32)
        return out

    # ---- the epoch iterator
    def __iter__(self):
        iter(self.sampler)
        return self

    def __next__(self) -> Dict[str, torch.Tensor]:
        return self.sample(next(self.sampler))
