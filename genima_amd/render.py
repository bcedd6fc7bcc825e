"""Joint-action rendering on the device: the spheres the reference draws with pyrender on an OpenGL context (``render/joint_marker.py``)
and the dataset loop around them (``render/render_data.py``), on one HIP kernel (``gn_render_spheres``, csrc/render.hip) -- an Instinct
node has no graphics stack, and this is the first step of the train-and-eval workflow.

* ``JointMarker`` keeps the reference's constructor and ``render_action`` so ``render_data.py`` can import ours instead
  (``from genima_amd.render import JointMarker``).
* ``render_views`` is the batched form over device tensors: every output of the kernel, no host round trip.
* ``render_episode`` reproduces ``render_demo``'s loop (render_data.py:220-323) over plain arrays and writes the PNG trees with PIL.
* ``TrajectorySource`` feeds ``data.DataLoader(render_targets=...)``: the target image is drawn from the conditioning frame into the batch.

The trajectory (``traj``) is a dict of plain arrays over the L steps of a demo and the C cameras of ``cfg.cameras``, in that order:
``intrinsics`` [L, C, 3, 3], ``extrinsics`` [L, C, 4, 4] (RLBench's camera-to-world matrices, as stored), ``gripper_matrix`` [L, 4, 4],
``gripper_open`` [L], ``joint_poses`` [L, J, 7] (xyz + xyzw quaternion).  ``save_traj`` / ``load_traj`` keep it as an ``.npz`` of
exactly these five arrays; ``traj_from_low_dim_obs`` converts RLBench's ``low_dim_obs.pkl`` (RLBench is imported by the unpickling only).

Textures: ``texture_dir`` holds the reference's five ``sphere_<colour>_stripe_texture.png`` files; this package ships none.

Unpinned against pyrender (not installable here): the 4-sample pattern, the bottom-row ``v = 0`` and the planar-uv normalisation are
readings of pyrender's source, recorded in DESIGN.md section 4.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import tiling

MAX_SPHERES = 8  # csrc/render.hip
CAM_FLOATS, SPHERE_FLOATS = 18, 16
SPHERE_TEXTURES = ("sphere_yellow_stripe_texture.png", "sphere_cyan_stripe_texture.png", "sphere_green_stripe_texture.png",
                   "sphere_red_stripe_texture.png", "sphere_purple_stripe_texture.png")  # atlas layer order
COLOR_TEXTURES = {"green": "sphere_green_stripe_texture.png", "red": "sphere_red_stripe_texture.png", "purple": "sphere_purple_stripe_texture.png"}
JOINT_COLOR_MAP = {1: "red", 3: "green", 5: "purple"}  # render_data.py:15-19
SAMPLE_OFFSETS = {1: ((0.5, 0.5),), 4: ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))}


# ---- host-side setup (joint_marker.py) ----
def flip_extrinsic(cam_extrinsic) -> np.ndarray:
    """RLBench camera-to-world -> OpenGL convention: R <- R . Rx(-180 deg) (joint_marker.py:101-118), on a copy."""
    ext = np.array(cam_extrinsic, dtype=np.float64)
    a = np.radians(-180)
    rotation_x = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ext[:3, :3] = np.dot(ext[:3, :3], rotation_x)
    return ext


def texture_name(gripper_open: float, color: Optional[str]) -> str:
    """joint_marker.py:128-140."""
    if color is None:
        return "sphere_yellow_stripe_texture.png" if gripper_open <= 0.1 else "sphere_cyan_stripe_texture.png"
    return COLOR_TEXTURES[color]


def base_color(gripper_open: float):
    """joint_marker.py:168-172 (rgb of the rgba factor)."""
    return (0.60392156862, 0.86274509803, 1.0) if gripper_open > 0.1 else (1.0, 1.0, 0.0)


def load_atlas(texture_dir: str) -> np.ndarray:
    """The five sphere textures as uint8 [5, th, tw, 4] (``Image.open(...).convert("RGBA")``, joint_marker.py:142-147), in SPHERE_TEXTURES order."""
    from PIL import Image

    layers = [np.asarray(Image.open(os.path.join(texture_dir, n)).convert("RGBA"), dtype=np.uint8) for n in SPHERE_TEXTURES]
    if len({l.shape for l in layers}) != 1:
        raise ValueError(f"{texture_dir}: the sphere textures must share one size, got {[l.shape for l in layers]}")
    return np.ascontiguousarray(np.stack(layers))


def pack_view(cam_intrinsic, cam_extrinsic, joint_matrices, joint_opens, sphere_colors, radius: float, znear: float, zfar: float,
              S: int = 4):
    """One view's kernel inputs: (cam f32 [18], spheres f32 [S, 16], tex_index int32 [S], count).  ``cam_extrinsic`` is RLBench's (the flip
    is applied here); texture and factor are chosen as ``render_action`` does."""
    n = len(joint_matrices)
    if n > S or S > MAX_SPHERES:
        raise ValueError(f"{n} spheres in a view packed for {S} (at most {MAX_SPHERES})")
    K = np.asarray(cam_intrinsic, dtype=np.float64)
    cam = np.zeros(CAM_FLOATS, np.float32)
    cam[:4] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    cam[4:16] = flip_extrinsic(cam_extrinsic)[:3, :4].reshape(-1)
    cam[16:] = (znear, zfar)
    sph, tex = np.zeros((S, SPHERE_FLOATS), np.float32), np.zeros(S, np.int32)
    for i, (m, op) in enumerate(zip(joint_matrices, joint_opens)):
        sph[i, :12] = np.asarray(m, dtype=np.float64)[:3, :4].reshape(-1)
        sph[i, 12] = radius
        sph[i, 13:] = base_color(op)
        tex[i] = SPHERE_TEXTURES.index(texture_name(op, sphere_colors[i]))
    return cam, sph, tex, n


def pack_views(views: Sequence, S: int = 4) -> Dict[str, np.ndarray]:
    """``pack_view`` tuples -> the batch arrays of ``render_views``."""
    return {"cams": np.stack([v[0] for v in views]), "spheres": np.stack([v[1] for v in views]),
            "tex_index": np.stack([v[2] for v in views]).astype(np.int32), "count": np.asarray([v[3] for v in views], np.int32)}


WINDOW_HALF_MAX = 127.0  # a window is at most 255 pixels a side: inside gn_openloop_sphere_metrics' 256


def sphere_windows(cams, spheres, count, H: int, W: int, scale: float = 2.0, min_half: float = 3.0) -> np.ndarray:
    """The pixel window around each sphere's projected centre, for ``gn_openloop_sphere_metrics``: ``cams`` [..., 18], ``spheres``
    [..., S, 16], ``count`` [...] (the ``pack_views`` / ``replay.view_tables`` layouts) -> int32 [..., S, 4] = (x0, y0, x1, y1), half-open.

    ``gn_render_spheres``' ray rule (include/genima_hip.h) inverted, in numpy f64: with ``R | t`` the camera pose and ``c`` the sphere pose's
    translation column, ``p = R^T (c - t)``, ``z = -p.z``, ``u = cx + fx p.x / z``, ``v = cy - fy p.y / z``, ``r_px = |fx| radius / z``,
    ``h = min(max(min_half, scale r_px), 127)``; ``x0 = clip(floor(u - h), 0, W)``, ``x1 = clip(ceil(u + h), 0, W)``, ``y0`` / ``y1`` likewise
    with ``v`` and ``H``.  A sphere with index ``s >= count``, with ``z`` outside ``[znear, zfar]`` or whose clipped window is empty gets
    ``(0, 0, 0, 0)``.  ``r_px`` is the radius at the centre's depth: ``scale`` is the margin for perspective and for a generated sphere that
    sits beside the true one.  Windows of different spheres may overlap; they then share pixels."""
    cams, sph, count = np.asarray(cams, np.float64), np.asarray(spheres, np.float64), np.asarray(count)
    S = sph.shape[-2]
    fx, fy, cx, cy, znear, zfar = (cams[..., i, None] for i in (0, 1, 2, 3, 16, 17))
    pose = cams[..., 4:16].reshape(cams.shape[:-1] + (3, 4))
    d = sph[..., [3, 7, 11]] - pose[..., None, :, 3]  # c - t, [..., S, 3]
    p = np.einsum("...ji,...sj->...si", pose[..., :3], d)  # R^T (c - t)
    z = -p[..., 2]
    ok = (np.arange(S) < count[..., None]) & (z >= znear) & (z <= zfar) & (z > 0)
    zs = np.where(ok, z, 1.0)
    u, v = cx + fx * p[..., 0] / zs, cy - fy * p[..., 1] / zs
    h = np.minimum(np.maximum(float(min_half), float(scale) * np.abs(fx) * sph[..., 12] / zs), WINDOW_HALF_MAX)
    with np.errstate(invalid="ignore"):
        win = np.stack([np.clip(np.floor(u - h), 0, W), np.clip(np.floor(v - h), 0, H), np.clip(np.ceil(u + h), 0, W), np.clip(np.ceil(v + h), 0, H)], axis=-1)
    ok &= np.isfinite(win).all(axis=-1) & (win[..., 2] > win[..., 0]) & (win[..., 3] > win[..., 1])
    return np.where(ok[..., None], win, 0.0).astype(np.int32)


# ---- the device path ----
def _engine(engine=None):
    if engine is None:
        from .engine import Engine

        engine = Engine("cuda:0")
    return engine


def render_views(E, views: Dict, atlas, H: int, W: int, samples: int = 4, *, bg=None, bg2=None, blend=None, tile_index=None,
                 bg_tiled: bool = False, n_tiled: Optional[int] = None, want=("full",), full_scale=(2.0, -1.0), rnd_scale=(1.0, 0.0)) -> Dict:
    """Render and composite a batch of views on the device.  ``views``: the ``pack_views`` arrays (numpy, uploaded here, or device tensors);
    ``atlas`` uint8 [T, th, tw, 4], ``bg`` / ``bg2`` uint8 device tensors ([B, H, W, 3], or tiled [n, 2H, 2W, 3] with ``bg_tiled``),
    ``blend`` float64 [B].  ``want`` names the outputs: ``full``, ``rnd``, ``occupied`` (uint8) and ``full_f16``, ``rnd_f16`` (f16 NHWC-8
    [n_tiled, 2H, 2W, 8], the trainer's layout).  -> {name: device tensor}; nothing is copied back."""
    import torch

    dev = E.device

    def up(x, dtype):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=dev, dtype=dtype).contiguous()

    cams, spheres = up(views["cams"], torch.float32), up(views["spheres"], torch.float32)
    tex, count = up(views["tex_index"], torch.int32), up(views["count"], torch.int32)
    B = cams.shape[0]
    if n_tiled is None:
        n_tiled = (B + 3) // 4
    unknown = set(want) - {"full", "rnd", "occupied", "full_f16", "rnd_f16"}
    if unknown:
        raise ValueError(f"render_views: unknown outputs {sorted(unknown)}")
    out = {}
    for k in want:
        if k == "occupied":
            out[k] = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        elif k in ("full", "rnd"):
            out[k] = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        else:
            out[k] = torch.zeros((n_tiled, 2 * H, 2 * W, 8), dtype=torch.float16, device=dev)
    E.render_spheres(cams, spheres, tex, count, up(atlas, torch.uint8), H, W, samples, bg=bg, bg2=bg2,
                     blend=None if blend is None else up(blend, torch.float64), tile_index=None if tile_index is None else up(tile_index, torch.int32),
                     bg_tiled=bg_tiled, n_tiled=n_tiled, full_scale=full_scale, rnd_scale=rnd_scale, **out)
    return out


class JointMarker:
    """``render/joint_marker.py``'s JointMarker on the HIP ray-caster: same constructor (+ ``texture_dir``, the reference reads
    ``./sphere_textures/``; ``samples``; ``engine``) and the same ``render_action``."""

    def __init__(self, image_width, image_height, camera_scales, sphere_radius=0.008, znear=0.00001, zfar=3.0,
                 texture_dir="./sphere_textures/", samples: int = 4, engine=None):
        self._image_width, self._image_height = int(image_width), int(image_height)
        self._sphere_radius, self._znear, self._zfar = sphere_radius, znear, zfar
        self._camera_scales = list(camera_scales)
        self._samples = samples
        self.atlas = load_atlas(texture_dir)
        self._engine, self._atlas_dev, self._white = engine, None, None

    def _device(self):
        import torch

        if self._atlas_dev is None:
            self._engine = _engine(self._engine)
            self._atlas_dev = torch.from_numpy(self.atlas).to(self._engine.device)
            # the raw render is the composite over a white frame: white ? 255 : pixel
            self._white = torch.full((1, self._image_height, self._image_width, 3), 255, dtype=torch.uint8, device=self._engine.device)
        return self._engine

    def pack(self, cam_intrinsic, cam_extrinsic, joint_matrices, joint_opens, camera_scale=1.0, sphere_colors=(None,), S: int = 4):
        if camera_scale not in self._camera_scales:
            raise KeyError(camera_scale)  # the reference's mesh cache holds the constructor's scales only
        return pack_view(cam_intrinsic, cam_extrinsic, joint_matrices, joint_opens, sphere_colors, self._sphere_radius * camera_scale,
                         self._znear, self._zfar, S)

    def render_action(self, cam_intrinsic, cam_extrinsic, joint_matrices, joint_opens, camera_scale=1.0, sphere_colors=(None,)):
        """-> rendered_img: (h, w, 3) uint8 array, white where nothing was drawn (joint_marker.py:61-181)."""
        E = self._device()
        v = self.pack(cam_intrinsic, cam_extrinsic, joint_matrices, joint_opens, camera_scale, sphere_colors, S=max(4, len(joint_matrices)))
        out = render_views(E, pack_views([v], S=v[1].shape[0]), self._atlas_dev, self._image_height, self._image_width, self._samples,
                           bg=self._white, want=("full",))
        return out["full"][0].cpu().numpy()


# ---- the dataset loop (render_data.py) ----
@dataclass
class RenderConfig:
    """``render/cfgs/render.yaml``, same names and values (``render.sphere.radius`` -> sphere_radius, ``render.joints`` -> joints,
    ``draw.*`` -> draw_*)."""
    cameras: Sequence[str] = ("wrist", "front", "right_shoulder", "left_shoulder", "overhead")
    camera_scales: Sequence[float] = (3.0, 8.0, 6.5, 6.5, 6.5)
    image_width: int = 256
    image_height: int = 256
    znear: float = 0.00001
    zfar: float = 3.0
    action_horizon: int = 20
    alpha_blend: float = 0.7
    sphere_radius: float = 0.01
    joints: Dict[str, Sequence[int]] = field(default_factory=lambda: {"wrist": [1, 3, 5], "front": [1, 3, 5], "right_shoulder": [1, 3, 5],
                                                                      "left_shoulder": [1, 3, 5], "overhead": []})
    textures_path: Optional[str] = None  # directory of random background textures (None: no random-context tree)
    draw_rgb_rendered: bool = True
    draw_rnd_bg: bool = True
    texture_dir: str = "./sphere_textures/"
    samples: int = 4


def window_step(ts: int, n_steps: int, action_horizon: int) -> Optional[int]:
    """The one step of the horizon window whose poses are drawn at ``ts`` (render_data.py:235-242: the last of ``range(ts + 1,
    min(ts + 1 + horizon, n - 1))``), or None when the window is empty (the last ``ts``)."""
    last_idx = min(ts + 1 + action_horizon, n_steps - 1)
    return last_idx - 1 if last_idx > ts + 1 else None


def quat_xyzw_to_matrix(q) -> np.ndarray:
    """scipy's ``Rotation.from_quat([x, y, z, w]).as_matrix()`` (the quaternion is normalised first)."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def step_spheres(traj: Dict, cfg: RenderConfig, ts: int, camera: str):
    """-> (joint_matrices, joint_opens, colors) drawn into ``camera`` at ``ts``: the gripper, then the camera's listed joints, of the
    window's last step (render_data.py:233-267); three empty lists at the last ``ts``."""
    i = window_step(ts, len(traj["gripper_open"]), cfg.action_horizon)
    if i is None:
        return [], [], []
    mats, opens, colors = [np.array(traj["gripper_matrix"][i], dtype=np.float64)], [float(traj["gripper_open"][i])], [None]
    for joint in cfg.joints[camera]:
        pose = np.asarray(traj["joint_poses"][i][joint], dtype=np.float64)
        m = np.eye(4)
        m[:3, 3] = pose[:3]
        m[:3, :3] = quat_xyzw_to_matrix(pose[3:7])
        mats.append(m), opens.append(1.0), colors.append(JOINT_COLOR_MAP[joint])
    return mats, opens, colors


def tile_cameras(cameras: Sequence[str]) -> List[str]:
    """The cameras of the 2x2 tiling, in tile order: every camera but ``overhead`` (render_data.py:230, :293)."""
    return [c for c in cameras if "overhead" not in c]


def pack_step(traj: Dict, cfg: RenderConfig, ts: int, cameras: Optional[Sequence[str]] = None, S: int = 4):
    """``pack_view`` of every camera of ``cameras`` (default: all of cfg.cameras) at ``ts``."""
    out = []
    for cam in (cfg.cameras if cameras is None else cameras):
        c = list(cfg.cameras).index(cam)
        mats, opens, colors = step_spheres(traj, cfg, ts, cam)
        out.append(pack_view(traj["intrinsics"][ts][c], traj["extrinsics"][ts][c], mats, opens, colors,
                             cfg.sphere_radius * cfg.camera_scales[c], cfg.znear, cfg.zfar, S))
    return out


TRAJ_KEYS = ("intrinsics", "extrinsics", "gripper_matrix", "gripper_open", "joint_poses")


def save_traj(path: str, traj: Dict):
    np.savez(path, **{k: np.asarray(traj[k], dtype=np.float64) for k in TRAJ_KEYS})


def load_traj(path: str) -> Dict[str, np.ndarray]:
    with np.load(path) as z:
        return {k: z[k] for k in TRAJ_KEYS}


def traj_from_low_dim_obs(pkl_path: str, cameras: Sequence[str]) -> Dict[str, np.ndarray]:
    """RLBench's ``low_dim_obs.pkl`` (a pickled ``Demo`` of ``Observation``s: unpickling imports ``rlbench``, which must be installed for
    this call and for nothing else here) -> the plain-array trajectory."""
    import pickle

    with open(pkl_path, "rb") as f:
        obs = pickle.load(f)
    return {"intrinsics": np.array([[o.misc[f"{c}_camera_intrinsics"] for c in cameras] for o in obs], dtype=np.float64),
            "extrinsics": np.array([[o.misc[f"{c}_camera_extrinsics"] for c in cameras] for o in obs], dtype=np.float64),
            "gripper_matrix": np.array([o.gripper_matrix for o in obs], dtype=np.float64),
            "gripper_open": np.array([o.gripper_open for o in obs], dtype=np.float64),
            "joint_poses": np.array([o.misc["joint_poses"] for o in obs], dtype=np.float64)}


def render_episode(traj: Dict, rgb_frames: Dict[str, np.ndarray], out_dir: str, cfg: RenderConfig, rnd_out_dir: Optional[str] = None,
                   engine=None, steps_per_launch: int = 16):
    """``RenderData.render_demo``'s loop (render_data.py:220-323) for one episode: for every ``ts < L - 1`` and camera, draw the window's
    last step over the camera's frame.  Writes ``<out_dir>/<camera>_rgb/<ts>.png`` (the composite, as the reference overwrites its copy of
    the frame), ``tiled_rgb/<ts>.png``, ``tiled_rgb_rendered/<ts>.png`` (these three with ``cfg.draw_rgb_rendered``) and ``traj.npz``; with ``cfg.textures_path`` and ``rnd_out_dir``
    also ``<rnd_out_dir>/<camera>_rgb/<ts>.png``, the blend over a random texture -- texture by ``np.random.choice``, blend by
    ``np.random.uniform(alpha_blend, 1)``, drawn from numpy's global state per (ts, camera) in the reference's order.
    ``rgb_frames``: {camera: uint8 [L, H, W, 3]}."""
    import torch
    from PIL import Image

    E = _engine(engine)
    H, W, cams = cfg.image_height, cfg.image_width, list(cfg.cameras)
    L, C = len(traj["gripper_open"]), len(cams)
    tiles = tile_cameras(cams)
    assert len(tiles) == 4, "the 2x2 tiling takes exactly four cameras besides overhead"
    rnd = bool(cfg.draw_rnd_bg and cfg.textures_path and rnd_out_dir)
    texture_files = [os.path.join(cfg.textures_path, f) for f in os.listdir(cfg.textures_path)] if rnd else []
    draw_full = bool(cfg.draw_rgb_rendered)  # render_data.py:270: the full-context tree is written only when asked for
    for d in ([os.path.join(out_dir, f"{c}_rgb") for c in cams] + [os.path.join(out_dir, "tiled_rgb"), os.path.join(out_dir, "tiled_rgb_rendered")]
              if draw_full else [out_dir]):
        os.makedirs(d, exist_ok=True)
    for c in cams if rnd else []:
        os.makedirs(os.path.join(rnd_out_dir, f"{c}_rgb"), exist_ok=True)
    save_traj(os.path.join(out_dir, "traj.npz"), traj)
    atlas = torch.from_numpy(load_atlas(cfg.texture_dir)).to(E.device)
    for t0 in range(0, L - 1, steps_per_launch):
        steps = list(range(t0, min(t0 + steps_per_launch, L - 1)))
        views, bg, bg2, blend = [], [], [], []
        for ts in steps:  # view order: ts-major, camera-minor -- the order of the reference's random draws
            views += pack_step(traj, cfg, ts)
            for cam in cams:
                bg.append(np.asarray(rgb_frames[cam][ts], dtype=np.uint8))
                if rnd:
                    tex = Image.open(np.random.choice(texture_files)).resize((W, H))
                    bg2.append(np.asarray(tex.convert("RGB"), dtype=np.uint8))
                    blend.append(np.random.uniform(cfg.alpha_blend, 1.0))
        kw = dict(bg2=torch.from_numpy(np.stack(bg2)).to(E.device), blend=np.asarray(blend, np.float64)) if rnd else {}
        out = render_views(E, pack_views(views), atlas, H, W, cfg.samples, bg=torch.from_numpy(np.stack(bg)).to(E.device),
                           want=("full", "rnd") if rnd else ("full",), **kw)
        full = out["full"].cpu().numpy().reshape(len(steps), C, H, W, 3)
        rnds = out["rnd"].cpu().numpy().reshape(len(steps), C, H, W, 3) if rnd else None
        for k, ts in enumerate(steps):
            for c, cam in enumerate(cams):
                if draw_full:
                    Image.fromarray(full[k, c]).save(os.path.join(out_dir, f"{cam}_rgb", f"{ts}.png"))
                if rnd:
                    Image.fromarray(rnds[k, c]).save(os.path.join(rnd_out_dir, f"{cam}_rgb", f"{ts}.png"))
            if not draw_full:
                continue
            ix = [cams.index(c) for c in tiles]
            Image.fromarray(_tile([rgb_frames[c][ts] for c in tiles])).save(os.path.join(out_dir, "tiled_rgb", f"{ts}.png"))
            Image.fromarray(_tile([full[k, i] for i in ix])).save(os.path.join(out_dir, "tiled_rgb_rendered", f"{ts}.png"))


def _tile(images) -> np.ndarray:
    """Four [H, W, 3] images -> [2H, 2W, 3] in the order of ``tiling.CROP_ORDER`` (``RenderData.tile_images``: (0, 0), (W, 0), (0, H), (W, H))."""
    h, w = images[0].shape[:2]
    if (h, w) == (256, 256):
        return tiling.tile_u8(images, 1)[0]
    out = np.zeros((2 * h, 2 * w, 3), np.uint8)
    for t, im in enumerate(images):
        out[(t >> 1) * h:(t >> 1) * h + h, (t & 1) * w:(t & 1) * w + w] = im
    return out


class TrajectorySource:
    """What ``data.DataLoader(render_targets=...)`` draws its targets from: for a sample whose conditioning image is
    ``<episode>/tiled_rgb/<ts>.png`` the four tile cameras' views at ``ts`` of ``<episode>/traj.npz`` (``render_episode`` writes both)."""

    def __init__(self, cfg: RenderConfig, traj_name: str = "traj.npz"):
        self.cfg, self.traj_name = cfg, traj_name
        self.H, self.W, self.samples = cfg.image_height, cfg.image_width, cfg.samples
        self.atlas = load_atlas(cfg.texture_dir)
        self._trajs: Dict[str, Dict] = {}
        self._views: Dict = {}  # (episode, ts) -> packed views: every epoch asks for the same ones
        self._atlas_dev = None

    def views(self, conditioning_path: str):
        ep = os.path.dirname(os.path.dirname(os.path.abspath(conditioning_path)))
        ts = int(os.path.splitext(os.path.basename(conditioning_path))[0])
        got = self._views.get((ep, ts))
        if got is None:
            traj = self._trajs.get(ep)
            if traj is None:
                traj = self._trajs[ep] = load_traj(os.path.join(ep, self.traj_name))
            got = self._views[(ep, ts)] = pack_step(traj, self.cfg, ts, tile_cameras(self.cfg.cameras))
        return got

    def atlas_on(self, device):
        import torch

        if self._atlas_dev is None or self._atlas_dev.device != torch.device(device):
            self._atlas_dev = torch.from_numpy(self.atlas).to(device)
        return self._atlas_dev


def synthetic_episode(L: int = 9, seed: int = 7, texture_dir: str = "./sphere_textures/", action_horizon: int = 4):
    """A generated demo in render.yaml's geometry for tests and benchmarks (no simulator needed): five fixed RLBench-style cameras
    (negative focal lengths, looking down +z) 0.9 m from the origin, a gripper and seven joints that move round it, random 256^2 frames.
    -> (RenderConfig, traj, {camera: uint8 [L, 256, 256, 3]})."""
    rng = np.random.RandomState(seed)
    cfg = RenderConfig(action_horizon=action_horizon, texture_dir=texture_dir)
    C, H, W = len(cfg.cameras), cfg.image_height, cfg.image_width

    def rot():
        q = rng.randn(4)
        return quat_xyzw_to_matrix(q)

    intr, extr = np.zeros((L, C, 3, 3)), np.zeros((L, C, 4, 4))
    for c in range(C):
        E = np.eye(4)
        E[:3, :3] = rot()
        E[:3, 3] = -E[:3, :3] @ np.array([0.0, 0.0, 0.9])  # every camera sees the origin 0.9 m ahead
        intr[:, c], extr[:, c] = np.array([[-351.6, 0, W / 2], [0, -351.6, H / 2], [0, 0, 1.0]]), E
    grip, opens, joints = np.zeros((L, 4, 4)), np.zeros(L), np.zeros((L, 7, 7))
    for i in range(L):
        p = np.array([0.1 * np.sin(i), 0.1 * np.cos(i), 0.05 * np.sin(2 * i)])
        grip[i] = np.eye(4)
        grip[i, :3, :3], grip[i, :3, 3] = rot(), p
        opens[i] = 1.0 if i % 3 else 0.0
        for j in range(7):
            q = rng.randn(4)
            joints[i, j] = np.concatenate([p + rng.uniform(-0.15, 0.15, 3), q / np.linalg.norm(q)])
    traj = {"intrinsics": intr, "extrinsics": extr, "gripper_matrix": grip, "gripper_open": opens, "joint_poses": joints}
    return cfg, traj, {c: rng.randint(0, 256, (L, H, W, 3), dtype=np.uint8) for c in cfg.cameras}
