"""Camera-pose and light perturbations of held-out frames, on the host: the settings, their draws and the camera algebra behind
``OpenLoopEval(perturb=...)``.  Numpy only; the pixels are moved by ``gn_view_perturb`` (csrc/view_perturb.hip).

The reference's robustness evaluation ships six Colosseum factor files (controller/cfgs/colosseum/*.yaml).  Two of them can be built from a
held-out frame alone:

* ``camera_pose``.  A camera that rotates about its own optical centre sees the same rays, so the new image is a homography of the old one
  for any scene -- no parallax -- and a zoom or a principal-point shift, a change of intrinsics, maps the image the same way.  The evaluator's
  ground-truth target is drawn per batch from the camera table, so warping the observation and changing the table consistently gives a
  perturbed view that everything downstream describes without knowing about it.  This part is EXACT.  Colosseum also moves the camera
  (``position_range`` +-0.1 m); a translation needs depth, cannot be reproduced from an image and is LEFT OUT.
* ``light_color``.  Colosseum draws the colour of three lights; what that does to a pixel depends on materials nobody here knows.  A
  per-channel gain and offset on the observation is an image-space STAND-IN (``"model": "channel_gain"``).

Object colour, distractors, table texture and background texture need masks or a simulator and are out of scope.

The camera model is ``gn_render_spheres``' (include/genima_hip.h): a table row is ``fx fy cx cy | R t (3x4, camera to world) | znear zfar`` in
the convention ``render.pack_view`` stores -- x right, y up, -z forward -- and pixel (u, v) looks along ``R (dx, dy, -1)`` with ``dx = (u - cx)
/ fx``, ``dy = (cy - v) / fy`` and SIGNED fx, fy (RLBench's fx is negative).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

Range = Tuple[float, float]
CAMERA_KEYS = ("pitch", "yaw", "roll", "zoom", "shift_x", "shift_y")
_CAMERA_IDENTITY = {"pitch": 0.0, "yaw": 0.0, "roll": 0.0, "zoom": 1.0, "shift_x": 0.0, "shift_y": 0.0}
LIGHT_KEYS = ("r", "g", "b", "r_offset", "g_offset", "b_offset")  # the spec's names of gain[0..2] and offset[0..2]
_ONE3: Tuple[Range, Range, Range] = ((1.0, 1.0),) * 3
_ZERO3: Tuple[Range, Range, Range] = ((0.0, 0.0),) * 3


def _range(key: str, value) -> Range:
    """A number (a fixed value: lo == hi) or a (lo, hi) pair -> (lo, hi) as floats, refused by ``key`` where it is not one."""
    try:
        lo, hi = (value, value) if np.isscalar(value) else value
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"perturbation: {key} = {value!r} is not a number or a (lo, hi) pair") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"perturbation: {key} = {value!r} must be finite")
    if lo > hi:
        raise ValueError(f"perturbation: {key} has lo = {lo} > hi = {hi}")
    return lo, hi


@dataclasses.dataclass(frozen=True)
class Perturbation:
    """One setting: ranges that ``draw`` samples uniformly; a fixed value is ``lo == hi``.

    ``pitch`` / ``yaw`` / ``roll``: rotations in radians about the camera's own x (right), y (up) and z (backward) axes; ``zoom``: the factor
    on fx and fy; ``shift_x`` / ``shift_y``: the shift of the principal point in pixels; ``cameras``: the camera names the camera part applies
    to, None for all.  ``gain`` / ``offset``: per channel r, g, b a range each, the offsets in levels of 0 .. 255.  A number is taken as the
    fixed range (v, v)."""
    name: str = "identity"
    pitch: Range = (0.0, 0.0)
    yaw: Range = (0.0, 0.0)
    roll: Range = (0.0, 0.0)
    zoom: Range = (1.0, 1.0)
    shift_x: Range = (0.0, 0.0)
    shift_y: Range = (0.0, 0.0)
    cameras: Optional[Tuple[str, ...]] = None
    gain: Tuple[Range, Range, Range] = _ONE3
    offset: Tuple[Range, Range, Range] = _ZERO3

    def __post_init__(self):
        put = lambda k, v: object.__setattr__(self, k, v)  # frozen: normalise through object.__setattr__
        put("name", str(self.name))
        for k in CAMERA_KEYS:
            put(k, _range(k, getattr(self, k)))
        if not self.zoom[0] > 0.0:
            raise ValueError(f"perturbation: zoom = {self.zoom} must be > 0")
        for field, names in (("gain", LIGHT_KEYS[:3]), ("offset", LIGHT_KEYS[3:])):
            v = getattr(self, field)
            if np.isscalar(v) or len(v) != 3:
                raise ValueError(f"perturbation: {field} = {v!r} takes three ranges, one per channel")
            put(field, tuple(_range(n, x) for n, x in zip(names, v)))
        for n, (lo, _) in zip(LIGHT_KEYS[:3], self.gain):
            if lo < 0.0:
                raise ValueError(f"perturbation: {n} = {lo} is a gain and must not be negative")
        if self.cameras is not None:
            if isinstance(self.cameras, str) or not all(isinstance(c, str) and c for c in self.cameras):
                raise ValueError(f"perturbation: cameras = {self.cameras!r} must be a sequence of camera names or None")
            put("cameras", tuple(self.cameras))

    def describe(self) -> Dict:
        """A JSON-able dict from which ``parse`` rebuilds this setting.  It also says what the numbers are: ``camera["model"]`` is
        ``"rotation_about_optical_centre"`` with ``"translation": "left out"``, ``light["model"]`` is ``"channel_gain"``, a stand-in."""
        return {"name": self.name,
                "camera": dict({k: list(getattr(self, k)) for k in CAMERA_KEYS}, cameras=None if self.cameras is None else list(self.cameras),
                               model="rotation_about_optical_centre", translation="left out"),
                "light": {"gain": [list(r) for r in self.gain], "offset": [list(r) for r in self.offset], "model": "channel_gain"}}


PRESETS: Dict[str, Perturbation] = {
    # Colosseum's camera_pose.yaml draws euler_range +-0.05 rad and position_range +-0.1 m for the front and the two shoulder cameras, not the
    # wrist.  The rotation is reproduced; the +-0.1 m position_range cannot be reproduced from an image (a translation needs depth) and is left
    # out.  The rotation here is about THIS camera model's own axes (x right, y up, -z forward), not CoppeliaSim's: the same size, not the
    # same axes.
    "camera_pose": Perturbation("camera_pose", pitch=(-0.05, 0.05), yaw=(-0.05, 0.05), roll=(-0.05, 0.05),
                                cameras=("front", "left_shoulder", "right_shoulder")),
    # Colosseum's light_color.yaml draws the colour of three lights from [0, 0.5]^3.  The gain range here is a stated starting value for the
    # image-space stand-in; it has not been measured against Colosseum's lights.
    "light_color": Perturbation("light_color", gain=((0.5, 1.0),) * 3),
}


def _spec_range(key: str, text: str) -> Range:
    parts = text.split("..")
    try:
        if not 1 <= len(parts) <= 2:
            raise ValueError
        vals = [float(p) for p in parts]
    except ValueError:
        raise ValueError(f"perturbation: {key}={text!r}: a number or lo..hi expected") from None
    return _range(key, (vals[0], vals[-1]))


def _parse_one(text: str) -> Perturbation:
    if text in PRESETS:
        return PRESETS[text]
    fields: Dict = {}
    gain, offset = list(_ONE3), list(_ZERO3)
    for section in filter(None, (s.strip() for s in text.split(";"))):
        kind, sep, body = section.partition(":")
        kind = kind.strip()
        if not sep or kind not in ("camera", "light"):
            raise ValueError(f"perturbation: {section!r}: a preset ({', '.join(sorted(PRESETS))}) or camera:key=..,.. / light:key=..,.. expected")
        for item in filter(None, (s.strip() for s in body.split(","))):
            key, sep, val = item.partition("=")
            key, val = key.strip(), val.strip()
            if not sep:
                raise ValueError(f"perturbation: {item!r} in the {kind} section: key=value expected")
            if kind == "camera" and key == "cameras":
                fields["cameras"] = tuple(c for c in val.split("|") if c)
            elif kind == "camera" and key in CAMERA_KEYS:
                fields[key] = _spec_range(key, val)
            elif kind == "light" and key in LIGHT_KEYS:
                i = LIGHT_KEYS.index(key)
                (gain if i < 3 else offset)[i % 3] = _spec_range(key, val)
            else:
                raise ValueError(f"perturbation: unknown {kind} key {key!r} (camera: {', '.join(CAMERA_KEYS)}, cameras; light: {', '.join(LIGHT_KEYS)})")
    if not fields and gain == list(_ONE3) and offset == list(_ZERO3):
        raise ValueError(f"perturbation: {text!r} sets nothing")
    return Perturbation(text, gain=tuple(gain), offset=tuple(offset), **fields)


def _join(a: Perturbation, b: Perturbation, name: str) -> Perturbation:
    """Two settings as one: each field from the setting that moves it off the identity; a field both move differently is refused."""
    ident = Perturbation()
    out = {}
    for f in CAMERA_KEYS + ("cameras", "gain", "offset"):
        va, vb, v0 = getattr(a, f), getattr(b, f), getattr(ident, f)
        if va != v0 and vb != v0 and va != vb:
            raise ValueError(f"perturbation: {name!r} sets {f} twice, to {va} and to {vb}")
        out[f] = va if va != v0 else vb
    return Perturbation(name, **out)


def parse(text) -> Perturbation:
    """A preset name (``PRESETS``), a spec, or ``describe()``'s dict -> the setting.

    A spec is ``camera:pitch=-0.05..0.05,roll=0.1,zoom=0.95..1.05;light:r=0.5..1,g=0.5..1,b=0.5..1``: sections ``camera`` (keys pitch, yaw,
    roll in radians, zoom, shift_x, shift_y in pixels, ``cameras=front|wrist``) and ``light`` (keys r, g, b for the gains, r_offset, g_offset,
    b_offset in levels), a value ``lo..hi`` or one number for a fixed value.  ``+`` joins two settings into one (``camera_pose+light_color``).
    The setting's name is the text.  Unknown keys, lo > hi, zoom <= 0 and a gain < 0 raise a ValueError that names the key."""
    if isinstance(text, Perturbation):
        return text
    if isinstance(text, dict):
        cam, light = dict(text.get("camera", {})), dict(text.get("light", {}))
        extra = (set(text) - {"name", "camera", "light"}) | (set(cam) - set(CAMERA_KEYS) - {"cameras", "model", "translation"}) | (set(light) - {"gain", "offset", "model"})
        if extra:
            raise ValueError(f"perturbation: unknown keys {sorted(extra)} in a description")
        cams = cam.get("cameras")
        return Perturbation(text.get("name", "identity"), cameras=None if cams is None else tuple(cams), gain=tuple(map(tuple, light.get("gain", _ONE3))),
                            offset=tuple(map(tuple, light.get("offset", _ZERO3))), **{k: tuple(cam[k]) for k in CAMERA_KEYS if k in cam})
    text = str(text).strip()
    parts = [p.strip() for p in text.split("+")]
    if not all(parts):
        raise ValueError(f"perturbation: {text!r}: an empty setting beside a '+'")
    p = _parse_one(parts[0])
    for q in parts[1:]:
        p = _join(p, _parse_one(q), text)
    return p if len(parts) == 1 else dataclasses.replace(p, name=text)


def draw(p: Perturbation, n_episodes: int, cameras: Sequence[str], seed: int = 0, rng=None) -> Dict[str, np.ndarray]:
    """The values of one evaluation -> ``{"pitch" | "yaw" | "roll" | "zoom" | "shift_x" | "shift_y": f64 [E, V], "gain" | "offset": f64
    [E, 3]}``, E episodes and V cameras.

    One ``numpy.random.default_rng(seed)``, asked in this order, each call ``rng.uniform(lo, hi, size)``: pitch, yaw, roll, zoom, shift_x,
    shift_y with size (E, V); then gain r, g, b and offset r, g, b with size (E,) each.  Every call is made whatever the ranges are, so a
    value does not depend on which other ranges are fixed (``uniform(v, v)`` returns v exactly).  The camera values are per (episode, camera); a camera outside ``p.cameras``
    is set to the identity after the draw.  The colour values are per EPISODE and shared by that episode's views: it is the scene's light.
    Every transition of an episode uses its episode's draw, as Colosseum randomises per episode.

    ``rng``: a ``numpy.random.Generator`` to ask instead, in the same order (``seed`` is then not used): ``sample_tables`` draws its coin
    from the generator first."""
    E, V = int(n_episodes), len(cameras)
    if rng is None:
        rng = np.random.default_rng(int(seed))
    out = {k: rng.uniform(*getattr(p, k), size=(E, V)) for k in CAMERA_KEYS}
    if p.cameras is not None:
        off = np.asarray([c not in p.cameras for c in cameras], bool)
        for k in CAMERA_KEYS:
            out[k][:, off] = _CAMERA_IDENTITY[k]
    out["gain"] = np.stack([rng.uniform(lo, hi, size=(E,)) for lo, hi in p.gain], axis=1)
    out["offset"] = np.stack([rng.uniform(lo, hi, size=(E,)) for lo, hi in p.offset], axis=1)
    return out


def rotation(pitch, yaw, roll) -> np.ndarray:
    """``Q = Rz(roll) Ry(yaw) Rx(pitch)`` f64 [..., 3, 3] in the camera's own axes (x right, y up, -z forward; right-handed rotations)."""
    pitch, yaw, roll = np.broadcast_arrays(np.asarray(pitch, np.float64), np.asarray(yaw, np.float64), np.asarray(roll, np.float64))
    one, zero = np.ones_like(pitch), np.zeros_like(pitch)

    def mat(rows):
        return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)

    cp, sp, cy, sy, cr, sr = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    rx = mat([[one, zero, zero], [zero, cp, -sp], [zero, sp, cp]])
    ry = mat([[cy, zero, sy], [zero, one, zero], [-sy, zero, cy]])
    rz = mat([[cr, -sr, zero], [sr, cr, zero], [zero, zero, one]])
    return rz @ ry @ rx


def perturb_cams(cams, Q, zoom=1.0, shift=(0.0, 0.0)) -> np.ndarray:
    """``cams`` f32 [..., 18], ``Q`` f64 [..., 3, 3], ``zoom`` [...], ``shift`` [..., 2] = (x, y) pixels -> the perturbed f32 table: in f64
    from the f32 values, pose ``R | t`` -> ``R Q | t`` (the camera turns about its own optical centre), fx and fy times ``zoom``, cx and cy
    plus ``shift``; rounded to f32 once.  A row whose Q is the identity matrix, whose zoom is 1 and whose shift is 0 is the input's own
    bits (a negative zero included)."""
    cams = np.asarray(cams)
    if cams.dtype != np.float32 or cams.shape[-1] != 18:
        raise ValueError(f"perturb_cams: cams must be f32 [..., 18], got {cams.dtype} {cams.shape}")
    lead = cams.shape[:-1]
    Q = np.broadcast_to(np.asarray(Q, np.float64), lead + (3, 3))
    zoom = np.broadcast_to(np.asarray(zoom, np.float64), lead)
    shift = np.broadcast_to(np.asarray(shift, np.float64), lead + (2,))
    c = cams.astype(np.float64)
    pose = c[..., 4:16].reshape(lead + (3, 4))
    new = c.copy()
    new[..., 0], new[..., 1] = c[..., 0] * zoom, c[..., 1] * zoom
    new[..., 2], new[..., 3] = c[..., 2] + shift[..., 0], c[..., 3] + shift[..., 1]
    new[..., 4:16] = np.concatenate([pose[..., :3] @ Q, pose[..., 3:]], axis=-1).reshape(lead + (12,))
    same = (Q == np.eye(3)).all(axis=(-1, -2)) & (zoom == 1.0) & (shift == 0.0).all(axis=-1)
    return np.where(same[..., None], cams, new.astype(np.float32))


def homography(cam_old, cam_new) -> np.ndarray:
    """Two f32 camera tables [..., 18] that share an optical centre -> f64 [..., 9], the row-major matrix M that takes a pixel of the NEW view
    to the pixel of the OLD view that sees the same ray: what ``gn_view_perturb`` takes.  Built in f64 from the f32 tables the renderer will
    actually use: ``M = P_old (R_old^-1 R_new) D_new`` with

        D = [[1 / fx, 0, -cx / fx], [0, -1 / fy, cy / fy], [0, 0, -1]]      pixel -> ray direction (dx, dy, -1), signed fx and fy
        P = [[fx, 0, -cx], [0, -fy, -cy], [0, 0, -1]]                        ray direction d -> (u w, v w, w) with w = -d.z

    so w > 0 is "in front of the old camera".  The renderer casts its rays with R as the table stores it, and an f32 rotation is orthonormal
    only to about 6e-8, so the rays of the two views are matched through the INVERSE of R_old (its transpose for an exact rotation; the
    transpose of the rounded one would be off by 1e-5 px).  Where the two rows hold the same bits in their intrinsics and pose, M is the exact identity
    (fx (1 / fx) need not round to 1)."""
    old, new = np.asarray(cam_old), np.asarray(cam_new)
    if old.dtype != np.float32 or new.dtype != np.float32 or old.shape != new.shape or old.shape[-1] != 18:
        raise ValueError(f"homography: two f32 [..., 18] tables of one shape expected, got {old.dtype} {old.shape} and {new.dtype} {new.shape}")
    lead = old.shape[:-1]
    o, n = old.astype(np.float64), new.astype(np.float64)
    zero, one = np.zeros(lead), np.ones(lead)

    def mat(rows):
        return np.stack([np.stack(r, axis=-1) for r in rows], axis=-2)

    D = mat([[one / n[..., 0], zero, -n[..., 2] / n[..., 0]], [zero, -one / n[..., 1], n[..., 3] / n[..., 1]], [zero, zero, -one]])
    P = mat([[o[..., 0], zero, -o[..., 2]], [zero, -o[..., 1], -o[..., 3]], [zero, zero, -one]])
    Ro, Rn = o[..., 4:16].reshape(lead + (3, 4))[..., :3], n[..., 4:16].reshape(lead + (3, 4))[..., :3]
    M = (P @ (np.linalg.inv(Ro) @ Rn) @ D).reshape(lead + (9,))
    same = (old[..., :16].view(np.uint32) == new[..., :16].view(np.uint32)).all(axis=-1)
    return np.where(same[..., None], np.eye(3).reshape(9), M)


def transition_tables(p: Perturbation, cams, episode_of, n_episodes: int, cameras: Sequence[str], seed: int = 0):
    """The evaluator's part on the host: the clean f32 camera table [N, V, 18] and each transition's episode [N] -> ``(cams_new f32
    [N, V, 18], M f64 [N, V, 9], colour f64 [N, V, 6], draws)``: every transition gets its episode's draw, the colour row is shared by the
    episode's views, and ``draws`` is ``draw``'s dict."""
    cams = np.ascontiguousarray(cams)
    ep = np.asarray(episode_of, np.int64)
    d = draw(p, n_episodes, cameras, seed)
    Q = rotation(d["pitch"], d["yaw"], d["roll"])[ep]  # [N, V, 3, 3]
    new = perturb_cams(cams, Q, d["zoom"][ep], np.stack([d["shift_x"], d["shift_y"]], axis=-1)[ep])
    colour = np.concatenate([d["gain"], d["offset"]], axis=1)[ep]  # [N, 6]
    colour = np.ascontiguousarray(np.broadcast_to(colour[:, None, :], cams.shape[:2] + (6,)))
    return np.ascontiguousarray(new), np.ascontiguousarray(homography(cams, new)), colour, d


def sample_tables(p: Perturbation, cams, cameras: Sequence[str], key, prob: float = 1.0):
    """The train-time augmentation's part on the host (``data.DataLoader(view_augment=...)``): one sample's clean f32 camera table [4, 18],
    its rows in the order of ``cameras``, -> ``(cams_new f32 [4, 18], M f64 [4, 9], colour f64 [4, 6], applied)``.

    ``key``: a tuple of non-negative ints; the draw is a pure function of it.  ``rng = numpy.random.default_rng(list(key))``; FIRST ``applied
    = rng.random() < prob``, drawn whatever ``prob`` is, so the values below do not depend on ``prob``; then ``draw(p, 1, cameras,
    rng=rng)``.  ``cams_new = perturb_cams(...)``, ``M = homography(cams, cams_new)``, and the colour row is shared by the four views: it is
    the scene's light.  Not applied: the input camera bits and the identity of both parts.  A camera outside ``p.cameras`` keeps its bits and
    the identity matrix (the ``camera_pose`` preset leaves the wrist alone); the light still reaches it."""
    cams = np.ascontiguousarray(cams)
    V = len(cameras)
    if cams.dtype != np.float32 or cams.shape != (V, 18):
        raise ValueError(f"sample_tables: cams must be f32 [{V}, 18], got {cams.dtype} {cams.shape}")
    key = [int(k) for k in key]
    if not key or min(key) < 0:
        raise ValueError(f"sample_tables: key = {key} must be a non-empty tuple of non-negative ints")
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"sample_tables: prob = {prob} must lie in [0, 1]")
    rng = np.random.default_rng(key)
    applied = bool(rng.random() < float(prob))
    d = draw(p, 1, cameras, rng=rng)
    if not applied:
        return cams.copy(), np.tile(np.eye(3).reshape(1, 9), (V, 1)), np.tile(np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]), (V, 1)), False
    new = np.ascontiguousarray(perturb_cams(cams, rotation(d["pitch"][0], d["yaw"][0], d["roll"][0]), d["zoom"][0],
                                            np.stack([d["shift_x"][0], d["shift_y"][0]], axis=-1)))
    colour = np.ascontiguousarray(np.broadcast_to(np.concatenate([d["gain"][0], d["offset"][0]])[None, :], (V, 6)))
    return new, np.ascontiguousarray(homography(cams, new)), colour, True


def draw_ranges(draws: Dict[str, np.ndarray]) -> Dict:
    """``draw``'s dict -> per parameter the smallest and the largest value drawn (``gain`` / ``offset`` per channel), JSON-able."""
    out = {k: {"min": float(draws[k].min()), "max": float(draws[k].max())} for k in CAMERA_KEYS}
    for k in ("gain", "offset"):
        out[k] = {"min": draws[k].min(axis=0).tolist(), "max": draws[k].max(axis=0).tolist()}
    return out


def lost_windows(clean_windows, windows, drawn=None) -> int:
    """The number of spheres whose window (``render.sphere_windows``: (0, 0, 0, 0) is "none") exists in ``clean_windows`` and is empty in
    ``windows``: the perturbation moved them out of the view.  ``drawn``: a bool mask over the spheres to count, None for all."""
    had, has = np.asarray(clean_windows).any(axis=-1), np.asarray(windows).any(axis=-1)
    lost = had & ~has
    return int((lost if drawn is None else lost & np.asarray(drawn, bool)).sum())
