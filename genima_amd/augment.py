"""Train-time augmentation on the device: the reference's ``augment_data`` (diffusion/train_controlnet_genima.py:775-830, SDXL :770-,
InstructPix2Pix train_instruct_pix2pix_genima.py:655-710) for ``--augmentations`` from ``colorjitter,blur,affine,crop`` (README recipe
``crop,colorjitter``, README.md:204), on NHWC f16 8-channel batches already resident in HBM.

The ops run in the reference's fixed order whatever order the comma list gives; each draws from the torch CPU generator when it runs,
in torchvision's order, so a run seeded like the reference's draws the same values.  The reference calls every transform once on the
whole batch tensor, so each op makes ONE draw for the whole batch:
  colorjitter  ColorJitter.get_params: ``fn_idx = randperm(4)``; then brightness, contrast, saturation, hue factors, each
               ``float(torch.empty(1).uniform_(lo, hi))``; on the conditioning-role tensor;
  blur         GaussianBlur(3, sigma=(0.1, 2.0)).get_params: one uniform sigma; on the conditioning-role tensor;
  affine       RandomAffine.get_params(degrees (0, 10), translate (0.1, 0.1), scale (0.9, 1.1), shears (1, 1), img_size (res, res)):
               angle, tx, ty (``int(round(u))``), scale, shear_x (the empty range is still drawn); then F.affine (NEAREST, fill None) with
               the same parameters on both tensors -- the 0 fill lands in each tensor's own space;
  crop         RandomCrop.get_params on the reflect-padded image: ``i = randint(0, h - th + 1)``, ``j = randint(0, w - tw + 1)``; both.
``draw_augmentations`` makes the draws alone (no device); ``augment_data`` draws and launches.  ``elastic`` is not built and raises.
The ControlNet trainers' roles are ``pixel_values`` (image) / ``conditioning_pixel_values`` (conditioning); InstructPix2Pix's are
``original_pixel_values`` / ``edited_pixel_values`` (``P2P_ROLES``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import check
from .engine import Engine, _ptr

JITTER = dict(brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.9, 1.1), hue=(-0.05, 0.05))  # ColorJitter(0.2, 0.2, 0.1, 0.05)
CROP_PAD = 2
BLUR_KSIZE, BLUR_SIGMA = 3, (0.1, 2.0)  # GaussianBlur(kernel_size=3, sigma=(0.1, 2.0))
AFFINE = dict(degrees=(0.0, 10.0), translate=(0.1, 0.1), scale=(0.9, 1.1), shears=(1.0, 1.0))  # RandomAffine.get_params arguments
ORDER = ("colorjitter", "blur", "affine", "crop")  # augment_data's fixed order (elastic, between jitter and blur, is not built)
ROLES = ("pixel_values", "conditioning_pixel_values")  # (image role, conditioning role) of the ControlNet trainers' batch
P2P_ROLES = ("original_pixel_values", "edited_pixel_values")  # InstructPix2Pix: the edited image takes the conditioning role


def draw_color_jitter(generator: Optional[torch.Generator] = None) -> Tuple[Tuple[int, ...], Tuple[float, ...]]:
    """-> (op order, factors indexed by op id 0 brightness / 1 contrast / 2 saturation / 3 hue), torchvision's draw order."""
    order = tuple(int(v) for v in torch.randperm(4, generator=generator))
    factors = tuple(float(torch.empty(1).uniform_(lo, hi, generator=generator)) for lo, hi in
                    (JITTER["brightness"], JITTER["contrast"], JITTER["saturation"], JITTER["hue"]))
    return order, factors


def draw_crop(pad: int = CROP_PAD, generator: Optional[torch.Generator] = None) -> Tuple[int, int]:
    i = int(torch.randint(0, 2 * pad + 1, size=(1,), generator=generator))
    j = int(torch.randint(0, 2 * pad + 1, size=(1,), generator=generator))
    return i, j


def draw_blur_sigma(generator: Optional[torch.Generator] = None) -> float:
    """GaussianBlur.get_params: ``torch.empty(1).uniform_(0.1, 2.0).item()``."""
    return float(torch.empty(1).uniform_(BLUR_SIGMA[0], BLUR_SIGMA[1], generator=generator))


def draw_affine(resolution: int, generator: Optional[torch.Generator] = None):
    """RandomAffine.get_params with the reference's arguments and img_size (resolution, resolution) -> (angle, (tx, ty), scale,
    (shear_x, shear_y)); Python's round (half to even) on the translations, shear_y = 0 (two shear bounds)."""
    u = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=generator))  # noqa: E731
    angle = u(float(AFFINE["degrees"][0]), float(AFFINE["degrees"][1]))
    max_dx, max_dy = float(AFFINE["translate"][0] * resolution), float(AFFINE["translate"][1] * resolution)
    tx = int(round(u(-max_dx, max_dx)))
    ty = int(round(u(-max_dy, max_dy)))
    scale = u(AFFINE["scale"][0], AFFINE["scale"][1])
    shear_x = u(AFFINE["shears"][0], AFFINE["shears"][1])
    return angle, (tx, ty), scale, (shear_x, 0.0)


def affine_inverse_matrix(angle: float, translate: Sequence[float], scale: float, shear: Sequence[float],
                          center: Sequence[float] = (0.0, 0.0)) -> List[float]:
    """torchvision's _get_inverse_affine_matrix in f64; F.affine on a tensor passes centre (0, 0) (the grid is centred)."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = float(translate[0]), float(translate[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def gaussian_taps(sigma: float, ksize: int = BLUR_KSIZE) -> torch.Tensor:
    """torchvision _get_gaussian_kernel1d in f32: linspace(-(k - 1) / 2, (k - 1) / 2, k), exp(-0.5 (x / sigma)^2), normalised."""
    half = (ksize - 1) * 0.5
    x = torch.linspace(-half, half, steps=ksize)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def parse_augmentations(augmentations: Optional[str]) -> List[str]:
    """The comma list -> the requested ops in augment_data's order; ``elastic`` and unknown names raise."""
    augs = [a for a in (augmentations or "").split(",") if a]
    unsupported = [a for a in augs if a not in ORDER]
    if unsupported:
        raise NotImplementedError(f"augmentations {unsupported} are not built on the HIP path (built: {', '.join(ORDER)})")
    return [a for a in ORDER if a in augs]


def draw_augmentations(augs: Sequence[str], resolution: int, generator: Optional[torch.Generator] = None) -> Dict[str, object]:
    """Every draw of one augment_data call, in the reference's order, without touching the device: op name -> its parameters."""
    draws: Dict[str, object] = {}
    for a in ORDER:
        if a not in augs:
            continue
        if a == "colorjitter":
            draws[a] = draw_color_jitter(generator)
        elif a == "blur":
            draws[a] = draw_blur_sigma(generator)
        elif a == "affine":
            draws[a] = draw_affine(resolution, generator)
        else:
            draws[a] = draw_crop(CROP_PAD, generator)
    return draws


def _check_nhwc(x: torch.Tensor, what: str):
    if x.dim() != 4 or x.dtype != torch.float16 or not x.is_cuda or not x.is_contiguous() or x.shape[-1] % 8:
        raise ValueError(f"{what}: expected a contiguous NHWC f16 device tensor with C % 8 == 0, got {tuple(x.shape)} {x.dtype} {x.device}")


def color_jitter(E: Engine, x: torch.Tensor, order, factors, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x: f16 [B, H, W, ld >= 3], RGB in [0, 1]."""
    B, H, W, ld = x.shape
    out = torch.empty_like(x) if out is None else out
    ws = E._workspace(int(E.lib.gn_color_jitter_workspace_bytes(B)))
    check(E.lib.gn_color_jitter(E._ctx, _ptr(x), _ptr(out), B, H * W, ld, (C.c_int32 * 4)(*order), (C.c_float * 4)(*factors), _ptr(ws)), "gn_color_jitter")
    return out


def reflect_pad_crop(E: Engine, x: torch.Tensor, i: int, j: int, pad: int = CROP_PAD) -> torch.Tensor:
    B, H, W, Cc = x.shape
    out = torch.empty_like(x)
    check(E.lib.gn_reflect_pad_crop(E._ctx, _ptr(x), _ptr(out), B, H, W, Cc, pad, i, j), "gn_reflect_pad_crop")
    return out


def gaussian_blur(E: Engine, x: torch.Tensor, sigma: float, ksize: int = BLUR_KSIZE, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GaussianBlur with the drawn sigma on f16 [B, H, W, C % 8 == 0]: reflect padding + depthwise conv, every channel."""
    _check_nhwc(x, "gaussian_blur")
    B, H, W, Cc = x.shape
    out = torch.empty_like(x) if out is None else out
    taps = gaussian_taps(sigma, ksize)
    check(E.lib.gn_gaussian_blur(E._ctx, _ptr(x), _ptr(out), B, H, W, Cc, ksize, (C.c_float * ksize)(*taps.tolist())), "gn_gaussian_blur")
    return out


def affine(E: Engine, x: torch.Tensor, matrix: Sequence[float], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.affine (NEAREST, fill None) on f16 [B, H, W, C % 8 == 0] with the inverse matrix of ``affine_inverse_matrix`` (rounded to
    f32 as F_t.affine's theta); outside the image the output is 0."""
    _check_nhwc(x, "affine")
    B, H, W, Cc = x.shape
    out = torch.empty_like(x) if out is None else out
    theta = torch.tensor(list(matrix), dtype=torch.float32)
    check(E.lib.gn_affine_nearest(E._ctx, _ptr(x), _ptr(out), B, H, W, Cc, (C.c_float * 6)(*theta.tolist())), "gn_affine_nearest")
    return out


def augment_data(E: Engine, augmentations: Optional[str], batch: Dict[str, torch.Tensor], generator: Optional[torch.Generator] = None,
                 resolution: Optional[int] = None, roles: Tuple[str, str] = ROLES, extra: Optional[Dict[str, torch.Tensor]] = None):
    """``augment_data(args, batch)`` with ``args.augmentations`` given as the comma list; batch tensors NHWC f16 8-channel on the device.
    ``roles``: the batch keys of the image and conditioning roles (``P2P_ROLES`` for InstructPix2Pix).  ``resolution`` (the reference's
    ``args.resolution``, RandomAffine's img_size) defaults to the batch's H; ``affine`` needs square images.
    ``extra`` (not in the reference): further NHWC f16 tensors with C % 8 == 0 and the images' H x W (a per-pixel mask, say) that must stay
    registered with the images: each receives only the ops applied to BOTH roles -- ``affine`` then ``crop``, with the same draws -- and comes
    back under its own key.  The generator is consumed identically with or without it."""
    ik, ck = roles
    images, cond = batch[ik], batch[ck]
    extra = dict(extra or {})
    for k, v in extra.items():
        _check_nhwc(v, f"augment_data extra[{k!r}]")
        if k in batch or tuple(v.shape[:3]) != tuple(images.shape[:3]):
            raise ValueError(f"augment_data extra[{k!r}]: needs a key of its own and the images' {tuple(images.shape[:3])}, got {tuple(v.shape)}")
    augs = parse_augmentations(augmentations)
    if augs:
        H, W = int(images.shape[1]), int(images.shape[2])
        if "affine" in augs and (H != W or tuple(cond.shape[1:3]) != (H, W)):
            raise ValueError(f"affine augmentation needs square images of one size, got {tuple(images.shape)} / {tuple(cond.shape)}")
        draws = draw_augmentations(augs, H if resolution is None else int(resolution), generator)
        if "colorjitter" in draws:
            cond = color_jitter(E, cond, *draws["colorjitter"])
        if "blur" in draws:
            cond = gaussian_blur(E, cond, draws["blur"])
        if "affine" in draws:
            m = affine_inverse_matrix(*draws["affine"])
            images = affine(E, images, m)
            cond = affine(E, cond, m)
            extra = {k: affine(E, v, m) for k, v in extra.items()}
        if "crop" in draws:
            i, j = draws["crop"]
            images = reflect_pad_crop(E, images, i, j)
            cond = reflect_pad_crop(E, cond, i, j)
            extra = {k: reflect_pad_crop(E, v, i, j) for k, v in extra.items()}
    out = dict(batch)
    out[ik], out[ck] = images, cond
    out.update(extra)
    return out
