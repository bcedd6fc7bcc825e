"""CPU restatement of the torchvision 0.15.2 transforms the reference's ``augment_data`` chains beyond ColorJitter and the crop
(diffusion/train_controlnet_genima.py:775-830, train_instruct_pix2pix_genima.py:655-710): GaussianBlur / RandomAffine /
ColorJitter / RandomCrop ``get_params`` and ``F.gaussian_blur`` / ``F.affine`` on float NCHW tensors.

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED: torchvision is not installed in this image; this file restates the published code of
``torchvision.transforms.transforms`` (the ``get_params``), ``_functional_tensor`` (``_get_gaussian_kernel1d / 2d``, ``gaussian_blur``,
``affine``, ``_gen_affine_grid``, ``_apply_grid_transform``) and ``functional._get_inverse_affine_matrix``.  Every ``get_params`` takes an
explicit generator where torchvision uses the global one.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import augment_torch as OA

Tensor = torch.Tensor
AFFINE_ARGS = dict(degrees=(0.0, 10.0), translate=(0.1, 0.1), scale_ranges=(0.9, 1.1), shears=(1.0, 1.0))


# ---- get_params
def color_jitter_get_params(generator):
    fn_idx = torch.randperm(4, generator=generator)
    b = float(torch.empty(1).uniform_(0.8, 1.2, generator=generator))
    c = float(torch.empty(1).uniform_(0.8, 1.2, generator=generator))
    s = float(torch.empty(1).uniform_(0.9, 1.1, generator=generator))
    h = float(torch.empty(1).uniform_(-0.05, 0.05, generator=generator))
    return fn_idx, b, c, s, h


def blur_get_params(sigma_min, sigma_max, generator):
    return torch.empty(1).uniform_(sigma_min, sigma_max, generator=generator).item()


def affine_get_params(degrees, translate, scale_ranges, shears, img_size, generator):
    angle = float(torch.empty(1).uniform_(float(degrees[0]), float(degrees[1]), generator=generator).item())
    if translate is not None:
        max_dx = float(translate[0] * img_size[0])
        max_dy = float(translate[1] * img_size[1])
        tx = int(round(torch.empty(1).uniform_(-max_dx, max_dx, generator=generator).item()))
        ty = int(round(torch.empty(1).uniform_(-max_dy, max_dy, generator=generator).item()))
        translations = (tx, ty)
    else:
        translations = (0, 0)
    if scale_ranges is not None:
        scale = float(torch.empty(1).uniform_(scale_ranges[0], scale_ranges[1], generator=generator).item())
    else:
        scale = 1.0
    shear_x = shear_y = 0.0
    if shears is not None:
        shear_x = float(torch.empty(1).uniform_(shears[0], shears[1], generator=generator).item())
        if len(shears) == 4:
            shear_y = float(torch.empty(1).uniform_(shears[2], shears[3], generator=generator).item())
    return angle, translations, scale, (shear_x, shear_y)


def random_crop_get_params(h, w, th, tw, generator):
    if w == tw and h == th:
        return 0, 0, h, w
    i = torch.randint(0, h - th + 1, size=(1,), generator=generator).item()
    j = torch.randint(0, w - tw + 1, size=(1,), generator=generator).item()
    return i, j, th, tw


# ---- functional ops
def get_gaussian_kernel1d(kernel_size: int, sigma: float) -> Tensor:
    ksize_half = (kernel_size - 1) * 0.5
    x = torch.linspace(-ksize_half, ksize_half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(img: Tensor, kernel_size: int, sigma: float) -> Tensor:
    k1 = get_gaussian_kernel1d(kernel_size, sigma).to(img.dtype)
    kernel = torch.mm(k1[:, None], k1[None, :])
    kernel = kernel.expand(img.shape[-3], 1, kernel.shape[0], kernel.shape[1])
    p = kernel_size // 2
    img = F.pad(img, [p, p, p, p], mode="reflect")
    return F.conv2d(img, kernel, groups=img.shape[-3])


def inverse_affine_matrix(center, angle, translate, scale, shear):
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def gen_affine_grid(theta: Tensor, w: int, h: int, ow: int, oh: int) -> Tensor:
    d = 0.5
    base_grid = torch.empty(1, oh, ow, 3, dtype=theta.dtype)
    base_grid[..., 0].copy_(torch.linspace(-ow * 0.5 + d, ow * 0.5 + d - 1, steps=ow))
    base_grid[..., 1].copy_(torch.linspace(-oh * 0.5 + d, oh * 0.5 + d - 1, steps=oh).unsqueeze_(-1))
    base_grid[..., 2].fill_(1)
    rescaled_theta = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype)
    return base_grid.view(1, oh * ow, 3).bmm(rescaled_theta).view(1, oh, ow, 2)


def affine(img: Tensor, angle, translate, scale, shear) -> Tensor:
    """F.affine(img, angle, translate, scale, shear) with the defaults (NEAREST, fill=None, center=None) on a float tensor."""
    matrix = inverse_affine_matrix([0.0, 0.0], angle, [float(t) for t in translate], scale, shear)
    theta = torch.tensor(matrix, dtype=img.dtype).reshape(1, 2, 3)
    grid = gen_affine_grid(theta, w=img.shape[-1], h=img.shape[-2], ow=img.shape[-1], oh=img.shape[-2])
    grid = grid.expand(img.shape[0], grid.shape[1], grid.shape[2], grid.shape[3])
    return F.grid_sample(img, grid, mode="nearest", padding_mode="zeros", align_corners=False)


def affine_tie_mask(angle, translate, scale, shear, H: int, W: int, eps: float = 1e-3) -> Tensor:
    """[H, W] bool: output pixels whose f64 source coordinate (x or y) lies within ``eps`` of a half-integer -- a rounding tie of
    nearbyint, the image edges -0.5 / W - 0.5 included -- where f32 grids that round differently may pick different pixels."""
    m = inverse_affine_matrix([0.0, 0.0], angle, [float(t) for t in translate], scale, shear)
    bx = torch.arange(W, dtype=torch.float64) - W * 0.5 + 0.5
    by = (torch.arange(H, dtype=torch.float64) - H * 0.5 + 0.5)[:, None]
    ix = m[0] * bx + m[1] * by + m[2] + W * 0.5 - 0.5
    iy = m[3] * bx + m[4] * by + m[5] + H * 0.5 - 0.5
    near = lambda v: ((v - 0.5) - torch.round(v - 0.5)).abs() < eps  # noqa: E731
    return near(ix) | near(iy)


# ---- the reference's augment_data on (image role, conditioning role)
def augment_data(images: Tensor, cond: Tensor, augmentations: str, resolution: int, generator):
    """-> (images, cond, params): the chain of diffusion/train_controlnet_genima.py:775-830 (elastic left out); params holds what
    each op drew."""
    params = {}
    augs_list = augmentations.split(",")
    if "colorjitter" in augs_list:
        fn_idx, b, c, s, h = color_jitter_get_params(generator)
        params["colorjitter"] = (tuple(int(v) for v in fn_idx), (b, c, s, h))
        cond = OA.color_jitter(cond, *params["colorjitter"])
    if "blur" in augs_list:
        sigma = blur_get_params(0.1, 2.0, generator)
        params["blur"] = sigma
        cond = gaussian_blur(cond, 3, sigma)
    if "affine" in augs_list:
        p = affine_get_params(img_size=(resolution, resolution), generator=generator, **AFFINE_ARGS)
        params["affine"] = p
        images = affine(images, *p)
        cond = affine(cond, *p)
    if "crop" in augs_list:
        padded = F.pad(images, (2, 2, 2, 2), mode="reflect")
        i, j, h, w = random_crop_get_params(padded.shape[-2], padded.shape[-1], resolution, resolution, generator)
        params["crop"] = (i, j)
        images = padded[..., i:i + h, j:j + w]
        cond = F.pad(cond, (2, 2, 2, 2), mode="reflect")[..., i:i + h, j:j + w]
    return images, cond, params
