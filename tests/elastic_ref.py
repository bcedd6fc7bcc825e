"""float64 restatement of the ACT ElasticTransform displacement field (torchvision v2.ElasticTransform._get_params) with torch on the CPU:
``F.pad(mode="reflect")`` followed by ``F.conv2d`` along W and then along H, on the f32 noise and the f32 taps cast to f64, times the
per-plane scale.  Nothing of genima_amd's blur code is used (its numpy sliding-window route and its device kernels are what this checks);
only the draw order -- dx first, then dy, each ``torch.rand([1, 1, H, W]) * 2 - 1`` -- is restated here."""
import torch
import torch.nn.functional as F
from torch import Tensor

F64 = torch.float64


def draw_noise(H: int, W: int, generator: torch.Generator) -> Tensor:
    """The two uniform [-1, 1) planes as the transform draws them -> f32 [2, H, W] (plane 0 = dx, plane 1 = dy)."""
    return torch.cat([torch.rand([1, 1, H, W], generator=generator) * 2 - 1 for _ in range(2)], dim=1)[0]


def gaussian_taps(sigma: float) -> Tensor:
    """torchvision's kernel: k = int(8 sigma + 1) made odd, f32 linspace / exp / normalise -> f32 [k]."""
    k = int(8 * sigma + 1)
    if k % 2 == 0:
        k += 1
    half = (k - 1) * 0.5
    pdf = torch.exp(-0.5 * (torch.linspace(-half, half, k) / sigma).pow(2))
    return pdf / pdf.sum()


def blur_field(noise: Tensor, taps: Tensor, scale_x: float, scale_y: float) -> Tensor:
    """noise f32 [2, H, W], taps f32 [k] -> f64 [H, W, 2] = (scale_x * blur(noise[0]), scale_y * blur(noise[1]))."""
    k = taps.numel()
    R = k // 2
    x = F.pad(noise.to(F64)[None], (R, R, R, R), mode="reflect")  # [1, 2, H + 2R, W + 2R]
    w = taps.to(F64)
    x = F.conv2d(x, w.view(1, 1, 1, k).expand(2, 1, 1, k).contiguous(), groups=2)  # along W
    x = F.conv2d(x, w.view(1, 1, k, 1).expand(2, 1, k, 1).contiguous(), groups=2)  # along H
    scale = torch.tensor([scale_x, scale_y], dtype=F64)
    return (x[0].permute(1, 2, 0) * scale).contiguous()


def pixel_scales(H: int, W: int, alpha: float):
    """(scale_x, scale_y) of the pixel field: alpha / size (the transform's scale) times size / 2 (normalised grid units -> pixels)."""
    return (alpha / W) * (W / 2), (alpha / H) * (H / 2)


def field_bound(alpha: float, k: int) -> float:
    """max |f32 device field - f64 reference| in pixels: each output is alpha / 2 times a double convex combination of values in (-1, 1),
    evaluated as 2k f32 FMAs plus the f32 store between the passes, the scale multiply and the final rounding."""
    return (alpha / 2) * (2 * k + 8) * 2.0 ** -24
