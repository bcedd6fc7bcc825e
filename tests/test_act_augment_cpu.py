"""The ACT ElasticTransform's displacement field in pixels (genima_amd.act_training.elastic_displacement) against the convention
torchvision samples it with: grid_sample(identity grid + normalised field, align_corners=False) over the identity grid
linspace((1 - S) / S, (S - 1) / S, S).  PARITY UNPINNED for the identity grid (torchvision is not installed here: its published
``_create_identity_grid`` is restated); the un-normalisation ((g + 1) S - 1) / 2 is torch's documented grid_sample behaviour and is
what this test settles: a normalised displacement d is d * S / 2 pixels, not d * (S - 1) / 2."""
import torch
import torch.nn.functional as F

import act_ops_ref as R
from genima_amd.act_training import elastic_displacement, elastic_field

S, SIGMA, ALPHA = 24, 2.0, 80.0  # small and square; alpha / sigma chosen so the displacements are several pixels


def _identity_grid(s: int) -> torch.Tensor:
    ax = torch.linspace((1 - s) / s, (s - 1) / s, s, dtype=torch.float64)
    return torch.stack([ax[None, :].expand(s, s), ax[:, None].expand(s, s)], -1)  # [..., 0] = x, [..., 1] = y


def test_pixel_field_is_the_normalised_field_in_grid_sample_units():
    field = elastic_field(S, S, ALPHA, SIGMA, generator=torch.Generator().manual_seed(3))
    disp = elastic_displacement(S, S, ALPHA, SIGMA, generator=torch.Generator().manual_seed(3))
    assert field.dtype == torch.float64 and tuple(field.shape) == (S, S, 2)
    assert disp.dtype == torch.float32 and tuple(disp.shape) == (S, S, 2) and disp.is_contiguous()
    assert float(disp.abs().max()) > 2.0, "the field must move samples by several pixels for a (S - 1) / S scale error to show"
    # same draws in the same order: the pixel field is the normalised one times ONE constant (f32 rounding of the product only)
    ratio = disp.double() / field
    conv = round(2 * float(ratio.median())) / 2  # S / 2 or (S - 1) / 2: a half-integer in either reading, the f32 rounding noise taken off
    assert float((ratio - conv).abs().max()) <= conv * 2.0 ** -22, float((ratio - conv).abs().max())

    img = torch.rand(1, 3, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    want = F.grid_sample(img, (_identity_grid(S) + field)[None], mode="bilinear", padding_mode="zeros", align_corners=False)
    # with the package's conversion applied in f64 the plain sampler and grid_sample agree to f64 rounding -- or the conversion is wrong
    got = R.warp_bilinear(img.permute(0, 2, 3, 1), field * conv).permute(0, 3, 1, 2)
    err = float((got - want).abs().max())
    print(f"pixels per normalised unit {conv!r}; plain sampler vs grid_sample, f64 pixel field: max |diff| {err:.3e}")
    assert err <= 1e-12, (conv, err)
    # the field as the device kernel receives it (f32) moves every tap weight by <= |d| 2^-24 / px
    got32 = R.warp_bilinear(img.permute(0, 2, 3, 1), disp).permute(0, 3, 1, 2)
    err32 = float((got32 - want).abs().max())
    bound32 = 4 * float(disp.abs().max()) * 2.0 ** -24  # two axes, each weight's error enters two taps, |img| <= 1
    print(f"plain sampler vs grid_sample, f32 pixel field: max |diff| {err32:.3e} (bound {bound32:.3e})")
    assert err32 <= bound32, (err32, bound32)
    # and the old conversion is visibly something else: (S - 1) / 2 leaves the samples short by |d| / S of a pixel
    short = R.warp_bilinear(img.permute(0, 2, 3, 1), field * ((S - 1) / 2)).permute(0, 3, 1, 2)
    assert float((short - want).abs().max()) > 1e-3


def test_zero_field_and_integer_shift_of_the_reference_sampler():
    """The helper sampler itself: identity on a zero field, an exact zero-filled shift on an integer one, and equal to grid_sample on a
    random +-3 px field -- it is the second reference of the device warp test."""
    g = torch.Generator().manual_seed(5)
    img = torch.rand(2, 13, 17, 4, dtype=torch.float64, generator=g)
    zero = torch.zeros(13, 17, 2, dtype=torch.float64)
    assert torch.equal(R.warp_bilinear(img, zero), img)
    shift = zero.clone()
    shift[..., 0], shift[..., 1] = 2.0, -1.0
    want = torch.zeros_like(img)
    want[:, 1:, :-2] = img[:, :-1, 2:]
    assert torch.equal(R.warp_bilinear(img, shift), want)
    rnd = (torch.rand(13, 17, 2, dtype=torch.float64, generator=g) * 6 - 3)
    assert float((R.warp_bilinear(img, rnd) - R.grid_sample_warp(img, rnd)).abs().max()) <= 1e-12
