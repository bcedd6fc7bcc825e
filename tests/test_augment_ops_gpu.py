"""-m gpu: the device-side GaussianBlur / RandomAffine of genima_amd/augment.py and the whole augment_data chain against the torch
restatement of torchvision's ops (tests/augment_ref.py, oracle/augment_torch.py).

Bars: blur is f32 math stored as f16: <= 1e-3 absolute on values in [-1, 1].  affine is a gather: bit-exact, except at output pixels
whose f64 source coordinate lies within 1e-3 of a rounding tie of nearbyint (image edges included), where an f32 grid computed in
another order may pick the neighbour; those pixels stay under 1 %.  The chain's conditioning image goes through jitter, blur and the
gather with f16 storage between the ops: <= 3e-3 (the jitter bar of test_augment_gpu.py is 1.5e-3)."""
import pytest
import torch

import augment_ref as AR
from genima_amd import augment
from genima_amd._lib import GenimaHipError
from genima_amd.host import nchw_to_nhwc
from oracle import augment_torch as OA
from util import q16

pytestmark = pytest.mark.gpu


def _img(B, H, W, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return q16(torch.rand(B, 3, H, W, generator=g) * (hi - lo) + lo)


def _dev(x):
    return nchw_to_nhwc(x, 8).half().cuda()


def _host(y):
    return y[..., :3].permute(0, 3, 1, 2).float().cpu()


@pytest.mark.parametrize("sigma", [0.1, 0.7, 2.0])
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 1.0)])
def test_gaussian_blur_matches_reflect_pad_conv(engine, sigma, lo, hi):
    for (H, W), ksize in (((37, 29), 3), ((2, 9), 3), ((21, 45), 5), ((11, 13), 9)):
        x = _img(3, H, W, lo, hi, seed=H * W)
        y = augment.gaussian_blur(engine, _dev(x), sigma, ksize)
        ref = AR.gaussian_blur(x, ksize, sigma)
        err = float((_host(y) - ref).abs().max())
        assert err <= 1e-3, (H, W, ksize, sigma, err)
        assert float(y[..., 3:].abs().max()) == 0.0


def _check_affine(engine, x, params, max_excluded=0.01):
    H, W = x.shape[-2:]
    got = _host(augment.affine(engine, _dev(x), augment.affine_inverse_matrix(*params)))
    ref = AR.affine(x, *params)
    mask = AR.affine_tie_mask(*params, H, W)
    assert float(mask.float().mean()) < max_excluded, params
    keep = ~mask.expand_as(ref)
    assert torch.equal(got[keep], ref[keep]), (params, int((got != ref)[keep].sum()))
    return got, ref, mask


AFFINE_CASES = [
    (0.0, (0, 0), 1.0, (1.0, 0.0)),     # identity-like: the reference's 1-degree shear only
    (10.0, (0, 0), 1.0, (1.0, 0.0)),
    (10.0, (6, -6), 1.0, (1.0, 0.0)),
    (4.2, (-7, 5), 1.0, (1.0, 0.0)),
    (2.5, (0, 0), 0.9, (1.0, 0.0)),
    (7.9, (3, 2), 1.1, (1.0, 0.0)),
    (0.5, (0, 0), 0.9, (1.0, 0.0)),     # (a pure scale without rotation or shear puts whole rows on exact ties: not a reference case)
    (1.0, (2, -2), 1.1, (1.0, 0.0)),
]


@pytest.mark.parametrize("params", AFFINE_CASES)
def test_affine_matches_grid_sample(engine, params):
    x = _img(2, 64, 64, -1.0, 1.0, seed=4)
    got, ref, _ = _check_affine(engine, x, params)
    if params[2] <= 1.0 and (params[1] != (0, 0) or params[0] > 0):  # no zoom-in: some pixels map from outside the image
        assert float((got == 0).float().mean()) > 0.01  # the zero fill


def test_affine_identity_and_non_square(engine):
    x = _img(2, 48, 40, 0.0, 1.0, seed=5)
    got, _, mask = _check_affine(engine, x, (0.0, (0, 0), 1.0, (0.0, 0.0)))
    assert not bool(mask.any()) and torch.equal(got, x)
    got, _, mask = _check_affine(engine, x, (0.0, (5, -3), 1.0, (0.0, 0.0)))  # a pure integer shift: zero fill on two sides
    assert not bool(mask.any()) and torch.equal(got[..., :45, 5:], x[..., 3:, :35])
    assert float(got[..., 45:, :].abs().max()) == 0.0 and float(got[..., :5].abs().max()) == 0.0
    for params in ((6.1, (4, -4), 0.95, (1.0, 0.0)), (9.5, (-4, 3), 1.08, (1.0, 0.0))):
        _check_affine(engine, x, params)
    g = torch.Generator().manual_seed(21)
    for _ in range(4):
        _check_affine(engine, x, augment.draw_affine(48, g))


def _batch(px, cond, roles=augment.ROLES):
    return {roles[0]: _dev(px), roles[1]: _dev(cond), "input_ids": torch.zeros(px.shape[0], 77, dtype=torch.int64)}


def _cropped_mask(params, H, W):
    mask = AR.affine_tie_mask(*params["affine"], H, W) if "affine" in params else torch.zeros(H, W, dtype=torch.bool)
    if "crop" in params:
        mask = OA.reflect_pad_crop(mask[None, None].float(), *params["crop"])[0, 0] > 0
    return mask


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_augment_data_full_chain(engine, seed):
    R = 64
    px, cond = _img(2, R, R, -1.0, 1.0, seed), _img(2, R, R, 0.0, 1.0, seed + 100)
    augs = "colorjitter,blur,affine,crop"
    out = augment.augment_data(engine, augs, _batch(px, cond), generator=torch.Generator().manual_seed(seed))
    ref_p, ref_c, params = AR.augment_data(px, cond, augs, R, torch.Generator().manual_seed(seed))
    keep = ~_cropped_mask(params, R, R).expand_as(ref_p)
    assert float((~keep).float().mean()) < 0.01
    got_p, got_c = _host(out["pixel_values"]), _host(out["conditioning_pixel_values"])
    assert torch.equal(got_p[keep], ref_p[keep])
    err = float((got_c - ref_c)[keep].abs().max())
    assert err <= 3e-3, err
    assert float(out["conditioning_pixel_values"][..., 3:].abs().max()) == 0.0 and float(out["pixel_values"][..., 3:].abs().max()) == 0.0
    # the comma list's order does not matter: the reference's fixed order, the same draws
    again = augment.augment_data(engine, "crop,affine,blur,colorjitter", _batch(px, cond), generator=torch.Generator().manual_seed(seed))
    assert torch.equal(again["pixel_values"], out["pixel_values"]) and torch.equal(again["conditioning_pixel_values"], out["conditioning_pixel_values"])


def test_pix2pix_roles_jitter_clamps_like_the_reference(engine):
    """In InstructPix2Pix both images are in [-1, 1]; ColorJitter's _blend clamps the edited image into [0, 1] -- reproduced."""
    R = 48
    for seed in (1, 2, 3, 4):
        orig, edited = _img(2, R, R, -1.0, 1.0, seed), _img(2, R, R, -1.0, 1.0, seed + 50)
        batch = _batch(orig, edited, augment.P2P_ROLES)
        out = augment.augment_data(engine, "colorjitter", batch, generator=torch.Generator().manual_seed(seed), roles=augment.P2P_ROLES)
        ref_o, ref_e, _ = AR.augment_data(orig, edited, "colorjitter", R, torch.Generator().manual_seed(seed))
        got_e = _host(out["edited_pixel_values"])
        assert float((got_e - ref_e).abs().max()) <= 1.5e-3, seed
        assert float(got_e.min()) >= 0.0 and float(ref_e.min()) >= 0.0 and float(edited.min()) < -0.9
        assert out["original_pixel_values"] is batch["original_pixel_values"] and torch.equal(ref_o, orig)
    # the whole chain with the pix2pix roles: blur on the edited image only, affine and crop on both
    orig, edited = _img(2, R, R, -1.0, 1.0, 60), _img(2, R, R, -1.0, 1.0, 61)
    out = augment.augment_data(engine, "crop,colorjitter,blur,affine", _batch(orig, edited, augment.P2P_ROLES),
                               generator=torch.Generator().manual_seed(60), roles=augment.P2P_ROLES)
    ref_o, ref_e, params = AR.augment_data(orig, edited, "crop,colorjitter,blur,affine", R, torch.Generator().manual_seed(60))
    keep = ~_cropped_mask(params, R, R).expand_as(ref_o)
    assert torch.equal(_host(out["original_pixel_values"])[keep], ref_o[keep])
    assert float((_host(out["edited_pixel_values"]) - ref_e)[keep].abs().max()) <= 3e-3


def test_refusals(engine):
    x = _dev(_img(2, 16, 16, 0.0, 1.0, 0))
    batch = dict(pixel_values=x, conditioning_pixel_values=x.clone())
    for bad in ("elastic", "blur,elastic", "sharpen"):
        with pytest.raises(NotImplementedError):
            augment.augment_data(engine, bad, batch)
    with pytest.raises(GenimaHipError):
        augment.gaussian_blur(engine, _dev(_img(1, 1, 16, 0.0, 1.0, 0)), 1.0)
    with pytest.raises(GenimaHipError):
        augment.gaussian_blur(engine, x, 1.0, ksize=4)
    with pytest.raises(ValueError):  # affine draws at (resolution, resolution)
        augment.augment_data(engine, "affine", dict(pixel_values=_dev(_img(1, 16, 24, 0.0, 1.0, 0)),
                                                    conditioning_pixel_values=_dev(_img(1, 16, 24, 0.0, 1.0, 1))))
