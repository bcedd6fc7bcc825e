"""-m "not gpu": the host half of the blur / affine augmentations (genima_amd/augment.py) -- torchvision's draws, the inverse affine
matrix and the Gaussian taps -- against the restatement in tests/augment_ref.py, with no device."""
import math

import pytest
import torch

import augment_ref as AR
from genima_amd import augment as A


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
def test_draws_match_get_params(seed):
    g, r = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
    assert A.draw_blur_sigma(g) == AR.blur_get_params(0.1, 2.0, r)
    for res in (512, 256, 33):
        assert A.draw_affine(res, g) == AR.affine_get_params(img_size=(res, res), generator=r, **AR.AFFINE_ARGS)
    assert torch.equal(g.get_state(), r.get_state())


def test_affine_draw_ranges_and_the_empty_shear_range():
    g = torch.Generator().manual_seed(3)
    for _ in range(200):
        s0 = g.get_state()
        angle, (tx, ty), scale, shear = A.draw_affine(512, g)
        assert 0.0 <= angle <= 10.0 and 0.9 <= scale <= 1.1 and shear == (1.0, 0.0)
        assert isinstance(tx, int) and isinstance(ty, int) and abs(tx) <= 51 and abs(ty) <= 51
        # five uniforms: the shear draw is consumed although its range is empty
        h = torch.Generator()
        h.set_state(s0)
        for _ in range(5):
            torch.empty(1).uniform_(0, 1, generator=h)
        assert torch.equal(h.get_state(), g.get_state())


def test_translation_rounds_half_to_even():
    assert [int(round(v)) for v in (0.5, 1.5, 2.5, -0.5, -1.5)] == [0, 2, 2, 0, -2]  # the rule draw_affine relies on


@pytest.mark.parametrize("params", [(0.0, (0, 0), 1.0, (0.0, 0.0)), (7.3, (5, -12), 0.93, (1.0, 0.0)), (10.0, (-51, 51), 1.1, (1.0, 0.0)),
                                    (3.0, (1, 2), 1.0, (1.0, 0.5))])
def test_inverse_matrix_matches_restatement(params):
    got = A.affine_inverse_matrix(*params)
    want = AR.inverse_affine_matrix([0.0, 0.0], params[0], [float(t) for t in params[1]], params[2], params[3])
    assert got == want


def test_inverse_matrix_known_answers():
    assert A.affine_inverse_matrix(0.0, (0, 0), 1.0, (0.0, 0.0)) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    m = A.affine_inverse_matrix(90.0, (0, 0), 1.0, (0.0, 0.0))
    for a, b in zip(m, [0.0, 1.0, 0.0, -1.0, 0.0, 0.0]):
        assert abs(a - b) < 1e-12
    # scale and translation: the inverse undoes both, so the source of (tx, ty) is the centre
    m = A.affine_inverse_matrix(0.0, (4, -6), 2.0, (0.0, 0.0))
    assert m == [0.5, 0.0, -2.0, 0.0, 0.5, 3.0]
    assert abs(m[0] * 4 + m[1] * -6 + m[2]) < 1e-12 and abs(m[3] * 4 + m[4] * -6 + m[5]) < 1e-12


@pytest.mark.parametrize("sigma", [0.1, 0.7, 1.3, 2.0])
@pytest.mark.parametrize("ksize", [3, 5, 9])
def test_gaussian_taps(sigma, ksize):
    k = A.gaussian_taps(sigma, ksize)
    assert k.dtype == torch.float32 and k.shape == (ksize,)
    assert torch.equal(k, AR.get_gaussian_kernel1d(ksize, sigma))
    assert abs(float(k.sum()) - 1.0) < 1e-6 and torch.equal(k, k.flip(0))
    assert float(k[ksize // 2]) == float(k.max())
    if ksize == 3:  # closed form: [e, 1, e] / (1 + 2e), e = exp(-1 / (2 sigma^2))
        e = math.exp(-0.5 / sigma ** 2)
        assert abs(float(k[0]) - e / (1 + 2 * e)) < 1e-6


def test_parse_keeps_the_reference_order_and_refuses_elastic():
    assert A.parse_augmentations("crop,affine,blur,colorjitter") == ["colorjitter", "blur", "affine", "crop"]
    assert A.parse_augmentations("crop,colorjitter") == ["colorjitter", "crop"]
    assert A.parse_augmentations(None) == [] and A.parse_augmentations("") == []
    for bad in ("elastic", "crop,elastic", "sharpen", "blur,Affine"):
        with pytest.raises(NotImplementedError):
            A.parse_augmentations(bad)


@pytest.mark.parametrize("augs", ["colorjitter,blur,affine,crop", "crop,affine,blur,colorjitter", "affine,crop", "blur", "crop,colorjitter"])
def test_chain_draws_follow_the_restatement(augs):
    """The restated chain runs torchvision's ops on small CPU tensors; draw_augmentations must draw the same values and leave the
    generator in the same state."""
    R = 16
    g = torch.Generator().manual_seed(11)
    _, _, params = AR.augment_data(torch.rand(2, 3, R, R) * 2 - 1, torch.rand(2, 3, R, R), augs, R, g)
    h = torch.Generator().manual_seed(11)
    draws = A.draw_augmentations(A.parse_augmentations(augs), R, h)
    assert torch.equal(g.get_state(), h.get_state())
    assert list(draws) == [a for a in A.ORDER if a in augs.split(",")]
    for name, p in params.items():
        assert draws[name] == p, name


def test_crop_colorjitter_draws_are_unchanged():
    """The README recipe draws exactly what it drew before blur and affine existed: the jitter, then the crop offsets."""
    g = torch.Generator().manual_seed(5)
    draws = A.draw_augmentations(A.parse_augmentations("crop,colorjitter"), 512, g)
    h = torch.Generator().manual_seed(5)
    assert draws == {"colorjitter": A.draw_color_jitter(h), "crop": A.draw_crop(generator=h)}
    assert torch.equal(g.get_state(), h.get_state())
