"""The ACT ElasticTransform displacement field without a device: the f64 torch restatement (tests/elastic_ref.py) that the device test
compares with is pinned to the package's numpy route, the device route's surface exists, and factoring the tap helper out left the host
route's bits alone."""
import hashlib
import inspect

import pytest
import torch

import elastic_ref as ER
from genima_amd import _lib, act_training
from genima_amd.act_training import elastic_displacement, elastic_field

ALPHA = 80.0


@pytest.mark.parametrize("H, W, sigma, k", [(24, 24, 2.0, 17), (41, 48, 10.0, 81), (19, 37, 1.4, 13)])  # 1.4: int(8 sigma + 1) = 12 -> 13
def test_reference_agrees_with_the_numpy_route(H, W, sigma, k):
    taps = ER.gaussian_taps(sigma)
    assert taps.numel() == k and taps.dtype == torch.float32
    field = elastic_field(H, W, ALPHA, sigma, generator=torch.Generator().manual_seed(3))
    ref = ER.blur_field(ER.draw_noise(H, W, torch.Generator().manual_seed(3)), taps, ALPHA / W, ALPHA / H)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (H, W, 2) == tuple(field.shape)
    err = float((ref - field).abs().max())
    print(f"{H}x{W} sigma {sigma} (k {k}): max |torch f64 - numpy f64| {err:.3e} normalised units")
    assert err <= 1e-12


def test_the_abi_table_has_the_new_calls():
    assert "gn_elastic_field" in _lib.SIGNATURES and "gn_elastic_field_workspace_bytes" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["gn_elastic_field"]
    assert len(args) == 10 and len(_lib.SIGNATURES["gn_elastic_field_workspace_bytes"][1]) == 2


def test_the_device_route_surface_exists():
    assert callable(getattr(act_training, "elastic_displacement_device", None))
    p = inspect.signature(act_training.act_augment).parameters
    assert "field" in p and p["field"].default == "host"
    p = inspect.signature(act_training.elastic_displacement_device).parameters
    assert list(p) == ["E", "H", "W", "alpha", "sigma", "generator"] and p["alpha"].default == 80.0 and p["sigma"].default == 10.0


def test_taps_helper_is_the_reference_rule():
    for sigma in (1.4, 2.0, 10.0, 16.0):
        assert torch.equal(act_training.elastic_taps(sigma), ER.gaussian_taps(sigma))
    assert act_training.elastic_taps(16.0).numel() == 129


def test_host_route_kept_its_bits():
    # recorded on the parent commit (before the tap helper was factored out of elastic_field): sha256 of the f32 [24, 24, 2] bytes of
    # elastic_displacement(24, 24, 80.0, 2.0, generator=torch.Generator().manual_seed(3))
    parent = "0607dacc32224d035e48c9eef9c9ec2df4efd8d35e99547610a3135030def881"
    disp = elastic_displacement(24, 24, ALPHA, 2.0, generator=torch.Generator().manual_seed(3))
    assert hashlib.sha256(disp.numpy().tobytes()).hexdigest() == parent
