"""-m gpu: ``gn_view_perturb`` through the eager engine against tests/perturb_ref.py, the numpy f64 restatement of its pixel rule -- ``dst``,
``valid`` and ``n_revealed`` bit for bit (the rule is stated one rounded f64 operation at a time and the file is built without fused
multiply-adds, so there is no tolerance) -- and the refusals.

Shapes.  B = 5 views of 37 x 53: an odd view count, H != W, rows of 159 bytes that are no dword multiple (so aligned dword runs, unaligned
runs and the one-pixel tail of a row all occur), 518 runs per view = three workgroups.  B = 12 views of 64 x 64: the evaluator tests' size,
every row dword-aligned.  The five kinds of view cycle through the batch:

  0  the identity, gain 1 and offset 0: a copy
  1  an integer shift (+5, -3); gains 0.5 / 1.5 with offsets 0 / 0.5 so that results land on .5 (half to even) and saturate at 255
  2  a rotation by 20 degrees with a zoom-out of 1.25 about the centre: the samples leave all four edges; a gain that saturates and a
     negative offset that clamps at 0
  3  a zoom-out of 4 about the centre: su reaches both ends of its clamp, so the index one past 2 (W - 1) is reflected to -1 and caught by
     the clamp after the reflection
  4  a projective M given directly, whose w changes sign inside the image: the `!(w > 0)` branch, and huge u, v beside the zero line"""
import numpy as np
import pytest
import torch

import perturb_ref as PR
from genima_amd._lib import GenimaHipError

pytestmark = pytest.mark.gpu

COLOURS = np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0], [0.5, 1.5, 1.0, 0.0, 0.5, -0.5], [2.2, 1.0, 0.7, 0.0, -90.0, 10.0], [1.0, 0.9, 1.1, 0.5, 0.25, -0.75],
                    [0.9, 1.1, 1.0, 3.0, -3.0, 0.0]])


def _about_centre(A, H, W):
    """The 2x2 map ``A`` applied about the image centre, as a row-major 3x3."""
    c = np.array([W / 2.0, H / 2.0])
    M = np.eye(3)
    M[:2, :2], M[:2, 2] = A, c - A @ c
    return M.reshape(9)


def _case(B, H, W, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    a = np.deg2rad(20.0)
    kinds = [np.eye(3).reshape(9), np.array([1.0, 0, 5, 0, 1, -3, 0, 0, 1]),
             _about_centre(1.25 * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]), H, W), _about_centre(4.0 * np.eye(2), H, W),
             np.array([1.0, 0, 0, 0, 1, 0, -1.0 / (0.47 * W), 0.01, 1.0])]
    M = np.stack([kinds[b % 5] for b in range(B)])
    colour = np.stack([COLOURS[b % 5] for b in range(B)])
    return src, M, colour


@pytest.fixture(scope="module", params=[(5, 37, 53), (12, 64, 64)], ids=["5x37x53", "12x64x64"])
def case(request):
    B, H, W = request.param
    src, M, colour = _case(B, H, W, seed=B)
    return dict(B=B, H=H, W=W, src=src, M=M, colour=colour, want=PR.view_perturb(src, M, colour))  # the reference once per shape


def test_the_cases_reach_what_they_are_there_for(case):
    """On the reference alone: the properties the docstring lists are really in these inputs."""
    B, H, W, src = case["B"], case["H"], case["W"], case["src"]
    dst, valid, n = case["want"]
    assert np.array_equal(dst[0], src[0]) and valid[0].all() and n[0] == 0
    assert np.array_equal(valid[1, 3:, : W - 5], np.ones((H - 3, W - 5), np.uint8)) and n[1] == H * W - (H - 3) * (W - 5)
    shifted = src[1, : H - 3, 5:].astype(np.float64)
    assert np.array_equal(dst[1, 3:, : W - 5, 0], np.rint(shifted[..., 0] * 0.5).astype(np.uint8)) and (shifted[..., 0] % 2 == 1).any()  # .5, to even
    assert (dst[1, ..., 1] == 255).any() and (dst[2, ..., 0] == 255).any() and (dst[2, ..., 1] == 0).any()
    inv = valid[2] == 0
    assert inv[0].any() and inv[-1].any() and inv[:, 0].any() and inv[:, -1].any() and valid[2].any()  # all four edges left
    # kind 3: the corner pixels sample beyond both ends of the clamp
    X = np.array([0.5, W - 0.5])
    u = case["M"][3][0] * X + case["M"][3][2]
    assert u[0] - 0.5 < -(W - 1) and u[1] - 0.5 > 2 * (W - 1)
    # kind 4: w changes sign inside the image; behind the line everything is black and revealed
    Y, Xg = np.mgrid[0:H, 0:W] + 0.5
    w = (case["M"][4][6] * Xg + case["M"][4][7] * Y) + case["M"][4][8]
    assert (w > 0).any() and (w <= 0).any() and not dst[4][w <= 0].any() and not valid[4][w <= 0].any() and valid[4].any()
    assert n.tolist() == (valid == 0).reshape(B, -1).sum(axis=1).tolist()


def test_bits_equal_the_reference(engine, case):
    B, H, W = case["B"], case["H"], case["W"]
    src, M, colour = (torch.from_numpy(case[k]).cuda() for k in ("src", "M", "colour"))
    valid = torch.full((B, H, W), 9, dtype=torch.uint8, device="cuda")
    n = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    dst = engine.view_perturb(src, M, colour, valid=valid, n_revealed=n)
    want_dst, want_valid, want_n = case["want"]
    got = dst.cpu().numpy()
    bad = int((got != want_dst).sum())
    print(f"{B} x {H} x {W}: {bad} of {got.size} bytes differ from the reference; revealed per view {n.cpu().numpy().tolist()}")
    assert got.shape == (B, H, W, 3) and got.dtype == np.uint8 and bad == 0
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    assert n.cpu().numpy().tolist() == want_n.tolist()
    assert torch.equal(src, torch.from_numpy(case["src"]).cuda()), "the source was written"
    # the optional outputs are optional, and a second run gives the same bits (the counts are zeroed by the call, not accumulated)
    assert torch.equal(engine.view_perturb(src, M, colour), dst)
    out2 = torch.empty_like(dst)
    assert engine.view_perturb(src, M, colour, out=out2, n_revealed=n) is out2 and torch.equal(out2, dst) and n.cpu().numpy().tolist() == want_n.tolist()


def test_refusals(engine):
    """Argument checks only: every call below is refused before a launch and the outputs stay as they were."""
    B, H, W = 2, 8, 12
    src, M, colour = (torch.from_numpy(a).cuda() for a in _case(B, H, W, seed=1))
    out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    n = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    for bad in (dict(out=src), dict(M=None), dict(colour=None), dict(M=M.float()), dict(M=M[:1]), dict(colour=colour[:, :5].contiguous()), dict(src=src.cpu()),
                dict(src=src[..., :2].contiguous()), dict(out=out[:1]), dict(n_revealed=n.long()), dict(valid=torch.zeros((B, H, W, 1), dtype=torch.uint8, device="cuda"))):
        a = dict(dict(src=src, M=M, colour=colour, out=out, valid=None, n_revealed=n), **bad)
        with pytest.raises(GenimaHipError):
            engine.view_perturb(a["src"], a["M"], a["colour"], out=a["out"], valid=a["valid"], n_revealed=a["n_revealed"])
    lib, ctx = engine.lib, engine._ctx
    s, o, m, c, r = src.data_ptr(), out.data_ptr(), M.data_ptr(), colour.data_ptr(), n.data_ptr()
    big = torch.zeros((2 * B * H * W * 3,), dtype=torch.uint8, device="cuda").data_ptr()
    for args in ((s, s, None, r, m, c, B, H, W),  # dst == src
                 (big, big + 3, None, r, m, c, B, H, W), (big + 3, big, None, r, m, c, B, H, W),  # any overlap, either way round
                 (s, o, None, r, None, c, B, H, W), (s, o, None, r, m, None, B, H, W), (None, o, None, r, m, c, B, H, W), (s, None, None, r, m, c, B, H, W),
                 (s, o, None, r, m, c, B, H, 0), (s, o, None, r, m, c, B, 0, W), (s, o, None, r, m, c, 0, H, W), (s, o, None, r, m, c, -1, H, W),
                 (s, o, None, r, m + 4, c, B, H, W), (s, o, None, r + 2, m, c, B, H, W)):
        assert lib.gn_view_perturb(ctx, *args) != 0, args
        assert b"gn_view_perturb" in lib.gn_last_error()
    engine.synchronize()
    assert (out == 7).all() and (n == 7).all(), "a refused call wrote something"
