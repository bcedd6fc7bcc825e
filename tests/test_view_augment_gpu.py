"""-m gpu: ``gn_view_augment_tiled`` and the loader path around it (``DataLoader(view_augment=...)``).

Kernel.  Every tile of a 2 x 2 tiled frame is an independent view: the reference is tests/perturb_ref.py's ``view_perturb`` (the numpy f64
restatement of ``gn_view_perturb``'s pixel rule) on the untiled views, put back into the tiling in numpy -- ``dst``, ``valid`` and
``n_revealed`` bit for bit, and ``dst_f16`` against ``Engine.image_u8_to_f16`` of ``dst``, bit for bit.  No tolerance anywhere.

Shapes.  A: n = 3 frames of 37 x 53 tiles (tiled 74 x 106, rows of 318 bytes): an odd frame count, H != W, the right-hand tiles start 159
bytes into a row and so fall into another alignment class than the left-hand ones, one-pixel tails, three workgroups per tile.  B: n = 2
frames of 64 x 64 tiles, everything dword-aligned.  The (frame, tile) pairs cycle through five kinds, as tests/test_view_perturb_gpu.py's
views do: the identity; an integer shift; a rotation with zoom that leaves all four edges; a zoom-out of 4 that reaches the clamp after the
one reflection; an M whose w changes sign inside the tile.  The colour rows cycle with them: a gain that saturates, an offset that clamps at 0.
Both source forms: ``src`` stacked, and ``frames`` -- a pointer table into a larger buffer where the frames lie in reverse order, 4- but not
8-byte aligned, with one pointer repeated.

Loader.  The 256^2 synthetic episode of tests/test_render_gpu.py: the batches are recomputed outside the loader from the clean PNG tiles, the
batch's own tables, the numpy reference and ``Engine.render_spheres``."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import perturb_ref as PR
from genima_amd import data as D
from genima_amd import perturb as P
from genima_amd import render as R
from genima_amd._lib import GenimaHipError
from genima_amd.pipeline import HashTokenizer

pytestmark = pytest.mark.gpu

TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_textures")
COLOURS = np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0], [0.5, 1.5, 1.0, 0.0, 0.5, -0.5], [2.2, 1.0, 0.7, 0.0, -90.0, 10.0], [1.0, 0.9, 1.1, 0.5, 0.25, -0.75],
                    [0.9, 1.1, 1.0, 3.0, -3.0, 0.0]])


def untile(x):
    """[n, 2H, 2W, ...] -> [n * 4, H, W, ...]: tile t of a frame sits at tile row t // 2, tile column t % 2."""
    n, H, W = x.shape[0], x.shape[1] // 2, x.shape[2] // 2
    return np.stack([x[i, (t >> 1) * H:(t >> 1) * H + H, (t & 1) * W:(t & 1) * W + W] for i in range(n) for t in range(4)])


def retile(v):
    """The inverse of ``untile``."""
    n, H, W = v.shape[0] // 4, v.shape[1], v.shape[2]
    out = np.zeros((n, 2 * H, 2 * W) + v.shape[3:], v.dtype)
    for b in range(4 * n):
        i, t = divmod(b, 4)
        out[i, (t >> 1) * H:(t >> 1) * H + H, (t & 1) * W:(t & 1) * W + W] = v[b]
    return out


def reference(src, M, colour):
    """Tiled uint8 [n, 2H, 2W, 3], M [n, 4, 9], colour [n, 4, 6] -> (dst tiled, valid tiled, n_revealed [n, 4]) by the numpy rule per tile."""
    n = src.shape[0]
    dst, valid, rev = PR.view_perturb(untile(src), M.reshape(n * 4, 9), colour.reshape(n * 4, 6))
    return retile(dst), retile(valid), rev.reshape(n, 4)


def _about_centre(A, H, W):
    c = np.array([W / 2.0, H / 2.0])
    M = np.eye(3)
    M[:2, :2], M[:2, 2] = A, c - A @ c
    return M.reshape(9)


def _kinds(H, W):
    a = np.deg2rad(20.0)
    return [np.eye(3).reshape(9), np.array([1.0, 0, 5, 0, 1, -3, 0, 0, 1]),
            _about_centre(1.25 * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]), H, W), _about_centre(4.0 * np.eye(2), H, W),
            np.array([1.0, 0, 0, 0, 1, 0, -1.0 / (0.47 * W), 0.01, 1.0])]


def _case(n, H, W, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (n, 2 * H, 2 * W, 3)).astype(np.uint8)
    kinds = _kinds(H, W)
    M = np.stack([kinds[b % 5] for b in range(4 * n)]).reshape(n, 4, 9)
    colour = np.stack([COLOURS[b % 5] for b in range(4 * n)]).reshape(n, 4, 6)
    return src, M, colour


@pytest.fixture(scope="module", params=[(3, 37, 53), (2, 64, 64)], ids=["A-3x37x53", "B-2x64x64"])
def case(request):
    n, H, W = request.param
    src, M, colour = _case(n, H, W, seed=n)
    return dict(n=n, H=H, W=W, src=src, M=M, colour=colour, want=reference(src, M, colour))  # the reference once per shape


def test_the_cases_reach_what_they_are_there_for(case):
    """On the reference alone: the properties the docstring lists are really in these inputs, every kind in at least one tile."""
    n, H, W = case["n"], case["H"], case["W"]
    dst, valid, rev = (untile(a) if a.ndim > 2 else a.reshape(-1) for a in case["want"])
    src, M = untile(case["src"]), case["M"].reshape(-1, 9)
    assert 4 * n >= 5
    assert np.array_equal(dst[0], src[0]) and valid[0].all() and rev[0] == 0  # the identity: a copy
    assert rev[1] == H * W - (H - 3) * (W - 5) and (dst[1, ..., 1] == 255).any()  # the shift reveals its border; a gain that saturates
    assert (dst[2, ..., 0] == 255).any() and (dst[2, ..., 1] == 0).any()  # an offset that clamps at 0
    inv = valid[2] == 0
    assert inv[0].any() and inv[-1].any() and inv[:, 0].any() and inv[:, -1].any() and valid[2].any()  # all four edges left
    X = np.array([0.5, W - 0.5])
    u = M[3][0] * X + M[3][2]
    assert u[0] - 0.5 < -(W - 1) and u[1] - 0.5 > 2 * (W - 1)  # the clamp is reached beyond the one reflection
    Y, Xg = np.mgrid[0:H, 0:W] + 0.5
    w = (M[4][6] * Xg + M[4][7] * Y) + M[4][8]
    assert (w > 0).any() and (w <= 0).any() and not dst[4][w <= 0].any() and not valid[4][w <= 0].any() and valid[4].any()  # the sign change is inside
    assert (rev[1:5] > 0).all() and rev.tolist() == (valid == 0).reshape(4 * n, -1).sum(axis=1).tolist()
    assert ((W * 3) % 4 != 0) == (W == 53)  # case A's right-hand tiles are in another alignment class


def _scattered(src):
    """The frames in a larger device buffer: in reverse order with gaps between them, each 4- but not 8-byte aligned; the last pointer
    repeats the first.  -> (buffer, device int64 pointer table, the frame each pointer names)."""
    n, fb = src.shape[0], src[0].size
    pitch = (fb + 15) // 8 * 8  # a multiple of 8 with a gap of 8 .. 15 bytes: every frame starts 4 bytes past an 8-byte boundary
    buf = torch.full((4 + n * pitch + 64,), 201, dtype=torch.uint8, device="cuda")
    off = [4 + (n - 1 - k) * pitch for k in range(n)]
    for k in range(n):
        buf[off[k]:off[k] + fb] = torch.from_numpy(src[k].reshape(-1)).cuda()
    order = list(range(n))
    order[-1] = 0
    addr = [buf.data_ptr() + off[k] for k in order]
    assert all(a % 4 == 0 and a % 8 != 0 for a in addr)
    return buf, torch.tensor(addr, dtype=torch.int64, device="cuda"), order


@pytest.mark.parametrize("form", ["src", "frames"])
def test_bits_equal_the_reference(engine, case, form):
    n, H, W = case["n"], case["H"], case["W"]
    M, colour = torch.from_numpy(case["M"]).cuda(), torch.from_numpy(case["colour"]).cuda()
    if form == "src":
        src = torch.from_numpy(case["src"]).cuda()
        source, keep, (want_dst, want_valid, want_n) = dict(src=src), src.clone(), case["want"]
    else:
        buf, ptrs, order = _scattered(case["src"])
        source, keep = dict(frames=ptrs), buf.clone()
        want_dst, want_valid, want_n = case["want"] if order == list(range(n)) else reference(case["src"][order], case["M"], case["colour"])
    tiled = (n, 2 * H, 2 * W)
    valid = torch.full(tiled, 9, dtype=torch.uint8, device="cuda")
    rev = torch.full((n, 4), -5, dtype=torch.int32, device="cuda")
    f16 = torch.full(tiled + (8,), 3.0, dtype=torch.float16, device="cuda")
    dst, got_f16 = engine.view_augment_tiled(M, colour, H, W, out_f16=f16, out_u8=torch.full(tiled + (3,), 77, dtype=torch.uint8, device="cuda"),
                                             scale=(1.0, 0.0), valid=valid, n_revealed=rev, **source)
    got = dst.cpu().numpy()
    bad = int((got != want_dst).sum())
    print(f"{form} {n} x {2 * H} x {2 * W}: {bad} of {got.size} bytes differ from the reference; revealed {rev.cpu().numpy().tolist()}")
    assert got_f16 is f16 and got.shape == tiled + (3,) and bad == 0
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    assert rev.cpu().numpy().tolist() == want_n.tolist()
    assert torch.equal(keep, source["src"] if form == "src" else buf), "the source was written"
    assert torch.equal(f16.view(torch.int16), engine.image_u8_to_f16(dst, 8, 1.0, 0.0).view(torch.int16))
    # the f16 output alone (no dst), at the target's scale; a second run gives the same bits and counts (zeroed by the call, not accumulated)
    _, f2 = engine.view_augment_tiled(M, colour, H, W, out_f16=torch.full(tiled + (8,), 3.0, dtype=torch.float16, device="cuda"), scale=(2.0, -1.0),
                                      n_revealed=rev, **source)
    assert torch.equal(f2.view(torch.int16), engine.image_u8_to_f16(dst, 8, 2.0, -1.0).view(torch.int16))
    assert rev.cpu().numpy().tolist() == want_n.tolist()
    only_u8, none = engine.view_augment_tiled(M, colour, H, W, **source)  # with no output named, the uint8 one is allocated
    assert none is None and torch.equal(only_u8, dst)


def test_the_identity_is_a_copy_and_the_plain_conversion(engine):
    n, H, W = 2, 37, 53
    src = torch.from_numpy(_case(n, H, W, seed=5)[0]).cuda()
    M = torch.from_numpy(np.tile(np.eye(3).reshape(9), (n, 4, 1))).cuda()
    colour = torch.from_numpy(np.tile(COLOURS[0], (n, 4, 1))).cuda()
    rev = torch.full((n, 4), 1, dtype=torch.int32, device="cuda")
    dst, f16 = engine.view_augment_tiled(M, colour, H, W, src=src, out_u8=torch.empty_like(src), n_revealed=rev,
                                         out_f16=torch.empty((n, 2 * H, 2 * W, 8), dtype=torch.float16, device="cuda"))
    assert torch.equal(dst, src) and not rev.any()
    assert torch.equal(f16.view(torch.int16), engine.image_u8_to_f16(src, 8, 1.0, 0.0).view(torch.int16))


def test_no_sample_reads_a_neighbouring_tile(engine):
    """Four tiles of constant, distinct colours and a shift larger than the tile in each of the four directions (one frame each), then the
    zoom-out that reaches the clamp and the projective kind: every output byte is its own tile's colour, or black."""
    H, W = 10, 14
    tile_colour = np.array([[250, 10, 20], [30, 240, 40], [50, 60, 230], [200, 210, 90]], np.uint8)
    kinds = _kinds(H, W)
    mats = [np.array([1.0, 0, sx, 0, 1, sy, 0, 0, 1]) for sx, sy in ((W + 3.5, 0), (-W - 3.5, 0), (0, H + 2.5), (0, -H - 2.5), (2 * W + 0.25, -2 * H - 0.25))] + kinds[3:]
    n = len(mats)
    src = retile(np.broadcast_to(np.tile(tile_colour, (n, 1))[:, None, None, :], (4 * n, H, W, 3)).copy())
    M = np.stack([np.tile(m, (4, 1)) for m in mats])
    colour = np.tile(COLOURS[0], (n, 4, 1))
    want, want_valid, _ = reference(src, M, colour)
    assert (want_valid[:5] == 0).all()  # every sample of the five shifts lies outside its tile
    dst, _ = engine.view_augment_tiled(torch.from_numpy(M).cuda(), torch.from_numpy(colour).cuda(), H, W, src=torch.from_numpy(src).cuda())
    got = untile(dst.cpu().numpy())
    for b in range(4 * n):
        own = (got[b] == tile_colour[b % 4]).all(axis=-1) | (got[b] == 0).all(axis=-1)
        assert own.all(), (b, got[b][~own][:4])
    assert np.array_equal(dst.cpu().numpy(), want)


def test_refusals(engine):
    """Argument checks only: every call below is refused before a launch and the outputs stay as they were."""
    n, H, W = 2, 8, 12
    src, M, colour = (torch.from_numpy(a).cuda() for a in _case(n, H, W, seed=1))
    tiled = (n, 2 * H, 2 * W)
    out = torch.full(tiled + (3,), 7, dtype=torch.uint8, device="cuda")
    f16 = torch.full(tiled + (8,), 7.0, dtype=torch.float16, device="cuda")
    valid = torch.full(tiled, 7, dtype=torch.uint8, device="cuda")
    rev = torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
    ptrs = torch.tensor([src.data_ptr(), src[1].data_ptr()], dtype=torch.int64, device="cuda")
    good = dict(M=M, colour=colour, src=src, frames=None, out_u8=out, out_f16=f16, valid=valid, n_revealed=rev)
    for bad in (dict(frames=ptrs), dict(src=None), dict(out_u8=src), dict(M=None), dict(colour=None), dict(M=M.float()), dict(M=M[:1]), dict(M=M.view(n * 4, 9)),
                dict(colour=colour[..., :5].contiguous()), dict(src=src.cpu()), dict(src=src[:, :, : 2 * W - 1].contiguous()), dict(src=None, frames=ptrs.int()),
                dict(src=None, frames=ptrs[:1]), dict(out_u8=out[:1]), dict(out_f16=f16.float()), dict(out_f16=f16[..., :4].contiguous()),
                dict(n_revealed=rev.long()), dict(n_revealed=rev.view(-1)), dict(valid=valid[..., None]), dict(scale=(float("inf"), 0.0)),
                dict(scale=(1.0, float("nan")))):
        a = dict(good, **bad)
        with pytest.raises(GenimaHipError):
            engine.view_augment_tiled(a.pop("M"), a.pop("colour"), H, W, **a)
    lib, ctx = engine.lib, engine._ctx
    s, p, o, h, v, r, m, c = (t.data_ptr() for t in (src, ptrs, out, f16, valid, rev, M, colour))
    big = torch.zeros((2 * src.numel(),), dtype=torch.uint8, device="cuda").data_ptr()
    for args in ((None, s, None, o, h, v, r, m, c, n, H, W, 1.0, 0.0),  # a NULL ctx
                 (ctx, s, None, o, h, v, r, None, c, n, H, W, 1.0, 0.0), (ctx, s, None, o, h, v, r, m, None, n, H, W, 1.0, 0.0),
                 (ctx, s, p, o, h, v, r, m, c, n, H, W, 1.0, 0.0), (ctx, None, None, o, h, v, r, m, c, n, H, W, 1.0, 0.0),  # both sources, neither
                 (ctx, s, None, None, None, v, r, m, c, n, H, W, 1.0, 0.0),  # no output
                 (ctx, s, None, o, h, v, r, m, c, 0, H, W, 1.0, 0.0), (ctx, s, None, o, h, v, r, m, c, -1, H, W, 1.0, 0.0),
                 (ctx, s, None, o, h, v, r, m, c, n, 0, W, 1.0, 0.0), (ctx, s, None, o, h, v, r, m, c, n, H, 0, 1.0, 0.0),
                 (ctx, s, None, o, h, v, r, m, c, 16384, 1, 1, 1.0, 0.0),  # 4 n = 65536
                 (ctx, s, None, o, h, v, r, m, c, 1, 13378, 13378, 1.0, 0.0),  # 4 * 13378^2 * 3 = 2 147 650 608 >= 2^31
                 (ctx, s, None, o, h, v, r, m + 4, c, n, H, W, 1.0, 0.0), (ctx, s, None, o, h, v, r, m, c + 4, n, H, W, 1.0, 0.0),
                 (ctx, s, None, o, h, v, r + 2, m, c, n, H, W, 1.0, 0.0), (ctx, s, None, o, h + 8, v, r, m, c, n, H, W, 1.0, 0.0),
                 (ctx, s, None, s, h, v, r, m, c, n, H, W, 1.0, 0.0),  # dst == src
                 (ctx, big, None, big + 3, h, v, r, m, c, n, H, W, 1.0, 0.0), (ctx, big + 3, None, big, h, v, r, m, c, n, H, W, 1.0, 0.0),  # any overlap
                 (ctx, s, None, o, h, v, r, m, c, n, H, W, float("inf"), 0.0), (ctx, s, None, o, h, v, r, m, c, n, H, W, 1.0, float("nan"))):
        assert lib.gn_view_augment_tiled(*args) != 0, args
        assert b"gn_view_augment_tiled" in lib.gn_last_error()
    engine.synchronize()
    assert (out == 7).all() and (f16 == 7.0).all() and (valid == 7).all() and (rev == 7).all(), "a refused call wrote something"
    engine.record = True  # a recording engine refuses the op before anything else
    try:
        with pytest.raises(RuntimeError, match="eager op"):
            engine.view_augment_tiled(M, colour, H, W, src=src)
    finally:
        engine.record = False


# ---- the loader ----
BOTH = "camera_pose+light_color"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The 256^2 synthetic episode (L = 6) as a tree of ``tiled_rgb`` frames and ``traj.npz``, as ``render_episode`` lays them out: the
    targets are drawn by the loader, so no rendered PNG is needed.  -> (dataset, RenderConfig, clean tiled frames uint8 [4, 512, 512, 3])."""
    root = str(tmp_path_factory.mktemp("view_augment_gpu"))
    cfg, traj, frames = R.synthetic_episode(6, 7, TEXTURES)
    base = os.path.join(root, "open_box", "variation0")
    ep = os.path.join(base, "episodes", "episode0")
    os.makedirs(os.path.join(ep, "tiled_rgb"))
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["open the box"], f)
    tiles = R.tile_cameras(cfg.cameras)
    clean = [R._tile([frames[c][ts] for c in tiles]) for ts in range(5)]
    for ts, im in enumerate(clean):
        Image.fromarray(im).save(os.path.join(ep, "tiled_rgb", f"{ts}.png"))
    R.save_traj(os.path.join(ep, "traj.npz"), traj)
    ds = D.RLBenchDataset(root, tasks="open_box", num_demos=1, image_type="tiled_rgb", conditioning_image_type="tiled_rgb")
    assert len(ds) == 4 and [e["conditioning_image"] for e in ds.examples] == [os.path.join(ep, "tiled_rgb", f"{i}.png") for i in range(4)]
    return ds, cfg, np.stack(clean[:4])


def _loader(tree, **kw):
    ds, cfg, _ = tree
    return D.DataLoader(ds, 3, HashTokenizer(1024), 512, seed=1, render_targets=R.TrajectorySource(cfg), **kw)


def _first(engine, loader):
    """-> (dataset indices of the first batch of the loader's next epoch, its host batch, its device batch)."""
    ix = loader._batches()[0]
    host = next(iter(loader))
    return ix, host, D.to_device(engine, host)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("kw,cache", [(dict(view_augment=P.Perturbation()), "device"), (dict(view_augment="camera_pose", view_augment_prob=0.0), None)],
                         ids=["identity", "prob0"])
def test_loader_identity_and_prob_zero_are_the_loader_without_the_argument(engine, tree, kw, cache):
    plain, aug = _loader(tree, cache=cache), _loader(tree, cache=cache, **kw)
    for _ in range(2):
        for a, b in zip(plain, aug):
            assert "M" in b["render_views"] and "M" not in a["render_views"]
            a, b = D.to_device(engine, a), D.to_device(engine, b)
            assert set(b) == set(a) | {"view_revealed"} and not b["view_revealed"].any()
            assert _same(a["pixel_values"], b["pixel_values"]) and _same(a["conditioning_pixel_values"], b["conditioning_pixel_values"])
            assert torch.equal(a["input_ids"], b["input_ids"])


@pytest.fixture(scope="module")
def recomputed():
    return {}  # epoch -> the first batch recomputed outside the loader, shared by the two cache settings


@pytest.mark.parametrize("cache", [None, "device"])
def test_loader_batches_equal_the_recomputation_outside_it(engine, tree, recomputed, cache):
    ds, cfg, clean = tree
    loader, second = _loader(tree, cache=cache, view_augment=BOTH, prefetch=0), _loader(tree, cache=cache, view_augment=BOTH, prefetch=0)
    seen = []
    for epoch in range(2):
        ix, host, dev = _first(engine, loader)
        v = host["render_views"]
        M, colour, cams = v["M"].numpy(), v["colour"].numpy(), v["cams"].numpy()
        B = len(ix)
        assert B == 3 and M.shape == (B, 4, 9) and dev["view_revealed"].shape == (B, 4) and dev["view_revealed"].dtype == torch.int32
        if epoch not in recomputed:
            names = R.tile_cameras(cfg.cameras)
            src = R.TrajectorySource(cfg)
            for k, i in enumerate(ix):  # the tables are the draw of (seed, epoch, dataset index)
                want = P.sample_tables(P.parse(BOTH), np.stack([w[0] for w in src.views(ds.examples[i]["conditioning_image"])]), names, (1, epoch, i))
                assert np.array_equal(want[0], cams[4 * k:4 * k + 4]) and np.array_equal(want[1], M[k]) and np.array_equal(want[2], colour[k])
            frames, _, rev = reference(clean[ix], M, colour)
            bg = torch.from_numpy(frames).cuda()
            px = torch.empty((B, 512, 512, 8), dtype=torch.float16, device="cuda")
            engine.render_spheres(*(v[k].cuda() for k in ("cams", "spheres", "tex_index", "count")), src.atlas_on("cuda"), 256, 256, cfg.samples, bg=bg,
                                  bg_tiled=True, n_tiled=B, full_f16=px, full_scale=(2.0, -1.0))
            recomputed[epoch] = dict(ix=ix, cond=engine.image_u8_to_f16(bg, 8, 1.0, 0.0), px=px, rev=rev, frames=frames)
        want = recomputed[epoch]
        assert ix == want["ix"]
        assert _same(dev["conditioning_pixel_values"], want["cond"]) and _same(dev["pixel_values"], want["px"])
        assert dev["view_revealed"].cpu().numpy().tolist() == want["rev"].tolist()
        share = want["rev"] / (256.0 * 256.0)
        print(f"cache={cache} epoch {epoch}: samples {ix}, revealed share per (sample, view) {np.round(share, 4).tolist()}")
        assert (want["rev"][:, 0] == 0).all() and (want["rev"][:, 1:] > 0).all()  # the preset leaves the wrist alone and turns the others
        assert not np.array_equal(want["frames"], clean[ix])  # warped
        assert not _same(want["px"], engine.image_u8_to_f16(torch.from_numpy(want["frames"]).cuda(), 8, 2.0, -1.0))  # and spheres were drawn over it
        _, _, dev2 = _first(engine, second)  # a second loader repeats the first one's bits
        assert _same(dev2["pixel_values"], dev["pixel_values"]) and _same(dev2["conditioning_pixel_values"], dev["conditioning_pixel_values"])
        assert torch.equal(dev2["view_revealed"], dev["view_revealed"])
        seen.append((ix, M.copy(), dev["conditioning_pixel_values"]))
    both = sorted(set(seen[0][0]) & set(seen[1][0]))  # the two epochs draw differently for the same sample
    assert both and all(not np.array_equal(seen[0][1][seen[0][0].index(i)], seen[1][1][seen[1][0].index(i)]) for i in both)
    assert all(not _same(seen[0][2][seen[0][0].index(i)], seen[1][2][seen[1][0].index(i)]) for i in both)


def test_loader_wrist_tile_is_the_clean_tile_where_the_light_is_off(engine, tree):
    _, _, clean = tree
    ix, host, dev = _first(engine, _loader(tree, view_augment="camera_pose", prefetch=0))
    want = engine.image_u8_to_f16(torch.from_numpy(clean[ix]).cuda(), 8, 1.0, 0.0)
    got = dev["conditioning_pixel_values"]
    assert _same(got[:, :256, :256].contiguous(), want[:, :256, :256].contiguous())
    for rows, cols in ((slice(0, 256), slice(256, 512)), (slice(256, 512), slice(0, 256)), (slice(256, 512), slice(256, 512))):
        assert not _same(got[:, rows, cols].contiguous(), want[:, rows, cols].contiguous())
    assert not dev["view_revealed"][:, 0].any() and (dev["view_revealed"][:, 1:] > 0).all()


def test_train_step_takes_view_augmented_batches(engine, tree):
    """Two epochs of augmented batches through the tiny family's fine-tune: finite losses, the same sequence in a second run, another
    sequence than the un-augmented loader's, and a run with ``sphere_loss_weight`` completes."""
    from genima_amd import configs, schema, weights
    from genima_amd.packing import pack_state_dict
    from genima_amd.scheduler import DDPMScheduler
    from genima_amd.training import ControlNetTrainer

    ds, cfg, _ = tree
    fam = configs.family("tiny")
    tok = HashTokenizer(fam["text"]["vocab_size"])

    def run(epochs=2, frozen=None, **kw):
        synth = lambda sch, s: weights.synth_state_dict(sch, s)  # noqa: E731
        tr = ControlNetTrainer(engine, fam["unet"], fam["controlnet"], pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), "cuda"),
                               synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-4)
        tr.attach_frozen(fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), "cuda"), fam["text"],
                         pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), "cuda"), DDPMScheduler(), seed=5, augmentations="crop,colorjitter",
                         **(frozen or {}))
        loader = D.DataLoader(ds, 2, tok, 512, shuffle=True, seed=0, render_targets=R.TrajectorySource(cfg), cache="device", **kw)
        return [float(tr.train_step(batch)) for _ in range(epochs) for batch in loader]

    aug = run(view_augment=BOTH)
    print("augmented losses", aug)
    assert len(aug) == 4 and all(np.isfinite(aug)) and len(set(aug)) > 1
    assert run(view_augment=BOTH) == aug
    plain = run()
    print("un-augmented losses", plain)
    assert all(np.isfinite(plain)) and plain != aug
    weighted = run(epochs=1, frozen=dict(sphere_loss_weight=2.0), view_augment=BOTH)
    assert len(weighted) == 2 and all(np.isfinite(weighted))
