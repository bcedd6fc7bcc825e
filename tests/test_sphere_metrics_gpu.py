"""-m gpu: ``gn_openloop_sphere_metrics`` bit for bit against the int64 restatement (tests/sphere_metrics_ref.py: every column is an integer
sum, so there is no tolerance), known answers on discs, ``render.sphere_windows`` against what ``gn_render_spheres`` draws, and the refusals.

Shapes: tiled B = 3, V = 4, 20 x 20 with ``n_valid = 2``, ``row0 = 1``, ``rows = 4`` (marker rows around the scored ones); per-view B = 2, V = 2,
13 x 19 (W * 3 = 57 is no multiple of 4: rows start off the dword grid); S = 3 windows per view from three patterns that hold an interior
window, two overlapping ones, windows at each border, the whole image, single pixels and empty ones; thresholds 0 and 48."""
import numpy as np
import pytest
import torch

import openloop_ref as OR
import replay_render_ref as RR
import sphere_metrics_ref as SR
from genima_amd import render as R
from genima_amd.openloop import OpenLoopResult

pytestmark = pytest.mark.gpu

MARK = -0x0123456789ABCDEF


def _windows(B, V, H, W):
    patterns = [[(3, 4, 12, 11), (8, 6, 16, 12), (0, 0, 0, 0)],                      # interior; overlapping the first; empty
                [(W - 6, 0, W, 5), (5, 5, 6, 6), (0, H - 4, 7, H)],                  # top-right corner; one pixel; bottom-left corner
                [(0, 0, W, H), (2, 2, 2, 9), (W - 1, H - 1, W, H)]]                  # the whole image; zero width; the last pixel
    win = np.zeros((B * V, 3, 4), np.int32)
    for i in range(B * V):
        win[i] = patterns[i % 3]
    return win


def _images(B, V, H, W, seed, tiled):
    rng = np.random.RandomState(seed)
    gen = rng.randint(0, 256, (B, 2 * H, 2 * W, 3) if tiled else (B, V, H, W, 3)).astype(np.uint8)
    gt, cond = (rng.randint(0, 256, (B * V, H, W, 3)).astype(np.uint8) for _ in range(2))
    occ = (rng.randint(0, 3, (B * V, H, W)) == 0).astype(np.uint8) * rng.randint(1, 256, (B * V, H, W)).astype(np.uint8)  # any non-zero byte counts
    return gen, gt, cond, occ


def _ref(gen, gt, cond, occ, win, B, V, H, W, tiled, threshold):
    views = OR.untile(gen) if tiled else gen
    return SR.sphere_metrics(views, gt.reshape(B, V, H, W, 3), cond.reshape(B, V, H, W, 3), occ.reshape(B, V, H, W), win.reshape(B, V, -1, 4), threshold)


def _run(engine, gen, gt, cond, occ, win, rows, threshold, **kw):
    V = 4 if gen.ndim == 4 else gen.shape[1]
    out = torch.full((rows, V, win.shape[1], 17), MARK, dtype=torch.int64, device="cuda")
    engine.openloop_sphere_metrics(*(torch.from_numpy(a).cuda() for a in (gen, gt, cond, occ, win)), out, threshold=threshold, **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("threshold", [0, 48])
@pytest.mark.parametrize("B,V,H,W,tiled,row0,n_valid,rows", [(3, 4, 20, 20, True, 1, 2, 4), (2, 2, 13, 19, False, 0, 2, 2)])
def test_sphere_metrics_equal_the_int64_reference(engine, B, V, H, W, tiled, row0, n_valid, rows, threshold):
    gen, gt, cond, occ = _images(B, V, H, W, 23, tiled)
    win = _windows(B, V, H, W)
    want = _ref(gen, gt, cond, occ, win, B, V, H, W, tiled, threshold)
    assert (want[:, :, :, 1] > 0).any() and (want[..., 9] > 0).any() and (want[0, 0, 2] == 0).all()  # the inputs exercise the columns
    if threshold == 0:  # the two overlapping windows share pixels: each is summed on its own
        assert want[0, 0, 0, 0] == 9 * 7 and want[0, 0, 1, 0] == 8 * 6
    got = _run(engine, gen, gt, cond, occ, win, rows, threshold, row0=row0, n_valid=n_valid)
    assert np.array_equal(got[row0: row0 + n_valid], want[:n_valid])
    keep = np.ones(rows, bool)
    keep[row0: row0 + n_valid] = False
    assert (got[keep] == MARK).all()  # rows the call does not own, and the samples past n_valid, keep the marker
    assert np.array_equal(_run(engine, gen, gt, cond, occ, win, rows, threshold, row0=row0, n_valid=n_valid), got)  # a second run: the same bits
    assert np.array_equal(_run(engine, gen, gt, cond, occ, win, rows, threshold, row0=row0, n_valid=n_valid, win_host=win), got)  # ... also when checked
    assert (_run(engine, gen, gt, cond, occ, win, rows, threshold, row0=row0, n_valid=0) == MARK).all()  # n_valid = 0: accepted, writes nothing


def test_windows_the_host_never_saw_are_clamped(engine):
    """Without ``win_host`` the kernel clamps: x0 into [0, W], x1 into [x0, min(W, x0 + 256)], y likewise (include/genima_hip.h)."""
    B, V, H, W = 1, 2, 13, 19
    gen, gt, cond, occ = _images(B, V, H, W, 5, False)
    bad = np.array([[[-5, -7, 1000, 1000], [9, 8, 4, 3], [17, 11, 400, 12]], [[30, 30, 40, 40], [-9, -9, -1, -1], [0, 0, 19, 13]]], np.int32)
    same = np.array([[[0, 0, 19, 13], [9, 8, 9, 8], [17, 11, 19, 12]], [[19, 13, 19, 13], [0, 0, 0, 0], [0, 0, 19, 13]]], np.int32)
    assert np.array_equal(_run(engine, gen, gt, cond, occ, bad, B, 0), _ref(gen, gt, cond, occ, same, B, V, H, W, False, 0))


def _disc(H, W, cx, cy, r, colour, base):
    img = base.copy()
    y, x = np.mgrid[0:H, 0:W]
    mask = (x - cx) ** 2 + (y - cy) ** 2 <= r * r
    img[mask] = colour
    return img, mask


def _box5(img):
    p = np.pad(img.astype(np.int64), ((2, 2), (2, 2), (0, 0)))
    return (sum(p[dy: dy + img.shape[0], dx: dx + img.shape[1]] for dy in range(5) for dx in range(5)) // 25).astype(np.uint8)


@pytest.mark.parametrize("threshold", [0, 48])
def test_known_answers_on_discs(engine, threshold):
    """Four samples in one launch, one view, one window (4, 4, 36, 36) of a 40 x 40 image, a disc of radius 5 and colour (200, 100, 50) -- a
    mass of 350 - threshold per pixel over a black observation: 0 the disc moved by (3, -2); 1 the disc after a 5 x 5 box filter; 2 gen = cond
    over a random dark observation; 3 gen = gt over the same."""
    H = W = 40
    black = np.zeros((H, W, 3), np.uint8)
    dark = np.random.RandomState(1).randint(0, 40, (H, W, 3)).astype(np.uint8)
    gt0, mask = _disc(H, W, 18, 20, 5, (200, 100, 50), black)
    moved, _ = _disc(H, W, 21, 18, 5, (200, 100, 50), black)
    gtd, _ = _disc(H, W, 18, 20, 5, (200, 100, 50), dark)
    gen = np.stack([moved, _box5(gt0), dark, gtd])[:, None]
    gt = np.stack([gt0, gt0, gtd, gtd])
    cond = np.stack([black, black, dark, dark])
    occ = np.stack([mask.astype(np.uint8)] * 4)
    win = np.tile(np.array([4, 4, 36, 36], np.int32), (4, 1, 1))
    tab = _run(engine, gen, gt, cond, occ, win, 4, threshold)
    assert np.array_equal(tab, SR.sphere_metrics(gen, gt[:, None], cond[:, None], occ[:, None], win[:, None], threshold))
    res = OpenLoopResult(None, {}, [0] * 4, list(range(4)), [0] * 4, ["t"], ["cam"], 7, H, W, spheres=tab, windows=win[:, None])
    shift, mass, spread = res.sphere_shift()[:, 0, 0], res.sphere_mass_ratio()[:, 0, 0], res.sphere_spread_ratio()[:, 0, 0]
    ref = SR.derived(tab)
    print(f"threshold {threshold}: shift {shift}, mass ratio {mass}, spread ratio {spread}")
    assert abs(shift[0] - np.sqrt(13.0)) <= 1e-9 and mass[0] == 1.0 and abs(spread[0] - 1.0) <= 1e-12
    assert tab[0, 0, 0, 5] == mask.sum() * (350 - threshold) and tab[0, 0, 0, 9] == mask.sum() and tab[0, 0, 0, 0] == 32 * 32
    assert spread[1] > 1.0 and abs(mass[1] - ref["mass_ratio"][1, 0, 0]) <= 1e-9 and shift[1] < 0.1  # blurred: wider, where it was
    assert (tab[2, 0, 0, 1:5] == 0).all() and np.isnan(shift[2]) and mass[2] == 0.0 and tab[2, 0, 0, 5] > 0  # nothing generated
    assert np.array_equal(tab[3, 0, 0, 1:5], tab[3, 0, 0, 5:9]) and tab[3, 0, 0, 10] == 0 and np.array_equal(tab[3, 0, 0, 11:14], tab[3, 0, 0, 14:17])
    assert shift[3] == 0.0 and mass[3] == 1.0 and spread[3] == 1.0


@pytest.mark.parametrize("samples", [1, 4])
def test_windows_hold_what_the_renderer_draws(engine, samples):
    """One sphere per view at 32 x 32: fx = fy = 40, centre (16, 16), the camera at the origin looking along -z; radius 0.08 at depth 1 is 3.2
    px.  The window's centre is within 0.5 px of the projected centre (floor / ceil of u -+ h), the silhouette's centre within u_off (r / z)^2
    < 0.06 px of it, and a centroid of whole pixels adds well under the rest of the pixel the issue allows."""
    H = W = 32
    centres = [(0.0, 0.0, -1.0), (0.15, -0.1, -1.0), (-0.2, 0.2, -1.0), (0.1, 0.18, -1.0), (0.36, -0.3, -1.0), (0.0, 0.0, 1.0)]
    central = 4  # the first four lie within a quarter of the image of its centre; the fifth touches the border, the sixth is behind the camera
    B = len(centres)
    cams = np.zeros((B, 18), np.float32)
    cams[:, :4], cams[:, 16:] = (40, 40, 16, 16), (0.01, 3.0)
    cams[:, 4:16] = np.eye(3, 4).reshape(-1)
    sph = np.zeros((B, 1, 16), np.float32)
    sph[:, 0, :12] = np.eye(3, 4).reshape(-1)
    sph[:, 0, [3, 7, 11]] = centres
    sph[:, 0, 12], sph[:, 0, 13:] = 0.08, (1.0, 1.0, 0.0)  # the yellow factor: no drawn pixel is white
    views = {"cams": cams, "spheres": sph, "tex_index": np.zeros((B, 1), np.int32), "count": np.ones(B, np.int32)}
    occ = R.render_views(engine, views, R.load_atlas(RR.GOLDEN_SPHERES), H, W, samples, want=("occupied",))["occupied"].cpu().numpy() != 0
    win = R.sphere_windows(cams, sph, views["count"], H, W)
    assert win.shape == (B, 1, 4)
    for b in range(B):
        x0, y0, x1, y1 = win[b, 0]
        ys, xs = np.nonzero(occ[b])
        if b == B - 1:
            assert len(xs) == 0 and (win[b, 0] == 0).all()
            continue
        assert len(xs) >= 16, b  # a disc of 3.2 px
        assert xs.min() >= x0 and xs.max() < x1 and ys.min() >= y0 and ys.max() < y1, (b, win[b, 0])
        if b < central:
            cx, cy = xs.mean() + 0.5, ys.mean() + 0.5  # pixel x covers [x, x + 1)
            print(f"samples {samples} view {b}: window {win[b, 0]}, centre ({(x0 + x1) / 2}, {(y0 + y1) / 2}), occupied centroid ({cx:.3f}, {cy:.3f})")
            assert abs((x0 + x1) / 2 - cx) <= 1.0 and abs((y0 + y1) / 2 - cy) <= 1.0, b


def test_refused_arguments_leave_the_output_untouched(engine):
    lib, ctx = engine.lib, engine._ctx
    B, V, H, W, S = 1, 4, 300, 300, 2  # every buffer holds these shapes: a call accepted by mistake would still stay inside them
    gen, gt, cond = (torch.zeros(B * V * H * W * 3, dtype=torch.uint8, device="cuda") for _ in range(3))
    occ = torch.zeros(B * V * H * W, dtype=torch.uint8, device="cuda")
    win_h = np.tile(np.array([[0, 0, 8, 8], [290, 290, 300, 300]], np.int32), (B * V, 1, 1))
    win = torch.zeros(B * V * S * 4 + 4, dtype=torch.int32, device="cuda")
    win[: B * V * S * 4] = torch.from_numpy(win_h.reshape(-1)).cuda()
    out = torch.full((B * V * S * 17 + 2,), MARK, dtype=torch.int64, device="cuda")
    ok = dict(gen=gen.data_ptr(), gt=gt.data_ptr(), cond=cond.data_ptr(), occ=occ.data_ptr(), win=win.data_ptr(), host=None, out=out.data_ptr(), B=B, V=V, H=H,
              W=W, S=S, tiled=1, thr=30, row0=0, n_valid=B, rows=B)

    def call(a):
        return lib.gn_openloop_sphere_metrics(ctx, a["gen"], a["gt"], a["cond"], a["occ"], a["win"], a["host"], a["out"], a["B"], a["V"], a["H"], a["W"], a["S"],
                                              a["tiled"], a["thr"], a["row0"], a["n_valid"], a["rows"])

    bad = [dict(gen=None), dict(gt=None), dict(cond=None), dict(occ=None), dict(win=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(S=0),
           dict(S=9), dict(thr=-1), dict(V=3), dict(V=5), dict(n_valid=-1), dict(n_valid=B + 1), dict(row0=-1), dict(row0=1), dict(rows=0),
           dict(win=win.data_ptr() + 2), dict(out=out.data_ptr() + 4)]
    for first in ([0, 0, 257, 2], [0, 0, 2, 257], [290, 0, 301, 4], [0, 290, 4, 301], [-1, 0, 3, 3], [0, -1, 3, 3], [5, 0, 3, 4], [0, 5, 4, 3]):
        h = win_h.copy()
        h[B * V - 1, S - 1] = first  # the last window of the table
        bad.append(dict(host=h))
    for change in bad:
        a = dict(ok, **change)
        if isinstance(a["host"], np.ndarray):
            a["host"] = a["host"].ctypes.data
        assert call(a) != 0, change
    torch.cuda.synchronize()
    assert bool((out == MARK).all())
    # ... and the unchanged arguments are accepted, with and without the host copy
    assert call(ok) == 0 and call(dict(ok, host=win_h.ctypes.data)) == 0
    torch.cuda.synchronize()
    got = out[: B * V * S * 17].view(B, V, S, 17).cpu().numpy()
    assert (got[..., 0] == [64, 100]).all() and (got[..., 1:] == 0).all() and bool((out[B * V * S * 17:] == MARK).all())
    from genima_amd.engine import Engine

    rec = Engine("cuda:0", record=True)
    with pytest.raises(RuntimeError, match="eager"):
        rec.openloop_sphere_metrics(gen.view(B, 2 * H, 2 * W, 3), gt.view(B * V, H, W, 3), cond.view(B * V, H, W, 3), occ.view(B * V, H, W),
                                    win[: B * V * S * 4].view(B * V, S, 4), out[: B * V * S * 17].view(B, V, S, 17))
