"""-m "not gpu": known answers on the float64 restatement of the sphere renderer (tests/render_reference.py) and on the host-side setup
of genima_amd/render.py (extrinsic flip, texture / factor selection, the horizon window, the tile order, the ABI binding)."""
import ctypes
import os

import numpy as np
import pytest

import render_reference as ref
from genima_amd import _lib, tiling
from genima_amd import render as R

TEXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_textures")
H = W = 64


def _cam(fx=100.0, fy=100.0, cx=31.3, cy=33.6, znear=1e-5, zfar=3.0, pose=None):
    cam = np.zeros(18)
    cam[:4] = fx, fy, cx, cy
    cam[4:16] = (np.eye(4)[:3] if pose is None else pose).reshape(-1)
    cam[16:] = znear, zfar
    return cam


def _sphere(c, r=0.05, factor=(1.0, 1.0, 1.0), rot=None):
    s = np.zeros(16)
    P = np.eye(4)[:3]
    if rot is not None:
        P[:, :3] = rot
    P[:, 3] = c
    s[:12], s[12], s[13:] = P.reshape(-1), r, factor
    return s


def _flat(rgb, n=4):
    a = np.zeros((1, n, n, 4), np.uint8)
    a[..., :3], a[..., 3] = rgb, 255
    return a


def _draw(cam, spheres, atlas, tex=None, samples=1):
    sp = np.stack(spheres)
    return ref.render(cam, sp, np.arange(len(spheres)) if tex is None else tex, len(spheres), atlas, H, W, samples)[0]


def test_symbol_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "gn_render_spheres" in _lib.SIGNATURES and hasattr(lib, "gn_render_spheres")
    assert ctypes.sizeof(_lib.RenderDesc) == 15 * 8 + 10 * 4 + 4 * 4  # 15 pointers, 10 int32, 4 float: no padding
    assert int(lib.gn_render_spheres(None, None)) != 0  # refused, not launched


@pytest.mark.parametrize("samples", [1, 4])
def test_sphere_on_the_axis_is_centred_with_radius_f_r_over_d(samples):
    d, r = 0.8, 0.05
    img = _draw(_cam(), [_sphere((0, 0, -d), r)], _flat((200, 10, 10)), samples=samples)
    ys, xs = np.nonzero(np.any(img != 255, -1))
    assert abs(xs.mean() + 0.5 - 31.3) < 0.5 and abs(ys.mean() + 0.5 - 33.6) < 0.5
    want = 100.0 * r / d
    assert abs((xs.max() - xs.min() + 1) / 2 - want) <= 1 and abs((ys.max() - ys.min() + 1) / 2 - want) <= 1
    assert tuple(img[33, 31]) == (200, 10, 10)  # factor 1 x a flat texture


def test_negative_focal_lengths_mirror_both_axes():
    s = [_sphere((0.1, 0.05, -0.8), 0.03)]
    pos = _draw(_cam(cx=32, cy=32), s, _flat((0, 0, 0)))
    neg = _draw(_cam(fx=-100.0, fy=-100.0, cx=32, cy=32), s, _flat((0, 0, 0)))
    ys, xs = np.nonzero(np.any(pos != 255, -1))
    assert xs.mean() > 40 and ys.mean() < 28  # +x right, +y up
    assert np.array_equal(neg, pos[::-1, ::-1])


def test_beyond_zfar_or_behind_the_camera_draws_nothing():
    for c in ((0, 0, -3.5), (0, 0, 0.8)):
        assert np.all(_draw(_cam(), [_sphere(c, 0.05)], _flat((0, 0, 0))) == 255)
    assert np.any(_draw(_cam(), [_sphere((0, 0, -2.9), 0.05)], _flat((0, 0, 0))) != 255)
    assert np.all(_draw(_cam(znear=1.0), [_sphere((0, 0, -0.8), 0.05)], _flat((0, 0, 0))) == 255)  # nearer than znear


def test_the_nearer_of_two_overlapping_spheres_wins():
    atlas = np.concatenate([_flat((255, 0, 0)), _flat((0, 0, 255))])
    far, near = _sphere((0, 0, -1.0), 0.05), _sphere((0.02, 0, -0.7), 0.03)
    for order, tex in (([far, near], [0, 1]), ([near, far], [1, 0])):
        img = _draw(_cam(cx=32, cy=32), order, atlas, tex=np.array(tex))
        assert tuple(img[32, 34]) == (0, 0, 255)  # where both cover: the near, blue one
        assert tuple(img[32, 28]) == (255, 0, 0)  # only the far, red one


def test_texture_orientation_and_bottom_row_origin():
    # an asymmetric 4 x 4 texture: every texel its own colour, image row 0 = top
    tex = np.zeros((1, 4, 4, 4), np.uint8)
    for j in range(4):
        for i in range(4):
            tex[0, j, i] = (40 * i + 20, 40 * j + 20, 7, 255)
    d, r = 0.5, 0.1  # 20 px radius
    img = _draw(_cam(cx=32, cy=32), [_sphere((0, 0, -d), r)], tex)

    def at(lx, ly):  # the pixel that sees the sphere's local (lx, ly) r (front side), by the pinhole with the hit's depth
        z = -d + r * np.sqrt(1 - lx * lx - ly * ly)
        return img[int(np.floor(32 - 100 * (ly * r) / -z)), int(np.floor(32 + 100 * (lx * r) / -z))]

    # uv = (p.xy / r + 1) / 2: u grows with the sphere's +x (image right), v with +y (image up); v = 0 is the texture's BOTTOM row
    right, left, up, down = at(0.62, 0.0), at(-0.62, 0.0), at(0.0, 0.62), at(0.0, -0.62)
    assert right[0] > left[0] + 60 and abs(int(right[1]) - int(left[1])) < 5
    assert down[1] > up[1] + 60  # low v reads the bottom rows = high image-row index = larger green
    # texel centres: u = 0.625 -> x = 2.0 -> texel column 2; v = 0.375 -> y = 1.0 -> row 1 from the bottom = image row 2 (a top-row origin
    # would read image row 1, green 60).  The pixel's centre lies within half a pixel = 0.05 texel of that point, and the texture changes by
    # 40 per texel there (no wrap edge nearby): within 2 of the texel's colour
    def near(px, want):
        return abs(int(px[0]) - want[0]) <= 2 and abs(int(px[1]) - want[1]) <= 2 and px[2] == want[2]

    assert near(at(0.25, -0.25), (100, 100, 7))
    # a sphere turned by 90 degrees about z turns the texture with it (p = Rs^T (hit - c))
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    img = _draw(_cam(cx=32, cy=32), [_sphere((0, 0, -d), r, rot=Rz)], tex)
    assert near(at(0.25, 0.25), (100, 100, 7))  # world (0.25, 0.25) r is local (0.25, -0.25) r


def test_composite_is_the_references_with_its_colour_key():
    rng = np.random.RandomState(0)
    render = rng.randint(0, 256, (8, 8, 3), dtype=np.uint8)
    render[0, :4] = 255
    rgb, tex = rng.randint(0, 256, (8, 8, 3), dtype=np.uint8), rng.randint(0, 256, (8, 8, 3), dtype=np.uint8)
    full, rnd, occ = ref.composite(render, rgb, tex, 0.8)
    assert np.array_equal(full[0, :4], rgb[0, :4]) and np.array_equal(full[1:], render[1:]) and not occ[0, :4].any() and occ[1:].all()
    assert np.array_equal(rnd[0, :4], tex[0, :4])
    assert np.array_equal(rnd[1:], (render[1:] * 0.8 + tex[1:] * (1 - 0.8)).astype(np.uint8))  # truncation, not rounding


def test_extrinsic_flip_is_diag_1_m1_m1_on_the_right():
    rng = np.random.RandomState(1)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = np.linalg.qr(rng.randn(3, 3))[0], rng.randn(3)
    keep = E.copy()
    F = R.flip_extrinsic(E)
    assert np.array_equal(E, keep)
    assert np.allclose(F[:3, :3], E[:3, :3] @ np.diag([1.0, -1.0, -1.0]), rtol=0, atol=1e-15)
    assert np.array_equal(F[:, 3], E[:, 3]) and np.array_equal(F[3], E[3])
    cam = R.pack_view(np.array([[-300.0, 0, 128], [0, -301.0, 127], [0, 0, 1]]), E, [], [], [], 0.03, 1e-5, 3.0)[0]
    assert cam.dtype == np.float32 and tuple(cam[:4]) == (-300.0, -301.0, 128.0, 127.0)  # signed focal lengths, no abs()
    assert np.array_equal(cam[4:16], F[:3].astype(np.float32).reshape(-1)) and tuple(cam[16:]) == (np.float32(1e-5), 3.0)


def test_texture_and_factor_selection():
    assert R.texture_name(0.1, None) == "sphere_yellow_stripe_texture.png" and R.base_color(0.1) == (1.0, 1.0, 0.0)
    assert R.texture_name(0.11, None) == "sphere_cyan_stripe_texture.png" and R.base_color(0.11) == (0.60392156862, 0.86274509803, 1.0)
    for color in ("green", "red", "purple"):
        assert R.texture_name(1.0, color) == f"sphere_{color}_stripe_texture.png"
    with pytest.raises(KeyError):
        R.texture_name(1.0, "blue")
    atlas = R.load_atlas(TEXTURES)
    assert atlas.shape == (5, 256, 256, 4) and atlas.dtype == np.uint8
    _, sph, tex, n = R.pack_view(np.eye(3), np.eye(4), [np.eye(4)] * 3, [0.1, 0.11, 1.0], [None, None, "red"], 0.03, 1e-5, 3.0)
    assert n == 3 and [R.SPHERE_TEXTURES[t] for t in tex[:3]] == [R.texture_name(0.1, None), R.texture_name(0.11, None), R.texture_name(1.0, "red")]
    assert np.allclose(sph[:3, 13:], [R.base_color(0.1), R.base_color(0.11), R.base_color(1.0)]) and np.all(sph[:3, 12] == np.float32(0.03))


def _traj(L=30):
    g = np.tile(np.eye(4), (L, 1, 1))
    g[:, 0, 3] = np.arange(L)  # the gripper's x names its step
    j = np.zeros((L, 7, 7))
    j[:, :, 0], j[:, :, 1], j[:, :, 6] = np.arange(L)[:, None], np.arange(7)[None], 1.0
    return {"intrinsics": np.tile(np.eye(3), (L, 5, 1, 1)), "extrinsics": np.tile(np.eye(4), (L, 5, 1, 1)), "gripper_matrix": g,
            "gripper_open": (np.arange(L) % 2).astype(float), "joint_poses": j}


def test_render_episode_window_logic():
    cfg, traj, L = R.RenderConfig(), _traj(), 30
    assert cfg.action_horizon == 20
    # ts = 0: range(1, 21) -> step 20; ts = L - 22: range(9, 29) -> step 28; from there on the window is cut at L - 1 (step 28 stays
    # the last drawn); the last ts, L - 2, has an empty window and draws nothing
    assert [R.window_step(ts, L, 20) for ts in (0, L - 22, L - 21, L - 3, L - 2)] == [20, 28, 28, 28, None]
    for ts, step in ((0, 20), (L - 22, 28)):
        mats, opens, colors = R.step_spheres(traj, cfg, ts, "front")
        assert [m[0, 3] for m in mats] == [step] * 4 and [m[1, 3] for m in mats[1:]] == [1, 3, 5]  # gripper, then joints 1, 3, 5 of that step
        assert opens == [traj["gripper_open"][step], 1.0, 1.0, 1.0] and colors == [None, "red", "green", "purple"]
        assert len(R.step_spheres(traj, cfg, ts, "overhead")[0]) == 1  # overhead: the gripper alone
    assert R.step_spheres(traj, cfg, L - 2, "front") == ([], [], [])
    views = R.pack_step(traj, cfg, 0)
    assert [v[3] for v in views] == [4, 4, 4, 4, 1]
    assert [v[1][0, 12] for v in views] == [np.float32(0.01 * s) for s in cfg.camera_scales]


def test_tile_order_matches_tiling():
    cfg = R.RenderConfig()
    assert R.tile_cameras(cfg.cameras) == ["wrist", "front", "right_shoulder", "left_shoulder"]  # overhead is rendered, not tiled
    imgs = [np.full((256, 256, 3), 10 * (t + 1), np.uint8) for t in range(4)]
    tiled = R._tile(imgs)
    assert np.array_equal(tiled, tiling.tile_u8(imgs, 1)[0])
    for t, (l, tp, r, b) in enumerate(tiling.CROP_ORDER):
        assert (l, tp) == ((t & 1) * 256, (t >> 1) * 256)  # the kernel's tile row (t % 4) / 2, column t % 2
        assert np.all(tiled[tp:b, l:r] == 10 * (t + 1))
    small = [np.full((8, 6, 3), t, np.uint8) for t in range(4)]
    assert np.array_equal(R._tile(small)[8:, :6], small[2]) and np.array_equal(R._tile(small)[:8, 6:], small[1])


def test_trajectory_npz_round_trip(tmp_path):
    traj = _traj(5)
    p = os.path.join(str(tmp_path), "traj.npz")
    R.save_traj(p, traj)
    back = R.load_traj(p)
    assert set(back) == set(R.TRAJ_KEYS) and all(np.array_equal(back[k], traj[k]) for k in R.TRAJ_KEYS)
    q = np.array([0.1, -0.2, 0.3, 0.9])
    M = R.quat_xyzw_to_matrix(q)
    assert np.allclose(M @ M.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(M), 1.0)
    assert np.allclose(R.quat_xyzw_to_matrix([0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4)]), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
