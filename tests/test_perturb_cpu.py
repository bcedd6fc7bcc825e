"""CPU: ``genima_amd.perturb`` (the settings, the draws, the camera algebra) and tests/perturb_ref.py (the numpy f64 restatement of
``gn_view_perturb``'s pixel rule) -- everything the GPU tests of the perturbed evaluator rely on, checked without a device."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import perturb_ref as PR
import render_reference as REF
import replay_render_ref as RR
import sphere_metrics_ref as SM
from genima_amd import _lib
from genima_amd import perturb as PB
from genima_amd import render as R
from genima_amd import replay as P

CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, PERTURB_SEED = 64, (6, 9), 3  # the evaluator GPU tests' episodes and their perturbation seed
ONE = np.array([[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]])


@pytest.fixture(scope="module")
def world():
    """The 13 transitions of the two synthetic episodes as the evaluator lays them out: view tables [N, V, ...] and each one's episode."""
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    vt = P.view_tables([traj for _, traj, _ in eps], cfg, CAMS)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)])
    rows = np.concatenate([starts[e] + np.arange(L - 1) for e, L in enumerate(LENGTHS)])
    ep_of = np.concatenate([np.full(L - 1, e) for e, L in enumerate(LENGTHS)])
    idx = (rows[:, None] * len(CAMS) + np.arange(len(CAMS))[None]).reshape(-1)
    views = {k: v[idx].reshape((len(rows), len(CAMS)) + v.shape[1:]) for k, v in vt.items()}
    windows = R.sphere_windows(views["cams"], views["spheres"], views["count"], SIZE, SIZE)
    return dict(cfg=cfg, views=views, ep_of=ep_of, windows=windows, atlas=R.load_atlas(cfg.texture_dir))


def _revealed_share(M, H, W):
    M = M.reshape(-1, 9)
    _, _, n = PR.view_perturb(np.zeros((len(M), H, W, 3), np.uint8), M, np.tile(ONE, (len(M), 1)))
    return float(n.mean()) / (H * W)


# ---- the library and the binding
def test_the_entry_point_is_bound_and_refuses_without_launching():
    from genima_amd import build

    assert "view_perturb.hip" in build.SOURCES and build.EXTRA_FLAGS["view_perturb.hip"] == ["-ffp-contract=off"]  # one rounded operation at a time
    lib = _lib.load()
    assert "gn_view_perturb" in _lib.SIGNATURES and hasattr(lib, "gn_view_perturb")
    buf = C.create_string_buffer(64)
    assert lib.gn_view_perturb(None, buf, buf, None, None, buf, buf, 1, 2, 2) != 0  # no context: refused before anything is touched
    assert b"gn_view_perturb" in lib.gn_last_error()


# ---- the algebra
def test_a_sphere_centre_through_the_homography_lands_on_its_old_projection(world):
    """1e-9 px: f64 round-off at these magnitudes (|fx| ~ 88, pixels < 64) with four orders of margin over the 4e-14 measured."""
    rng = np.random.default_rng(0)
    cams, worst, n = world["views"]["cams"].reshape(-1, 18), 0.0, 0
    for sign in (1.0, -1.0):  # the synthetic fx is negative as RLBench's is; the other sign too
        for i, cam in enumerate(cams):
            cam = cam.copy()
            cam[0] *= sign
            Q = PB.rotation(*rng.uniform(-0.1, 0.1, 3))
            new = PB.perturb_cams(cam, Q, rng.uniform(0.9, 1.1), rng.uniform(-3.0, 3.0, 2))
            assert new.dtype == np.float32 and np.array_equal(new[16:], cam[16:]) and np.array_equal(new[[7, 11, 15]], cam[[7, 11, 15]])  # t, znear, zfar stay
            M = PB.homography(cam, new)
            sph = world["views"]["spheres"].reshape(-1, 4, 16)[i]
            for s in range(int(world["views"]["count"].reshape(-1)[i])):
                c = sph[s, [3, 7, 11]].astype(np.float64)
                got, want = PR.through(M, *PR.project(new, c)), PR.project(cam, c)
                worst, n = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1])), n + 1
    print(f"{n} sphere centres: worst distance {worst:.3e} px")
    assert n > 300 and worst <= 1e-9


def test_the_identity_is_exact(world):
    cams = world["views"]["cams"].copy()
    cams[0, 0, 5] = -0.0  # a negative zero in a pose keeps its sign bit
    same = PB.perturb_cams(cams, np.eye(3), 1.0, (0.0, 0.0))
    assert same.dtype == np.float32 and np.array_equal(same.view(np.uint32), cams.view(np.uint32))
    assert np.array_equal(PB.perturb_cams(cams, PB.rotation(0.0, 0.0, 0.0)).view(np.uint32), cams.view(np.uint32))
    M = PB.homography(cams, same)
    assert M.dtype == np.float64 and M.shape == cams.shape[:-1] + (9,) and (M == np.eye(3).reshape(9)).all()
    new, M, colour, _ = PB.transition_tables(PB.Perturbation("nothing"), world["views"]["cams"], world["ep_of"], len(LENGTHS), CAMS, seed=5)
    assert np.array_equal(new.view(np.uint32), world["views"]["cams"].view(np.uint32)) and (M == np.eye(3).reshape(9)).all() and (colour == ONE[0]).all()


def test_rotation_is_roll_yaw_pitch_in_the_cameras_axes():
    Q = PB.rotation(0.3, -0.2, 0.1)
    assert np.allclose(Q @ Q.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(Q) - 1.0) < 1e-15
    assert np.allclose(PB.rotation(0.3, 0, 0) @ [0, 1, 0], [0, np.cos(0.3), np.sin(0.3)])  # pitch turns y towards z (the camera looks up)
    assert np.allclose(PB.rotation(0, 0, 0.1) @ [1, 0, 0], [np.cos(0.1), np.sin(0.1), 0])
    assert np.allclose(Q, PB.rotation(0, 0, 0.1) @ PB.rotation(0, -0.2, 0) @ PB.rotation(0.3, 0, 0))


# ---- the draws
def test_draws_repeat_leave_the_wrist_alone_and_share_one_colour_per_episode(world):
    p = PB.parse("camera_pose+light_color")
    a, b = PB.draw(p, 5, CAMS, seed=11), PB.draw(p, 5, CAMS, seed=11)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["pitch"], PB.draw(p, 5, CAMS, seed=12)["pitch"])
    w = CAMS.index("wrist")
    for k, ident in (("pitch", 0.0), ("yaw", 0.0), ("roll", 0.0), ("zoom", 1.0), ("shift_x", 0.0), ("shift_y", 0.0)):
        assert (a[k][:, w] == ident).all() and a[k].shape == (5, len(CAMS))
    others = [v for v in range(len(CAMS)) if v != w]
    assert (np.abs(a["pitch"][:, others]) <= 0.05).all() and (a["pitch"][:, others] != 0).all() and len(np.unique(a["roll"][:, others])) == 15
    assert a["gain"].shape == (5, 3) and (a["gain"] >= 0.5).all() and (a["gain"] <= 1.0).all() and (a["offset"] == 0).all()
    assert np.array_equal(PB.draw(PB.PRESETS["camera_pose"], 5, CAMS, seed=11)["yaw"], a["yaw"])  # a value does not depend on the other ranges
    new, M, colour, d = PB.transition_tables(p, world["views"]["cams"], world["ep_of"], len(LENGTHS), CAMS, seed=11)
    assert np.array_equal(new[:, w].view(np.uint32), world["views"]["cams"][:, w].view(np.uint32)) and (M[:, w] == np.eye(3).reshape(9)).all()
    assert (colour == colour[:, :1]).all()  # one colour row serves an episode's four views ...
    for e in range(len(LENGTHS)):  # ... and every transition of the episode
        rows = colour[world["ep_of"] == e]
        assert (rows == np.concatenate([d["gain"][e], d["offset"][e]])).all()
    assert not np.array_equal(colour[0], colour[-1])
    r = PB.draw_ranges(d)
    assert r["pitch"]["min"] == d["pitch"].min() and r["gain"]["max"] == d["gain"].max(axis=0).tolist() and json.loads(json.dumps(r)) == r


# ---- parsing
@pytest.mark.parametrize("text", ["camera_pose", "light_color", "camera_pose+light_color",
                                  "camera:pitch=-0.05..0.05,roll=0.1,zoom=0.95..1.05;light:r=0.5..1,g=0.5..1,b=0.5..1",
                                  "camera:shift_x=-2..2,shift_y=1.5,cameras=front|wrist", "light:r_offset=-20..10,b=1.5"])
def test_parse_rebuilds_a_setting_from_its_description(text):
    p = PB.parse(text)
    assert p.name == text and PB.parse(json.loads(json.dumps(p.describe()))) == p and PB.parse(p) is p
    d = p.describe()
    assert d["light"]["model"] == "channel_gain" and d["camera"]["translation"] == "left out"


def test_parse_reads_the_spec():
    p = PB.parse("camera:pitch=-0.05..0.05,roll=0.1,zoom=0.95..1.05;light:r=0.5..1,g=0.5..1,b=0.5..1")
    assert p.pitch == (-0.05, 0.05) and p.roll == (0.1, 0.1) and p.zoom == (0.95, 1.05) and p.yaw == (0.0, 0.0) and p.cameras is None
    assert p.gain == ((0.5, 1.0),) * 3 and p.offset == ((0.0, 0.0),) * 3
    c = PB.PRESETS["camera_pose"]
    assert c.pitch == c.yaw == c.roll == (-0.05, 0.05) and c.zoom == (1.0, 1.0) and c.shift_x == c.shift_y == (0.0, 0.0)
    assert set(c.cameras) == {"front", "left_shoulder", "right_shoulder"}
    assert PB.PRESETS["light_color"].gain == ((0.5, 1.0),) * 3 and PB.PRESETS["light_color"].pitch == (0.0, 0.0)
    j = PB.parse("camera_pose+light_color")
    assert j.pitch == c.pitch and j.cameras == c.cameras and j.gain == PB.PRESETS["light_color"].gain


@pytest.mark.parametrize("text, key", [("camera:tilt=0.1", "tilt"), ("light:w=0.5", "w"), ("camera:pitch=0.1..-0.1", "pitch"), ("camera:zoom=0", "zoom"),
                                       ("camera:zoom=-1..1", "zoom"), ("light:g=-0.5..1", "g"), ("camera:roll=abc", "roll"), ("weather", "weather"),
                                       ("camera:pitch=0.1+camera:pitch=0.2", "pitch")])
def test_each_refusal_names_its_key(text, key):
    with pytest.raises(ValueError, match=key):
        PB.parse(text)


def test_the_dataclass_refuses_what_parse_refuses():
    with pytest.raises(ValueError, match="zoom"):
        PB.Perturbation("x", zoom=(0.0, 1.0))
    with pytest.raises(ValueError, match="yaw"):
        PB.Perturbation("x", yaw=(1.0, 0.0))
    with pytest.raises(ValueError, match="b = "):
        PB.Perturbation("x", gain=((1, 1), (1, 1), (-0.1, 1)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        PB.PRESETS["camera_pose"].zoom = (2.0, 2.0)


# ---- the reference warp
def test_reference_warp_known_answers():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (3, 37, 53, 3)).astype(np.uint8)
    M, colour = PR.identity(3)
    dst, valid, n = PR.view_perturb(src, M, colour)
    assert np.array_equal(dst, src) and valid.all() and (n == 0).all()  # the identity copies
    M[1] = [1, 0, 5, 0, 1, -3, 0, 0, 1]  # output (x, y) reads source (x + 5, y - 3)
    dst, valid, n = PR.view_perturb(src, M, colour)
    assert np.array_equal(dst[1, 3:, :48], src[1, :34, 5:]) and np.array_equal(dst[0], src[0])
    assert valid[1, 3:, :48].all() and not valid[1, :3].any() and not valid[1, :, 48:].any() and n[1] == 37 * 53 - 34 * 48 and n[0] == 0
    assert np.array_equal(dst[1, 0, :48], src[1, 3, 5:])  # rows past the top edge mirror about row 0's centre: y - 3 = -3 -> 3
    flat = np.full((1, 4, 4, 3), 200, np.uint8)
    out, _, _ = PR.view_perturb(flat, PR.identity(1)[0], np.array([[2.0, 1.0, 0.5, 0.0, -250.0, 0.5]]))
    assert (out[..., 0] == 255).all() and (out[..., 1] == 0).all() and (out[..., 2] == 100).all()  # saturates, clamps at 0, 100.5 rounds to even
    out, _, _ = PR.view_perturb(flat, PR.identity(1)[0], np.array([[0.5, 1.0, 1.0, 1.5, 0.0, 0.0]]))
    assert (out[..., 0] == 102).all()  # 101.5 rounds to even too
    out, valid, n = PR.view_perturb(flat, np.array([[1.0, 0, 0, 0, 1, 0, 0, 0, -1]]), PR.identity(1)[1])
    assert not out.any() and not valid.any() and n[0] == 16  # w < 0 everywhere: behind the camera


def test_warped_render_agrees_with_the_re_render(world):
    """The render of the OLD camera over a frame, warped, against the render of the NEW camera over the warped frame -- both by the numpy
    references (tests/render_reference.py, perturb_ref) -- per sphere through tests/sphere_metrics_ref.py with the warped frame as the
    observation: the centroid distance and the mass ratio.  Their disagreement is the bilinear resampling of the warped spheres; it cannot
    be derived, so it was measured on these cases: 32 spheres of four views (one per camera) under the fixed rotations (1, -1.5, 3) degrees
    with zoom 1.05 and (3, -2, 8) degrees with zoom 0.92 -- worst centroid distance 1.675 px (a 5 px wrist sphere whose window overlaps
    its neighbours'; 0.94 px on the other cameras), mass ratio between 0.588 and 0.925 (the blur takes the thresholded change of the
    sphere's rim).  Asserted: twice the worst values, 3.35 px and |mass ratio - 1| <= 0.825."""
    H = W = SIZE
    yy, xx = np.mgrid[0:H, 0:W]
    frame = np.stack([96 + 40 * np.sin(xx / 9.0 + c) + 30 * np.cos(yy / 7.0 - c) for c in range(3)], axis=-1).astype(np.uint8)
    v, atlas, samples = world["views"], world["atlas"], world["cfg"].samples
    worst_shift, worst_mass, n_spheres = 0.0, 0.0, 0
    for pitch, yaw, roll, zoom in ((1.0, -1.5, 3.0, 1.05), (3.0, -2.0, 8.0, 0.92)):
        Q = PB.rotation(*np.deg2rad([pitch, yaw, roll]))
        for n, cam_i in ((0, 0), (2, 1), (6, 2), (9, 3)):
            cam, sph, tex, count = v["cams"][n, cam_i], v["spheres"][n, cam_i], v["tex_index"][n, cam_i], int(v["count"][n, cam_i])
            new = PB.perturb_cams(cam, Q, zoom)
            M = PB.homography(cam, new)[None]
            full_old = REF.composite(REF.render(cam, sph, tex, count, atlas, H, W, samples)[0], frame)[0]
            warped_render = PR.view_perturb(full_old[None], M, ONE)[0]
            warped_frame = PR.view_perturb(frame[None], M, ONE)[0]
            full_new, _, occupied = REF.composite(REF.render(new, sph, tex, count, atlas, H, W, samples)[0], warped_frame[0])
            win = R.sphere_windows(new, sph, count, H, W)[None, None]
            tab = SM.sphere_metrics(warped_render[None], full_new[None, None], warped_frame[None], occupied[None, None].astype(np.uint8), win, 30)[0, 0]
            d = SM.derived(tab)
            for s in range(count):
                assert tab[s, 5] > 0 and tab[s, 1] > 0, (n, cam_i, s)
                print(f"transition {n} camera {CAMS[cam_i]} sphere {s}: centroid distance {d['shift'][s]:.4f} px, mass ratio {d['mass_ratio'][s]:.4f}")
                worst_shift, worst_mass, n_spheres = max(worst_shift, d["shift"][s]), max(worst_mass, abs(d["mass_ratio"][s] - 1.0)), n_spheres + 1
    print(f"{n_spheres} spheres: worst centroid distance {worst_shift:.4f} px, worst |mass ratio - 1| {worst_mass:.4f}")
    assert n_spheres == 32 and worst_shift <= 3.35 and worst_mass <= 0.825


# ---- what the GPU tests rely on
def test_conditions_the_evaluator_gpu_tests_rely_on(world):
    """Under ``camera_pose`` with the GPU tests' seed every sphere drawn clean is still drawn and at most a quarter of a view is revealed
    border.  Measured here for fixed rotations of (1, -1.5, 3) degrees with zoom 1.05 and of (3, -2, 8) degrees with zoom 0.92: 176 of 176
    spheres kept both times, revealed share 0.026 and 0.203; the preset's +-2.87 degrees without zoom lies inside the second case."""
    v, clean = world["views"], world["windows"]
    assert int(clean.any(axis=-1).sum()) == 176  # 11 drawing transitions x 4 cameras x 4 spheres
    for (pitch, yaw, roll, zoom), most in (((1.0, -1.5, 3.0, 1.05), 0.03), ((3.0, -2.0, 8.0, 0.92), 0.25)):
        new = PB.perturb_cams(v["cams"], PB.rotation(*np.deg2rad([pitch, yaw, roll])), zoom)
        share = _revealed_share(PB.homography(v["cams"], new), SIZE, SIZE)
        lost = PB.lost_windows(clean, R.sphere_windows(new, v["spheres"], v["count"], SIZE, SIZE))
        print(f"rotation ({pitch}, {yaw}, {roll}) degrees, zoom {zoom}: {lost} spheres lost, revealed share {share:.4f}")
        assert lost == 0 and 0.0 < share <= most
    new, M, _, _ = PB.transition_tables(PB.PRESETS["camera_pose"], v["cams"], world["ep_of"], len(LENGTHS), CAMS, seed=PERTURB_SEED)
    share = _revealed_share(M, SIZE, SIZE)
    lost = PB.lost_windows(clean, R.sphere_windows(new, v["spheres"], v["count"], SIZE, SIZE))
    print(f"camera_pose, seed {PERTURB_SEED}: {lost} spheres lost, revealed share {share:.4f}")
    assert lost == 0 and 0.0 < share <= 0.25
    assert PB.lost_windows(clean, np.zeros_like(clean)) == 176 and PB.lost_windows(clean, np.zeros_like(clean), drawn=np.zeros(clean.shape[:-1], bool)) == 0
