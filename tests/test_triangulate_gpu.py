"""-m gpu: ``gn_openloop_triangulate`` against the f64 restatement (tests/triangulate_ref.py) per element on hand-built tables, its
refusals, and ``OpenLoopEval(triangulate=True)`` end to end on the tiny world.

Kernel shapes: N = 5, V = 4, S = 4, G = 4 over ``render.synthetic_episode``'s cameras (negative focal lengths).  Group g of a transition sits
in slot (g + v) % 4 of view v, so no slot index equals its group index in every view.  Observations are the exact projections of the
transition's four sphere centres plus up to 2 px of noise, drawn separately for the generated and the ground-truth columns, so every residual
is non-zero.  The rows: 0 -- 4, 3, 2 and 1 used views through slots of -1; 1 -- a group nobody shows, a group that loses two views to a
ground-truth mass of 0, a group whose generated mass is 1 below, exactly at and above ``min_ratio * gt_m``, a group nothing was generated
of; 2 -- an observation at (0.7, 0.9): its window starts at the image border; 3 -- two pairs of views that share one orientation a few
centimetres apart, [7] on either side of ``min_det`` (2e-3 here, so that the solved one keeps [7] >= 1e-3), beside two well-crossed pairs;
4 -- all four views of all four groups.

Both sides compute in f64; they differ by the order of operations (adjugate against LU, projection against cross product).  With [7] >= 1e-3
the solve amplifies a rounding of 1e-16 of a scene 1 m across to at most about 1e-12 m: 1e-9 m on positions and distances and 1e-7 px on the
reprojection residual are orders above it.

End to end: tests/test_openloop_spheres_gpu.py's world (64 x 64, V = 4, episodes of 6 and 9 observations = 13 transitions, batch 3), built
here on its own."""
import types

import numpy as np
import pytest
import torch

import replay_render_ref as RR
import triangulate_ref as TR
from genima_amd import render as R
from genima_amd import replay as P
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import OpenLoopEval, diffusion_validator

pytestmark = pytest.mark.gpu

CAMS = P.DEFAULT_CAMERAS
MARK = -1.2345e300
MIN_RATIO, MIN_DET = 0.5, 2e-3
N, V, S, G = 5, 4, 4, 4


def _sideways(cam, point, det):
    """The camera table moved along its own x axis, the same orientation from another place, so far that the two rays to ``point`` cross at
    [7] = ``det``: two unit rays at the angle t give det(A) = 2 sin^2 t and trace(A) = 4, so [7] = 27 / 32 sin^2 t, and t is about the
    baseline over the distance."""
    out = cam.copy()
    b = np.linalg.norm(point - cam[[7, 11, 15]]) * np.sqrt(det * 32.0 / 27.0)
    out[[7, 11, 15]] += (cam[4:16].reshape(3, 4)[:, 0] * np.float32(b)).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def tables():
    cfg, traj, _ = R.synthetic_episode(9, seed=7, texture_dir=RR.GOLDEN_SPHERES, action_horizon=4)
    views = [R.pack_views(R.pack_step(traj, cfg, ts, CAMS)) for ts in range(N)]
    cams = np.stack([v["cams"] for v in views])
    centre = np.stack([v["spheres"][0][:, [3, 7, 11]] for v in views]).astype(np.float64)  # the four spheres of view 0: [N, G, 3]
    assert (cams[..., :2] < 0).all()  # RLBench's negative focal lengths
    # two near-parallel pairs, (0, 1) looking at group 0 and (2, 3) at group 1: [7] about 0.75 and 1.35 min_det
    cams[3, 1], cams[3, 3] = _sideways(cams[3, 0], centre[3, 0], 0.75 * MIN_DET), _sideways(cams[3, 2], centre[3, 1], 1.35 * MIN_DET)
    rng = np.random.RandomState(11)
    slot = np.zeros((N, G, V), np.int32)
    obs = [[[None] * S for _ in range(V)] for _ in range(N)]
    gen = [[[None] * S for _ in range(V)] for _ in range(N)]
    for n in range(N):
        for g in range(G):
            for v in range(V):
                s = (g + v) % S
                slot[n, g, v] = s
                u, w = TR.observe(cams[n, v], centre[n, g])
                assert 4 < u < 252 and 4 < w < 252, (n, g, v, u, w)
                noise = rng.uniform(-2, 2, 4) if n != 3 else rng.uniform(-0.2, 0.2, 4)
                obs[n][v][s], gen[n][v][s] = (u + noise[0], w + noise[1]), (u + noise[2] * 0.7, w + noise[3] * 0.7)
    obs[2][0][slot[2, 0, 0]] = gen[2][0][slot[2, 0, 0]] = (0.7, 0.9)  # a window at the image border
    sph, win = TR.table_from_observations(obs, gen)
    assert (win[2, 0, slot[2, 0, 0]] == (0, 0, 12, 12)).all() and (sph >= 0).all() and (win[..., :2] >= 0).all()
    # row 0: 4, 3, 2, 1 used views
    slot[0, 1, 0] = slot[0, 2, :2] = slot[0, 3, :3] = -1
    # row 1: nobody shows group 0; group 1 has no ground-truth mass in views 1 and 3; group 2 straddles min_ratio; nothing generated of group 3
    slot[1, 0] = -1
    for v in (1, 3):
        sph[1, v, slot[1, 1, v], 5:9] = 0
    gt_m = int(sph[1, 0, slot[1, 2, 0], 5])
    for v, m in ((0, gt_m // 2 - 1), (1, gt_m // 2), (2, gt_m // 2 + 1)):
        q = sph[1, v, slot[1, 2, v]]
        q[2], q[3], q[1] = int(q[2]) * m // int(q[1]), int(q[3]) * m // int(q[1]), m  # python integers: the products pass 2^63
    for v in range(V):
        sph[1, v, slot[1, 3, v], 1:5] = 0
    # row 3: group 0 through the pair (0, 1), group 1 through (2, 3), groups 2 and 3 through the crossed pairs (0, 2) and (1, 3)
    slot[3, 0, 2:] = slot[3, 1, :2] = -1
    slot[3, 2, [1, 3]] = slot[3, 3, [0, 2]] = -1
    want = TR.triangulate(sph, win, cams, slot, centre, MIN_RATIO, MIN_DET)
    return types.SimpleNamespace(sph=sph, win=win, cams=cams, slot=slot, centre=centre, want=want)


def _dev(t):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (t.sph, t.win, t.cams, t.slot, t.centre)]


def test_the_hand_built_rows_hold_the_cases(tables):
    """On the CPU reference alone: the table exercises what the module docstring lists."""
    w = tables.want
    assert w[0, :, 1, 0].tolist() == [4, 3, 2, 1] and w[0, :, 0, 0].tolist() == [4, 3, 2, 1]
    assert w[1, :, 1, 0].tolist() == [0, 2, 4, 4] and w[1, :, 0, 0].tolist() == [0, 2, 3, 0]  # view 0 of group 2 is 1 below the ratio: not used
    assert (w[1, 0, :, 7] == 0).all() and np.isnan(w[1, 0, :, 1:7]).all() and np.isnan(w[1, 3, 0, 1:7]).all() and not np.isnan(w[1, 3, 1]).any()
    assert w[2, 0, 1, 0] == 4 and w[2, 0, 1, 6] > 20  # the border observation is far from where the other three views point
    d = w[3, :, 1, 7]
    print(f"row 3 conditioning: {d}")
    assert d[0] < MIN_DET < d[1] and d[0] > 0.5 * MIN_DET and d[1] < 2 * MIN_DET and (d[2:] > 0.1).all()  # the near-parallel pairs straddle min_det
    assert np.isnan(w[3, 0, :, 1:7]).all() and not np.isnan(w[3, 1:]).any()
    solved = ~np.isnan(w[..., 4])
    assert solved.sum() >= 28 and (w[..., 7][solved] >= 1e-3).all() and (w[..., 7] <= 1.0).all()
    assert (w[..., 5][solved] > 0).all() and (w[..., 6][solved] > 0).all() and np.median(w[..., 5][solved]) > 1e-4 and np.median(w[..., 6][solved]) > 0.1
    assert not np.array_equal(w[4, :, 0], w[4, :, 1])


def test_kernel_equals_the_f64_reference_per_element(engine, tables):
    t, want = tables, tables.want
    dev = _dev(t)
    out = torch.full((N, G, 2, 8), MARK, dtype=torch.float64, device="cuda")
    got = engine.openloop_triangulate(*dev, out, min_ratio=MIN_RATIO, min_det=MIN_DET, slot_host=t.slot, win_host=t.win).cpu().numpy()
    assert np.array_equal(got[..., 0], want[..., 0])  # the counts
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not (got == MARK).any()  # the NaN pattern; every element was written
    solved = ~np.isnan(want[..., 4])
    err = np.abs(got - want)
    print(f"max |kernel - reference|: position {err[..., 1:4][solved].max():.3e} m, error {err[..., 4][solved].max():.3e} m, ray residual "
          f"{err[..., 5][solved].max():.3e} m, reprojection {err[..., 6][solved].max():.3e} px, det {err[..., 7].max():.3e}")
    assert err[..., 1:6][solved].max() <= 1e-9 and err[..., 6][solved].max() <= 1e-7 and err[..., 7].max() <= 1e-12
    assert (got[..., 7][want[..., 0] < 2] == 0).all()
    # a second run, and one without the host copies: the same bits
    for kw in (dict(slot_host=t.slot, win_host=t.win), {}):
        again = engine.openloop_triangulate(*dev, min_ratio=MIN_RATIO, min_det=MIN_DET, **kw).cpu().numpy()
        assert np.array_equal(again.view(np.int64), got.view(np.int64))
    # slots the host never saw: anything outside [0, S) reads as -1
    wild = t.slot.copy()
    wild[t.slot < 0] = np.resize(np.array([S, -7, 1 << 30, -(1 << 31), 8], np.int32), int((t.slot < 0).sum()))
    dev[3] = torch.from_numpy(wild).cuda()
    assert np.array_equal(engine.openloop_triangulate(*dev, min_ratio=MIN_RATIO, min_det=MIN_DET).cpu().numpy().view(np.int64), got.view(np.int64))


def test_refused_arguments_leave_the_output_untouched(engine, tables):
    lib, ctx = engine.lib, engine._ctx
    n, big = 2, 9  # every buffer holds V = S = G = 9: a call accepted by mistake would still stay inside them
    sph = torch.zeros(n * big * big * 17 + 1, dtype=torch.int64, device="cuda")
    win = torch.zeros(n * big * big * 4 + 1, dtype=torch.int32, device="cuda")
    cams = torch.zeros(n * big * 18 + 1, dtype=torch.float32, device="cuda")
    slot = torch.full((n * big * big + 1,), -1, dtype=torch.int32, device="cuda")
    centre = torch.zeros(n * big * 3 + 1, dtype=torch.float64, device="cuda")
    out = torch.full((n * big * 2 * 8 + 1,), MARK, dtype=torch.float64, device="cuda")
    slot_h = np.full((n, G, V), -1, np.int32)
    win_h = np.tile(np.array([0, 0, 8, 8], np.int32), (n, V, S, 1))
    ok = dict(sph=sph.data_ptr(), win=win.data_ptr(), cams=cams.data_ptr(), slot=slot.data_ptr(), centre=centre.data_ptr(), slot_host=None, win_host=None,
              out=out.data_ptr(), min_ratio=0.5, min_det=1e-6, N=n, V=V, S=S, G=G)

    def call(a):
        return lib.gn_openloop_triangulate(ctx, a["sph"], a["win"], a["cams"], a["slot"], a["centre"], a["slot_host"], a["win_host"], a["out"], a["min_ratio"],
                                           a["min_det"], a["N"], a["V"], a["S"], a["G"])

    bad = [dict(sph=None), dict(win=None), dict(cams=None), dict(slot=None), dict(centre=None), dict(out=None), dict(N=-1), dict(V=1), dict(V=9), dict(S=0),
           dict(S=9), dict(G=0), dict(G=9), dict(min_ratio=-0.1), dict(min_ratio=float("nan")), dict(min_det=0.0), dict(min_det=-1e-6),
           dict(min_det=float("nan")), dict(sph=sph.data_ptr() + 4), dict(win=win.data_ptr() + 2), dict(cams=cams.data_ptr() + 2),
           dict(slot=slot.data_ptr() + 2), dict(centre=centre.data_ptr() + 4), dict(out=out.data_ptr() + 4),
           dict(slot_host=slot_h.ctypes.data + 2), dict(win_host=win_h.ctypes.data + 2)]
    keep = []  # the host tables of the calls below stay alive until they were made
    for value in (S, -2, 1 << 20):
        h = slot_h.copy()
        h[n - 1, G - 1, V - 1] = value  # the last slot of the table
        keep.append(h)
        bad.append(dict(slot_host=h.ctypes.data))
    for last in ([-1, 0, 3, 3], [0, -1, 3, 3], [5, 0, 3, 4], [0, 5, 4, 3], [0, 0, 257, 2], [0, 0, 2, 257]):
        h = win_h.copy()
        h[n - 1, V - 1, S - 1] = last  # the last window of the table
        keep.append(h)
        bad.append(dict(win_host=h.ctypes.data))
    for change in bad:
        assert call(dict(ok, **change)) != 0, change
    assert call(dict(ok, N=0)) == 0  # accepted, does nothing
    torch.cuda.synchronize()
    assert bool((out == MARK).all())
    # ... and the unchanged arguments are accepted, with and without the host copies: every group has no view
    assert call(ok) == 0 and call(dict(ok, slot_host=slot_h.ctypes.data, win_host=win_h.ctypes.data)) == 0
    torch.cuda.synchronize()
    got = out[: n * G * 2 * 8].view(n, G, 2, 8).cpu().numpy()
    assert (got[..., [0, 7]] == 0).all() and np.isnan(got[..., 1:7]).all() and bool((out[n * G * 2 * 8:] == MARK).all())
    from genima_amd._lib import GenimaHipError
    from genima_amd.engine import Engine

    dev = _dev(tables)
    with pytest.raises(RuntimeError, match="eager"):
        Engine("cuda:0", record=True).openloop_triangulate(*dev)
    with pytest.raises(GenimaHipError, match="must lie in"):
        engine.openloop_triangulate(*dev, slot_host=np.full((N, G, V), S, np.int32))
    with pytest.raises(GenimaHipError, match="host copy"):
        engine.openloop_triangulate(*dev, slot_host=tables.slot.astype(np.int64))
    with pytest.raises(GenimaHipError, match="contiguous device tensor"):
        engine.openloop_triangulate(dev[0], dev[1], dev[2], dev[3], dev[4].float())


# ---- end to end on the tiny world
SIZE, LENGTHS, BATCH, SEED = 64, (6, 9), 3, 2
# The evaluators below leave rays that cross at [7] < 1e-3 unsolved.  The 1e-9 m bar is stated for [7] >= 1e-3; the adjugate and an LU solve,
# both f64, drift apart as 1 / [7] (the same two-ray systems in numpy: at most 3e-13 m for [7] in 1e-3 .. 1e-2, 5e-10 m in 1e-6 .. 1e-5), so at
# the option's default of 1e-6 the bar would hold by a factor of two at best, and a views pair of this world can cross as badly as 1.6e-3.
TRI = dict(triangulate=True, tri_min_det=1e-3)
N_TR = sum(L - 1 for L in LENGTHS)


class _Drawn(OpenLoopEval):
    """A stand-in generator: the ground-truth render itself, or, with ``shift = (view, dx, dy)``, that render with one tile's spheres moved by
    (dx, dy) pixels over the observation."""
    shift = None

    def generate(self, batch, idx, generator):
        B, H, W = len(idx), self.H, self.W
        views = batch["full"].view(B, 4, H, W, 3).clone()
        if self.shift is not None:
            v, dx, dy = self.shift
            occ = torch.roll(batch["occupied"].view(B, 4, H, W)[:, v], (dy, dx), (1, 2)) != 0
            moved = torch.roll(views[:, v], (dy, dx), (1, 2))
            views[:, v] = torch.where(occ[..., None], moved, batch["images_u8"].view(B, 4, H, W, 3)[:, v])
        return views.view(B, 2, 2, H, W, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, 3).contiguous()


def _reference_points(ev, res):
    return TR.triangulate(res.spheres, res.windows, ev.views["cams"].cpu().numpy(), ev.point_slots_host, ev.point_centres_host, ev.tri_min_ratio, ev.tri_min_det)


def _assert_points(ev, res):
    """``points`` against the reference recomputed from the result's own tables, at the kernel test's bar on EVERY solved row.  The evaluators
    of these tests run with ``tri_min_det = 1e-3`` (``TRI``), so every solved row meets the bar's premise, [7] >= 1e-3."""
    want = _reference_points(ev, res)
    got = res.points
    assert got.shape == (N_TR, ev.point_slots_host.shape[1], 2, 8) and got.dtype == np.float64
    assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(np.isnan(got), np.isnan(want))
    solved = ~np.isnan(want[..., 4])
    err = np.abs(got - want)
    print(f"end to end, {int(solved.sum())} solved rows, min [7] {want[..., 7][solved].min():.3e}: max |points - reference| {err[..., 1:6][solved].max():.3e} m, "
          f"reprojection {err[..., 6][solved].max():.3e} px, [7] {err[..., 7].max():.3e}")
    assert ev.tri_min_det == 1e-3 and solved.sum() >= 20 and (want[..., 7][solved] >= 1e-3).all()
    assert err[..., 1:6][solved].max() <= 1e-9 and err[..., 6][solved].max() <= 1e-7 and err[..., 7].max() <= 1e-12
    return want


@pytest.fixture(scope="module")
def world(engine):
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    eps = [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=SIZE, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]
    stand_in = types.SimpleNamespace(pipe=types.SimpleNamespace(device=engine.device, encode_ids=lambda prompts: torch.zeros((len(prompts), 77), dtype=torch.int64)))

    def drawn(shift=None, **kw):
        ev = _Drawn(stand_in, None, eps, CAMS, render_cfg=cfg, stats=None, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine, **kw)
        ev.shift = shift
        return ev

    return types.SimpleNamespace(cfg=cfg, eps=eps, drawn=drawn)


def test_group_tables_of_the_evaluator(world):
    ev = world.drawn(**TRI)
    tab = {k: ev.views[k].cpu().numpy() for k in ("spheres", "count")}
    slot, centre = TR.group_tables(tab["spheres"], tab["count"], ev.windows_host)
    assert np.array_equal(ev.point_slots_host, slot) and np.array_equal(ev.point_centres_host, centre) and slot.shape == (N_TR, 4, 4)
    assert np.array_equal(ev.point_slots.cpu().numpy(), slot) and np.array_equal(ev.point_centres.cpu().numpy(), centre)
    assert (slot[[4, 12]] == -1).all() and (slot[0] >= 0).any()  # the last transition of each episode draws nothing
    off = world.drawn()
    assert off.point_slots is None and off.run().points is None


def test_a_generator_that_returns_the_render_has_no_excess(world, tmp_path):
    ev = world.drawn(**TRI)
    res = ev.run()
    want = _assert_points(ev, res)
    assert np.array_equal(res.points[:, :, 0].view(np.int64), res.points[:, :, 1].view(np.int64))  # kind 0 equals kind 1 bit for bit
    s = res.triangulation_summary()
    assert s["excess_mm"] == 0.0 and s["generated"] == s["ground_truth"] and s["generated"]["solved_rate"] == 1.0 and s["n_groups"] == int((want[:, :, 1, 0] >= 2).sum()) >= 20
    assert s["score_mm"] == s["generated"]["err_mm"]
    print(f"tiny world, ground truth: {s['ground_truth']}")
    assert np.array_equal(res.point_slots, ev.point_slots_host) and np.array_equal(res.cams, ev.views["cams"].cpu().numpy())
    # without the option: the same tables and summary(), no points, and to_json() is summary() alone
    plain = world.drawn().run()
    assert plain.points is None and plain.triangulation_summary() is None
    assert np.array_equal(plain.spheres, res.spheres) and np.array_equal(plain.image, res.image) and plain.summary() == res.summary()
    assert plain.to_json(str(tmp_path / "plain.json")) == plain.summary()
    assert res.to_json(str(tmp_path / "tri.json")) == dict(res.summary(), spheres_3d=s)
    assert np.array_equal(ev.run().points.view(np.int64), res.points.view(np.int64))  # a second run: the same bits


def test_one_shifted_tile_raises_the_residuals(world):
    base = world.drawn(**TRI).run().triangulation_summary()
    ev = world.drawn(shift=(2, 3, -2), **TRI)
    res = ev.run()
    _assert_points(ev, res)
    s = res.triangulation_summary()
    print(f"tiny world, view 2 moved by (3, -2) px: generated {s['generated']}, excess {s['excess_mm']}")
    assert s["ground_truth"] == base["ground_truth"]
    assert s["generated"]["reproj_px"] > base["generated"]["reproj_px"] and s["generated"]["ray_mm"] > base["generated"]["ray_mm"]
    assert not np.array_equal(res.points[:, :, 0], res.points[:, :, 1], equal_nan=True)
    plain = world.drawn(shift=(2, 3, -2)).run()
    assert plain.summary() == res.summary() and np.array_equal(plain.spheres, res.spheres)  # the other metrics are what they are without the option


def test_the_diffusion_agent_and_the_validator(world, engine):
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=2 * SIZE, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    agent = SDControlNetAgent(ns)
    ev = OpenLoopEval(agent, None, world.eps, CAMS, render_cfg=world.cfg, stats=None, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine, **TRI)
    res = ev.run()
    _assert_points(ev, res)
    s = res.triangulation_summary()
    validate = diffusion_validator(lambda: agent.pipe, world.eps, CAMS, render_cfg=world.cfg, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine,
                                   **TRI)
    line = validate(100)
    assert line["err_3d_mm"] == s["generated"]["err_mm"] and line["excess_mm"] == s["excess_mm"]
    assert line["select"] == res.summary()["image"]["spheres"]["score"]  # select is unchanged
    assert set(line) == {"step", "select", "found_rate", "shift_px", "mass_ratio", "spread_ratio", "colour_l1", "sphere_rmse", "background_rmse", "wrapped_mse", "n",
                         "err_3d_mm", "excess_mm"}
