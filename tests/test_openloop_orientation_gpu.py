"""-m gpu: ``gn_openloop_orientation`` bit for bit against the integer restatement (tests/orientation_ref.py) over candidate images that
``gn_render_spheres`` itself draws from the numpy-composed rotated tables, a planted rotation, the shift, the refusals, and
``OpenLoopEval(orientation=)`` end to end on the tiny families.

The kernel world: tests/render_reference.py's ``scene`` at 128 x 128 -- 2 samples x 4 views, S = 4 slots, 1 - 4 spheres drawn per view -- and
K = 7 candidates on a 5 degree grid."""
import types

import numpy as np
import pytest
import torch

import orientation_ref as OF
import render_reference as ref
import replay_render_ref as RR
from genima_amd import render as R
from genima_amd import replay as P
from genima_amd.agent import SDControlNetAgent
from genima_amd.openloop import SHIFT_FOUND_MASS, OpenLoopEval, orientation_candidates

pytestmark = pytest.mark.gpu

B, V, H, W, S, K = 2, 4, 128, 128, 4, 7
MARK = -0x0123456789ABCDEF


class _World:
    def __init__(self, engine):
        self.E = engine
        self.views = ref.scene(5, B=B * V, H=H, W=W)
        self.win = R.sphere_windows(self.views["cams"], self.views["spheres"], self.views["count"], H, W)
        self.atlas = torch.from_numpy(R.load_atlas(RR.GOLDEN_SPHERES)).cuda()
        self.angles, self.rot = orientation_candidates(K, 30.0)
        self.tables = OF.candidate_tables(self.views["spheres"], self.rot)  # [B * V, S, K, S, 16]
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in self.views.items()}
        self.dev["win"], self.dev["rot"] = torch.from_numpy(self.win).cuda(), torch.from_numpy(self.rot).cuda()
        self._drawn = {}

    def drawn(self, samples):
        """-> (gt uint8 [B * V, H, W, 3], occupied [B * V, H, W], cand [B * V, S, K, H, W, 3]) as gn_render_spheres draws them over an all-255
        background (``full`` is then the raw render), device and host: the reference is computed once per ``samples`` and shared."""
        if samples not in self._drawn:
            def draw(views, want):
                n = len(views["cams"])
                bg = torch.full((n, H, W, 3), 255, dtype=torch.uint8, device="cuda")
                return R.render_views(self.E, views, self.atlas, H, W, samples, bg=bg, want=want)

            gt = draw(self.views, ("full", "occupied"))
            rep = S * K
            many = {"cams": np.repeat(self.views["cams"], rep, axis=0), "spheres": self.tables.reshape(B * V * rep, S, 16),
                    "tex_index": np.repeat(self.views["tex_index"], rep, axis=0), "count": np.repeat(self.views["count"], rep, axis=0)}
            cand = draw(many, ("full",))["full"].view(B * V, S, K, H, W, 3)
            self._drawn[samples] = types.SimpleNamespace(gt=gt["full"], occ=gt["occupied"], cand=cand, gt_h=gt["full"].cpu().numpy(),
                                                         occ_h=gt["occupied"].cpu().numpy(), cand_h=cand.cpu().numpy())
        return self._drawn[samples]

    def run(self, gen, samples, *, shift=None, rows=B, row0=0, n_valid=B, out=None, win_host=True):
        d = self.drawn(samples)
        if out is None:
            out = torch.full((rows, V, S, K, 4), MARK, dtype=torch.int64, device="cuda")
        self.E.openloop_orientation(gen, d.gt, d.occ, self.dev["win"], self.dev["cams"], self.dev["spheres"], self.dev["tex_index"], self.dev["count"],
                                    self.atlas, self.dev["rot"], out, samples=samples, shift=shift, row0=row0, n_valid=n_valid,
                                    win_host=self.win if win_host else None)
        return out


@pytest.fixture(scope="module")
def world(engine):
    return _World(engine)


def _gen(views_u8, tiled):
    """uint8 [B * V, H, W, 3] per view -> the device tensor in the layout asked for."""
    return torch.from_numpy(OF.tile(views_u8) if tiled else views_u8.reshape(B, V, H, W, 3)).cuda()


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("tiled", [True, False])
def test_costs_equal_the_integer_sums_over_the_renderers_own_candidates(world, tiled, samples):
    d = world.drawn(samples)
    assert d.occ_h.any(axis=(1, 2)).all() and not np.array_equal(d.cand_h[:, :, 0], d.cand_h[:, :, K - 1])
    assert np.array_equal(d.cand_h[:, :, K // 2], np.repeat(d.gt_h[:, None], S, axis=1))  # the identity candidate is the ground truth, bit for bit
    rng = np.random.RandomState(3 + samples)
    gen = rng.randint(0, 256, (B * V, H, W, 3)).astype(np.uint8)
    shift = rng.randint(-6, 7, (B * V, S, 2)).astype(np.int32)
    shift[0, 0], shift[5, 1] = (130, -200), (-128, 127)  # clamped into [-127, 127]
    want = OF.orientation_sums(d.cand_h, gen, d.gt_h, d.occ_h, world.win, shift).reshape(B, V, S, K, 4)
    assert (want[..., 1] <= want[..., 3]).all() and (want[..., 1] < want[..., 3]).any() and (want[..., 3] >= 100).any()
    got = world.run(_gen(gen, tiled), samples, shift=torch.from_numpy(shift).cuda(), rows=4, row0=1).cpu().numpy()
    assert (got[0] == MARK).all() and (got[3] == MARK).all()  # the rows of other batches are not touched
    assert np.array_equal(got[1:3], want)
    # no shift table = zeros; the same bits again, with and without the host copy of the windows
    plain = OF.orientation_sums(d.cand_h, gen, d.gt_h, d.occ_h, world.win).reshape(B, V, S, K, 4)
    a, b = world.run(_gen(gen, tiled), samples).cpu().numpy(), world.run(_gen(gen, tiled), samples, win_host=False).cpu().numpy()
    assert np.array_equal(a, plain) and np.array_equal(b, plain) and np.array_equal(plain[..., 1], plain[..., 3])
    zero = world.run(_gen(gen, tiled), samples, shift=torch.zeros((B * V, S, 2), dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.array_equal(zero, plain)
    # a padded last batch: only the first sample is scored
    one = world.run(_gen(gen, tiled), samples, n_valid=1).cpu().numpy()
    assert np.array_equal(one[0], plain[0]) and (one[1] == MARK).all()


def test_a_planted_rotation_on_the_grid(world):
    samples, j = 4, 5  # candidate 5 is +10 degrees
    d = world.drawn(samples)
    n_readable = 0
    for s in range(S):  # gen = the kernel's own render of the view with sphere s at candidate j
        got = world.run(_gen(np.ascontiguousarray(d.cand_h[:, s, j]), True), samples).cpu().numpy().reshape(B * V, S, K, 4)[:, s]
        for i in range(B * V):
            x0, y0, wd, ht = OF.clamp_window(world.win[i, s], H, W)
            n_occ = int((d.occ_h[i, y0: y0 + ht, x0: x0 + wd] != 0).sum())
            assert got[i, j, 0] == 0 and (got[i, :, 1] == n_occ).all() and (got[i, :, 3] == n_occ).all(), (i, s)
            assert got[i, K // 2, 2] == 0, (i, s)
            if got[i, :, 2].max() > got[i, :, 2].min():  # readable: the window shows its own sphere
                n_readable += 1
                assert (np.delete(got[i, :, 0], j) > 0).all(), (i, s, got[i, :, 0].tolist())
                assert int(np.argmin(got[i, :, 0])) == j and int(np.argmin(got[i, :, 2])) == K // 2
            elif s >= world.views["count"][i]:
                assert (got[i, :, 2] == 0).all()  # an undrawn slot: every candidate is the unchanged view
    assert n_readable >= B * V  # at least one readable sphere per view on average


@pytest.mark.parametrize("dx,dy", [(3, -2), (45, -38)])
def test_a_moved_generated_image_is_read_through_the_shift(world, dx, dy):
    samples = 4
    d = world.drawn(samples)
    rng = np.random.RandomState(9)
    gen = rng.randint(0, 256, (B * V, H, W, 3)).astype(np.uint8)
    moved = np.zeros_like(gen)  # moved[y + dy, x + dx] = gen[y, x]
    ys, yd = (slice(-dy, H), slice(0, H + dy)) if dy < 0 else (slice(0, H - dy), slice(dy, H))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    moved[:, yd, xd] = gen[:, ys, xs]
    base = world.run(_gen(gen, True), samples).cpu().numpy().reshape(B * V, S, K, 4)
    shift = torch.from_numpy(np.tile(np.array([dx, dy], np.int32), (B * V, S, 1))).cuda()
    got = world.run(_gen(moved, True), samples, shift=shift).cpu().numpy().reshape(B * V, S, K, 4)
    assert np.array_equal(got[..., 2:], base[..., 2:])  # the ground-truth sums do not see the shift
    whole = cut = 0
    for i in range(B * V):
        for s in range(S):
            x0, y0, wd, ht = OF.clamp_window(world.win[i, s], H, W)
            py, px = np.nonzero(d.occ_h[i, y0: y0 + ht, x0: x0 + wd])
            inside = (px + x0 + dx >= 0) & (px + x0 + dx < W) & (py + y0 + dy >= 0) & (py + y0 + dy < H)
            assert (got[i, s, :, 1] == inside.sum()).all() and (base[i, s, :, 1] == len(px)).all(), (i, s)
            if inside.all():  # the shifted window stays inside the view: the unshifted result
                whole += len(px) > 0
                assert np.array_equal(got[i, s], base[i, s]), (i, s)
            else:
                cut += 1
                assert (got[i, s, :, 0] <= base[i, s, :, 0]).all()
    assert whole > 0 and (cut > 0 or (dx, dy) == (3, -2))


def test_refused_arguments_leave_the_output_untouched(engine):
    lib, ctx = engine.lib, engine._ctx
    b, v, h, w, s, k, T, th, tw = 1, 4, 64, 64, 2, 3, 2, 8, 8  # every buffer holds these shapes: a call accepted by mistake would still stay inside them
    gen, gt = (torch.zeros(b * v * h * w * 3, dtype=torch.uint8, device="cuda") for _ in range(2))
    occ = torch.zeros(b * v * h * w, dtype=torch.uint8, device="cuda")
    win_h = np.tile(np.array([[0, 0, 8, 8], [54, 54, 64, 64]], np.int32), (b * v, 1, 1))
    win = torch.zeros(b * v * s * 4 + 4, dtype=torch.int32, device="cuda")
    win[: b * v * s * 4] = torch.from_numpy(win_h.reshape(-1)).cuda()
    cams, sph = torch.zeros(b * v * 18 + 4, device="cuda"), torch.zeros(b * v * s * 16 + 4, device="cuda")
    tex, cnt = torch.zeros(b * v * s + 4, dtype=torch.int32, device="cuda"), torch.zeros(b * v + 4, dtype=torch.int32, device="cuda")
    atlas = torch.zeros(T * th * tw * 4 + 4, dtype=torch.uint8, device="cuda")
    rot, shift = torch.zeros(k * 9 + 4, device="cuda"), torch.zeros(b * v * s * 2 + 4, dtype=torch.int32, device="cuda")
    n_out = b * v * s * k * 4
    out = torch.full((n_out + 2,), MARK, dtype=torch.int64, device="cuda")
    ok = dict(gen=gen.data_ptr(), gt=gt.data_ptr(), occ=occ.data_ptr(), win=win.data_ptr(), host=None, cams=cams.data_ptr(), sph=sph.data_ptr(),
              tex=tex.data_ptr(), cnt=cnt.data_ptr(), atlas=atlas.data_ptr(), rot=rot.data_ptr(), shift=shift.data_ptr(), out=out.data_ptr(), B=b, V=v, H=h, W=w,
              S=s, K=k, T=T, th=th, tw=tw, samples=4, tiled=1, row0=0, n_valid=b, rows=b)

    def call(a):
        return lib.gn_openloop_orientation(ctx, a["gen"], a["gt"], a["occ"], a["win"], a["host"], a["cams"], a["sph"], a["tex"], a["cnt"], a["atlas"], a["rot"],
                                           a["shift"], a["out"], a["B"], a["V"], a["H"], a["W"], a["S"], a["K"], a["T"], a["th"], a["tw"], a["samples"],
                                           a["tiled"], a["row0"], a["n_valid"], a["rows"])

    bad = [dict(gen=None), dict(gt=None), dict(occ=None), dict(win=None), dict(cams=None), dict(sph=None), dict(tex=None), dict(cnt=None), dict(atlas=None),
           dict(rot=None), dict(out=None), dict(K=0), dict(K=65), dict(K=-1), dict(samples=0), dict(samples=2), dict(samples=8), dict(B=0), dict(H=0),
           dict(W=-1), dict(S=0), dict(S=9), dict(V=3), dict(V=5), dict(T=0), dict(th=0), dict(tw=-2), dict(n_valid=-1), dict(n_valid=b + 1), dict(row0=-1),
           dict(row0=1), dict(rows=0), dict(win=win.data_ptr() + 2), dict(cams=cams.data_ptr() + 2), dict(sph=sph.data_ptr() + 1), dict(tex=tex.data_ptr() + 2),
           dict(cnt=cnt.data_ptr() + 2), dict(atlas=atlas.data_ptr() + 1), dict(rot=rot.data_ptr() + 2), dict(shift=shift.data_ptr() + 2),
           dict(out=out.data_ptr() + 4)]
    for first in ([0, 0, 65, 2], [0, 0, 2, 65], [-1, 0, 3, 3], [0, -1, 3, 3], [5, 0, 3, 4], [0, 5, 4, 3]):
        hh = win_h.copy()
        hh[b * v - 1, s - 1] = first  # the last window of the table
        bad.append(dict(host=hh))
    for change in bad:
        a = dict(ok, **change)
        if isinstance(a["host"], np.ndarray):
            a["host"] = a["host"].ctypes.data
        assert call(a) != 0, change
    assert call(dict(ok, n_valid=0)) == 0  # accepted, and does nothing
    torch.cuda.synchronize()
    assert bool((out == MARK).all())
    # ... and the unchanged arguments are accepted, with and without the host copy and the shift table: nothing is occupied, so four zeros each
    for extra in (dict(), dict(host=win_h.ctypes.data), dict(shift=None)):
        out.fill_(MARK)
        assert call(dict(ok, **extra)) == 0
        torch.cuda.synchronize()
        assert bool((out[:n_out] == 0).all()) and bool((out[n_out:] == MARK).all())
    from genima_amd.engine import Engine

    with pytest.raises(RuntimeError, match="eager"):
        Engine("cuda:0", record=True).openloop_orientation(gen.view(b, 2 * h, 2 * w, 3), gt.view(b * v, h, w, 3), occ.view(b * v, h, w),
                                                           win[: b * v * s * 4].view(b * v, s, 4), cams[: b * v * 18].view(b * v, 18),
                                                           sph[: b * v * s * 16].view(b * v, s, 16), tex[: b * v * s].view(b * v, s), cnt[: b * v],
                                                           atlas[: T * th * tw * 4].view(T, th, tw, 4), rot[: k * 9].view(k, 9), out[:n_out].view(b, v, s, k, 4))


# ---- end to end: tests/test_openloop_spheres_gpu.py's world (64 x 64, two episodes, 13 transitions, batch 3), diffusion only
CAMS = P.DEFAULT_CAMERAS
SIZE, LENGTHS, BATCH, SEED = 64, (6, 9), 3, 2
N = sum(L - 1 for L in LENGTHS)


def test_the_evaluator_fills_the_orientation_table_and_changes_nothing_else(engine, tmp_path):
    cfg, eps = RR.episodes(LENGTHS, SIZE, CAMS)
    eps = [(demo, P.synthetic_demo(len(demo["gripper_open"]), seed=20 + e, size=SIZE, cameras=CAMS)[1], traj, desc) for e, (demo, traj, desc) in enumerate(eps)]
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=2 * SIZE, vae_slicing=False, upcast_vae=False,
                               fused_projections=True, enable_xformers_memory_efficient_attention=True, show_diffusion_progress=False, torch_compile=False,
                               autoencoder="")
    dagent = SDControlNetAgent(ns)

    def evaluator(**kw):
        return OpenLoopEval(dagent, None, eps, CAMS, render_cfg=cfg, stats=None, tokenizer=RR.tokens, batch_size=BATCH, seed=SEED, engine=engine, **kw)

    plain = evaluator().run()
    ev = evaluator(orientation=K)
    res = ev.run()
    assert plain.orientation is None and plain.orientation_summary() is None
    assert np.array_equal(res.image, plain.image) and np.array_equal(res.spheres, plain.spheres) and np.array_equal(res.windows, plain.windows)
    assert res.orientation.shape == (N, 4, 4, K, 4) == (13, 4, 4, 7, 4) and res.orientation.dtype == np.int64
    assert np.array_equal(res.orientation_angles, orientation_candidates(K)[0])
    ori = res.orientation
    assert (ori[..., 1] == ori[..., :1, 1]).all() and (ori[..., 3] == ori[..., :1, 3]).all() and (ori[..., 1] <= ori[..., 3]).all()
    assert (ori[..., K // 2, 2] == 0).all()  # the identity candidate against the ground truth
    assert np.array_equal(ori[..., 0, 3], res.spheres[..., 9])  # the pixels summed are the window's occupied pixels: the sphere table's n_occ
    sc = res.orientation_scores()
    drawn = res.sphere_drawn()
    assert (drawn & sc["readable"]).any() and (sc["floor_deg"][drawn & sc["readable"]] == 0.0).all()
    s = res.orientation_summary()
    assert s["overall"]["floor_deg"] == 0.0 and all(f in (0.0, None) for f in s["floor_deg"].values())
    assert (ori[[4, 12]] == 0).all()  # the steps that draw no sphere
    assert "orientation" in res.to_json(str(tmp_path / "with.json")) and "orientation" not in plain.to_json(str(tmp_path / "without.json"))
    # one batch recomputed outside the evaluator: the shift rule in numpy f64, the candidates from gn_render_spheres, the sums from orientation_ref
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    with torch.inference_mode():
        for k in range(2):
            idx = ev.batch_indices(k * BATCH)
            batch = ev.targets(idx)
            out = ev.generate(batch, idx, gen)
    t = res.spheres[idx].astype(np.float64)
    ok = (t[..., 1] > 0) & (t[..., 5] > 0) & (t[..., 1] >= SHIFT_FOUND_MASS * t[..., 5])
    with np.errstate(invalid="ignore", divide="ignore"):
        shift = np.stack([np.rint(t[..., 2] / t[..., 1] - t[..., 6] / t[..., 5]), np.rint(t[..., 3] / t[..., 1] - t[..., 7] / t[..., 5])], axis=-1)
    shift = np.where(ok[..., None], shift, 0.0).astype(np.int32).reshape(BATCH * 4, 4, 2)
    views = {k2: v.cpu().numpy() for k2, v in batch["views"].items()}
    rot = orientation_candidates(K)[1]
    tables = OF.candidate_tables(views["spheres"], rot)
    rep = 4 * K
    many = {"cams": np.repeat(views["cams"], rep, axis=0), "spheres": tables.reshape(-1, 4, 16), "tex_index": np.repeat(views["tex_index"], rep, axis=0),
            "count": np.repeat(views["count"], rep, axis=0)}
    bg = torch.full((BATCH * 4 * rep, SIZE, SIZE, 3), 255, dtype=torch.uint8, device="cuda")
    cand = R.render_views(engine, many, ev.atlas, SIZE, SIZE, ev.samples, bg=bg, want=("full",))["full"].view(BATCH * 4, 4, K, SIZE, SIZE, 3).cpu().numpy()
    # the evaluator's ground truth is composited over the frames; the candidates are compared with it as it is
    want = OF.orientation_sums(cand, OF.untile(out.cpu().numpy()), batch["full"].cpu().numpy(), batch["occupied"].cpu().numpy(),
                               res.windows[idx].reshape(BATCH * 4, 4, 4), shift)
    assert np.array_equal(ori[idx], want.reshape(BATCH, 4, 4, K, 4)) and list(idx) == [3, 4, 5]
