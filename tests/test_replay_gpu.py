"""-m gpu: the device-resident ACT replay -- ``gn_replay_gather`` against the numpy restatement bit for bit (clamps at episode ends, chunked
and misaligned frames, out-of-range indices), its conversion against ``gn_image_u8_to_f16``, the device route of ``GenimaACT`` against the
host-batch route, the training loop end to end, and ``actor_grad_clip``.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import replay_ref as R
from genima_amd import configs
from genima_amd import replay as P
from genima_amd._lib import GenimaHipError
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu

LENGTHS, T = (3, 6), 4
CAMS = ("left_shoulder", "right_shoulder", "front", "wrist")


def _episodes(lengths, cams, H, W, seed):
    rng = np.random.RandomState(seed)
    eps = []
    for L in lengths:
        demo = {"joint_positions": rng.randn(L, 7), "gripper_open": (rng.rand(L) > 0.5).astype(np.float64)}
        frames = {c: rng.randint(0, 256, (L, H, W, 3)).astype(np.uint8) for c in cams}
        eps.append((demo, frames, f"task {L}"))
    eps[0][1][cams[0]][0].reshape(-1)[:105] = np.arange(105) * 2 + 1  # many distinct byte values in one frame
    return eps


def _tokens(texts):
    t = np.zeros((1, 77), np.int32)
    t[0, :4] = [1000, 1 + sum(map(ord, texts[0])) % 900, 7, 1023]  # the last one is the highest id: the EOT position
    return t


def _reference(eps, cams, lengths):
    """The tables and the expected batch source, from replay_ref and the formulas alone."""
    acts = [R.actions_of(d["joint_positions"], d["gripper_open"]) for d, _, _ in eps]
    st = R.action_stats_of(np.concatenate(acts))
    ps = R.proprio_stats_of(np.concatenate(acts))
    action = np.concatenate(acts).astype(np.float64)
    action[:, :-1] = (action[:, :-1] - st["mean"][:-1]) / st["std"][:-1]
    qpos = np.concatenate([R.low_dim_state_of(d["joint_positions"], d["gripper_open"]) for d, _, _ in eps]).astype(np.float64)
    qpos[:, 1:] = (qpos[:, 1:] - ps["mean"][1:]) / (ps["std"][1:] + 1e-10)
    frames = np.stack([f[c][t] for (d, f, _), L in zip(eps, lengths) for t in range(L) for c in cams])
    return frames, qpos.astype(np.float32), action.astype(np.float32), R.tables(lengths)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_batch(got, want):
    img, img8, low, act = want
    assert got["images"].dtype == torch.float16 and got["images_u8"].dtype == torch.uint8
    assert np.array_equal(_bits(got["images"]).cpu().numpy(), img.view(np.int16))
    assert np.array_equal(got["images_u8"].cpu().numpy(), img8)
    assert np.array_equal(_bits(got["low_dim_state"]).cpu().numpy(), low.view(np.int32))
    assert np.array_equal(_bits(got["action"]).cpu().numpy(), act.view(np.int32))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("fs", [1, 3])
@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (37, 31)])  # 35 pixels: pixels % 4 = 3, and every other uint8 output frame off the dword grid; 1147: two blocks
def test_kernel_matches_the_restatement_bit_for_bit(engine, H, W, V, fs, B):
    cams = CAMS[:V]
    eps = _episodes(LENGTHS, cams, H, W, seed=H * 100 + V * 10 + fs)
    stride = (H * W * 3 + 3) // 4 * 4
    rp = P.DeviceReplay(eps, cams, engine=engine, frame_stack=fs, action_sequence=T, batch_size=2, tokenizer=_tokens, chunk_bytes=3 * stride)
    frames, qpos, action, (obs_index, first_obs, last_tr, episode) = _reference(eps, cams, LENGTHS)
    assert (rp.N, rp.N_obs, rp.V, rp.S, rp.A) == (7, 9, V, 8, 8) and len(rp.chunks) == -(-9 * V // 3) and rp.frames_per_chunk == 3
    assert np.array_equal(rp.host["obs_index"], obs_index) and np.array_equal(rp.host["first_obs"], first_obs)
    assert np.array_equal(rp.host["last_tr"], last_tr) and np.array_equal(rp.host["episode"], episode)
    assert np.array_equal(rp.host["qpos"].view(np.int32), qpos.view(np.int32)) and np.array_equal(rp.host["action"].view(np.int32), action.view(np.int32))
    # one frame pointer 1 byte off the dword grid: the first observation of episode 2, camera 0 (read by transition 2 at every fs)
    i = 3 * V
    off = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device="cuda")
    off[1: 1 + H * W * 3] = torch.from_numpy(frames[i].reshape(-1)).cuda()
    rp.frame_ptr[i] = off.data_ptr() + 1
    assert (off.data_ptr() + 1) % 4 == 1
    idx = [6] if B == 1 else [0, 1, 2, 6, 2]  # every episode's first and last transition, one of them twice
    want = R.gather(idx, frames, qpos, action, obs_index, first_obs, last_tr, V, fs, T)
    got = rp.sample(idx, want_u8=True)  # host indices: checked and uploaded
    assert tuple(got["images"].shape) == (B, V * fs, H, W, 8) and tuple(got["low_dim_state"].shape) == (B, fs, 8)
    assert tuple(got["action"].shape) == (B, T, 8) and tuple(got["lang_tokens"].shape) == (B, 1, 77)
    _assert_batch(got, want)
    _assert_batch(rp.sample(torch.tensor(idx, dtype=torch.int32, device="cuda"), want_u8=True), want)  # indices already on the device
    assert np.array_equal(got["lang_tokens"].cpu().numpy()[:, 0], np.concatenate([_tokens([eps[episode[n]][2]]) for n in idx]))
    assert got["reward"].tolist() == [1.0] * B
    assert "images_u8" not in rp.sample(idx)
    # the conversion is gn_image_u8_to_f16's with mul 1, add 0
    conv = engine.image_u8_to_f16(got["images_u8"].view(B * V * fs, H, W, 3), 8, 1.0, 0.0)
    assert torch.equal(_bits(conv.view_as(got["images"])), _bits(got["images"]))
    # ... and host_batch is the same sample in RoboBase's shapes
    hb = rp.host_batch(idx)
    assert [k for k in hb if k.endswith("_rgb")] == [f"{c}_rgb" for c in cams]
    stacked = np.stack([hb[f"{c}_rgb"] for c in cams], axis=1).reshape(B, V * fs, 3, H, W).transpose(0, 1, 3, 4, 2)
    assert np.array_equal(stacked, want[1]) and np.array_equal(hb["low_dim_state"].view(np.int32), want[2].view(np.int32))
    assert np.array_equal(hb["action"].view(np.int32), want[3].view(np.int32)) and hb["lang_tokens"].shape == (B, fs, 77)


def test_out_of_range_indices_are_clamped_and_nothing_else_is_written(engine):
    H, W, V, fs = 5, 7, 2, 3
    eps = _episodes(LENGTHS, CAMS[:V], H, W, seed=9)
    rp = P.DeviceReplay(eps, CAMS[:V], engine=engine, frame_stack=fs, action_sequence=T, batch_size=2)
    B, G = 2, 64  # G: guard elements on either side of every output
    shapes = ((B, V * fs, H, W, 8), torch.float16, 7.0), ((B, V * fs, H, W, 3), torch.uint8, 201), ((B, fs, 8), torch.float32, -5.0), ((B, T, 8), torch.float32, -5.0)
    flat = [torch.full((int(np.prod(s)) + 2 * G,), v, dtype=dt, device="cuda") for s, dt, v in shapes]
    out = tuple(f[G: f.numel() - G].view(s) for f, (s, _, _) in zip(flat, shapes)) + (None,)
    idx = torch.tensor([rp.N, -1], dtype=torch.int32, device="cuda")
    engine.replay_gather(rp.frame_ptr, rp.qpos, rp.action, rp.obs_index, rp.first_obs, rp.last_tr, idx, (H, W), V, fs, T, out=out)
    torch.cuda.synchronize()
    want = rp.sample([rp.N - 1, 0], want_u8=True)
    for o, k in zip(out, ("images", "images_u8", "low_dim_state", "action")):
        assert torch.equal(_bits(o), _bits(want[k])), k
    for f, (_, _, v) in zip(flat, shapes):
        assert bool((f[:G] == v).all()) and bool((f[-G:] == v).all())
    for bad in ([rp.N], [-1], [0, rp.N + 5], []):  # host-made indices are checked before the upload
        with pytest.raises(GenimaHipError):
            rp.sample(bad)
    with pytest.raises(ValueError):
        rp.host_batch([rp.N])


def test_capacity_bound_raises_before_allocating(engine):
    eps = _episodes(LENGTHS, CAMS[:1], 8, 8, seed=2)
    with pytest.raises(ValueError, match="capacity_bytes"):
        P.DeviceReplay(eps, CAMS[:1], engine=engine, capacity_bytes=9 * 192 - 1)
    assert P.DeviceReplay(eps, CAMS[:1], engine=engine, capacity_bytes=9 * 192).device_bytes == 9 * 192


def test_record_mode_refuses_replay_gather():
    E = Engine("cuda:0", record=True)
    z = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError, match="eager"):
        E.replay_gather(z, z, z, z, z, z, z, (8, 8), 1, 1, 4)


# ------------------------------------------------------------------------------------------------------------ the agent's two routes
def _agent(seed=4):
    from genima_amd.act import GenimaACT

    cfg, ccfg = dict(configs.TINY_ACT_POLICY, data_augmentation=True), configs.TINY_ACT_CLIP_TEXT
    return GenimaACT(cfg, None, ccfg, None, device="cuda", seed=seed), cfg, ccfg


def _tiny_replay(engine=None, lengths=(4, 5), batch_size=2, root=None, **kw):
    cfg = configs.TINY_ACT_POLICY
    eps = []
    for e, L in enumerate(lengths):
        demo, frames = P.synthetic_demo(L, seed=20 + e, size=cfg["image_size"], cameras=CAMS)
        if root is not None:
            P.write_episode(os.path.join(root, f"episode{e}"), demo, frames, f"open box {e}")
            eps.append(os.path.join(root, f"episode{e}"))
        else:
            eps.append((demo, frames, f"open box {e}"))
    return P.DeviceReplay(eps, CAMS, engine=engine, action_sequence=cfg["num_queries"], batch_size=batch_size, tokenizer=_tokens, **kw)


def _obs(rp, idx):
    hb = rp.host_batch(idx)
    return {k: torch.as_tensor(v) for k, v in hb.items() if k not in ("action", "reward")}


def test_device_route_equals_host_batch_route(engine):
    from genima_amd.act_training import act_augment

    rp = _tiny_replay(engine)
    a_dev, cfg, _ = _agent()
    a_host, _, _ = _agent()
    steps = ([0, 3], [6, 2], [5, 5])
    for i, ix in enumerate(steps):
        torch.manual_seed(100 + i)  # the Gaussian noise of the augmentation comes from the device's global generator
        m_dev = a_dev.update_device(rp.sample(ix), i, lr=1e-3, lr_backbone=1e-4)
        torch.manual_seed(100 + i)
        m_host = a_host.update(iter([rp.host_batch(ix)]), i, lr=1e-3, lr_backbone=1e-4)
        print(i, m_dev, m_host)
        assert set(m_dev) == {"actor_loss", "actor_l1_loss", "actor_gripper_loss", "actor_kl_loss", "batch_reward"}
        assert m_dev == m_host, i
    obs = _obs(rp, [1, 4])
    assert torch.equal(a_dev.act(obs), a_host.act(obs))
    # the augmented tensor itself: the f16 input skips the first conversion and is left as it was
    s = rp.sample([0, 3], want_u8=True)
    keep = s["images"].clone()
    torch.manual_seed(7)
    x16 = act_augment(engine, s["images"], torch.Generator().manual_seed(5))
    torch.manual_seed(7)
    x8 = act_augment(engine, s["images_u8"], torch.Generator().manual_seed(5))
    assert torch.equal(_bits(x16), _bits(x8)) and torch.equal(_bits(s["images"]), _bits(keep))


def test_training_loop_end_to_end(tmp_path, engine):
    from genima_amd.act import GenimaACT
    from genima_amd.act_train_loop import ControllerTrainLoop
    from genima_amd.harness import load_controller_ckpt

    rp = _tiny_replay(engine, lengths=(4, 4), root=str(tmp_path / "demos"), generator=torch.Generator().manual_seed(1))
    assert rp.N == 6 and rp.descriptions == ["open box 0", "open box 1"]
    agent, cfg, ccfg = _agent()
    logged = []
    loop = ControllerTrainLoop(agent, rp, str(tmp_path / "run"), num_train_epochs=2, checkpoint_every=1, log=lambda m, i: logged.append(i))
    last = loop.train()
    assert logged == list(range(6)) and np.isfinite(list(last.values())).all()
    d = os.path.join(str(tmp_path / "run"), "snapshots", "genima_controller")
    assert sorted(os.listdir(d)) == ["0.pt", "action_stats.json", "latest.pt", "proprio_stats.json"]
    a, p = P.load_stats(d)
    assert np.array_equal(a["mean"], rp.action_stats["mean"]) and np.array_equal(p["std"], rp.proprio_stats["std"])
    obs = _obs(rp, [0, 5])
    trained = agent.act(obs).cpu()
    fresh = GenimaACT(cfg, None, ccfg, agent._clip_sd, device="cuda", seed=123)
    ck = load_controller_ckpt(fresh, os.path.join(d, "latest.pt"))
    assert set(ck) == {"cfg", "_epoch", "_num_iters", "agent"} and ck["_num_iters"] == 6
    assert torch.equal(fresh.act(obs).cpu(), trained)
    again = ControllerTrainLoop(GenimaACT(cfg, None, ccfg, agent._clip_sd, device="cuda", seed=5), rp, str(tmp_path / "run"), num_train_epochs=2,
                                checkpoint_every=1)
    assert again._epoch == 2 and again._num_iters == 6
    assert again.train() == {}  # nothing left to do


def test_actor_grad_clip(engine):
    from genima_amd.act_training import ACTTrainer, act_train_schema
    from genima_amd import weights

    cfg, ccfg = dict(configs.TINY_ACT_POLICY, kl_weight=10.0), configs.TINY_ACT_CLIP_TEXT
    sd = weights.round_to(weights.synth_state_dict(act_train_schema(cfg), 61), torch.float16)
    g = torch.Generator().manual_seed(0)
    B, V, S = 2, cfg["num_views"], cfg["image_size"]
    img = torch.randint(0, 256, (B, V, S, S, 3), generator=g, dtype=torch.uint8).cuda()
    qpos, task = torch.randn(B, cfg["state_dim"], generator=g), torch.randn(B, cfg["lang_dim"], generator=g) * 0.5
    actions = torch.rand(B, cfg["num_queries"], cfg["action_dim"], generator=g)
    eps = torch.randn(B, cfg["latent_dim"], generator=g)

    def step(**kw):
        tr = ACTTrainer(Engine("cuda:0"), cfg, sd, ccfg, None, loss_scale=256.0, seed=3, **kw)
        before = tr.cn.master.clone()
        tr.update(img, qpos, task, actions, eps)
        return tr.cn.master - before, tr.last["grad_norm"]

    d_plain, n_plain = step()
    d_none, n_none = step(actor_grad_clip=None)
    d_clip, n_clip = step(actor_grad_clip=1e-3)
    print("grad norm", n_plain, "sum |dw| unclipped", float(d_plain.abs().sum()), "clipped to 1e-3", float(d_clip.abs().sum()))
    assert torch.equal(_bits(d_none), _bits(d_plain)) and n_none == n_plain  # None: today's bits
    assert n_clip == n_plain and n_plain > 1e-3  # the reported norm is the unclipped one
    assert float(d_clip.abs().sum()) < float(d_plain.abs().sum())
    with pytest.raises(ValueError):
        ACTTrainer(Engine("cuda:0"), cfg, sd, ccfg, None, actor_grad_clip=0.0)
