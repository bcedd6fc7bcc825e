"""-m gpu: temporal ensembling of action chunks on the device (csrc/ensemble.hip) against the float64 restatement of the rule
(tests/ensemble_ref.py) -- the kernel through the engine, then the controller (eager replay and hipGraph replay) and the harness.  The reference
project never implemented its `execution_horizon` / `temporal_agg` knobs, so the pinned behaviour is the ACT paper's rule as
include/genima_hip.h restates it, not an output of the reference.

Bound of every comparison with the f64 rule: |out - ref| <= 1e-5 * max|chunk|.  Derived, not measured: at most T = 20 f32 additions of terms
whose weights are <= 1 (about 20 * 2^-24 = 1.2e-6 relative to the largest value), a few ulp of expf in each weight, one division: ~2.5e-6,
taken with roughly 4x margin."""
import types

import numpy as np
import pytest
import torch

from ensemble_ref import EnsembleRef
from genima_amd import configs, harness, schema, weights
from genima_amd._lib import GenimaHipError
from genima_amd.act import GenimaACT, act_schema

pytestmark = pytest.mark.gpu

REL_BOUND = 1e-5
CALLS, RESET_CALL = 30, 11


def _chunks(B, T, A, ld, seed, n=CALLS):
    """n chunks f32 [B, T, ld] in [-2, 2]; the pad columns hold a value that would wreck any average that read them."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n, B, T, ld, generator=g) * 4.0 - 2.0
    c[..., A:] = 1e30
    return c


def _run_kernel(E, chunks, A, h, K, m=0.01, dtype=torch.float32, first_steps=None, reset_row=None):
    """The sequence of the issue through the eager engine: steps advance by h, ``reset_row`` is reset at call RESET_CALL only.
    -> (per-call device outputs as numpy f32 [B, h, A], the per-call steps / resets fed)."""
    n, B, T, ld = chunks.shape
    state = E.action_ensemble_state(B, T, A, K)
    base = np.asarray(first_steps if first_steps is not None else [0] * B, dtype=np.int64)
    outs, fed = [], []
    for c in range(n):
        steps = base + c * h
        reset = np.zeros(B, dtype=np.uint8)
        if reset_row is not None and c == RESET_CALL:
            reset[reset_row] = 1
        out = E.action_ensemble(chunks[c].to("cuda", dtype), state, torch.from_numpy(steps.astype(np.int32)).cuda(), torch.from_numpy(reset).cuda(),
                                h, K, m, A=A)
        outs.append(out.cpu().numpy())
        fed.append((steps, reset))
    return outs, fed


def _check(outs, fed, chunks, A, h, K, m=0.01):
    n, B, T, _ = chunks.shape
    ref = EnsembleRef(B, T, A, K, h, m)
    worst = 0.0
    for c in range(n):
        want = ref(chunks[c].numpy(), fed[c][0], fed[c][1])
        assert outs[c].shape == (B, h, A) and outs[c].dtype == np.float32
        scale = float(np.abs(chunks[c].numpy()[:, :, :A]).max())
        err = float(np.abs(outs[c].astype(np.float64) - want).max()) / scale
        worst = max(worst, err)
        assert err <= REL_BOUND, f"call {c}: |out - ref| / max|chunk| = {err:.3e} > {REL_BOUND:.0e}"
    return worst


@pytest.mark.parametrize("h", [1, 5, 7, 20])
def test_kernel_matches_the_f64_rule(engine, h):
    B, T, A, ld = 2, 20, 8, 16
    K = -(-T // h)
    chunks = _chunks(B, T, A, ld, seed=10 + h)
    outs, fed = _run_kernel(engine, chunks, A, h, K, first_steps=[0, 1000], reset_row=1)
    worst = _check(outs, fed, chunks, A, h, K)
    print(f"ensemble h={h} K={K}: worst |out - ref| / max|chunk| over {CALLS} calls = {worst:.3e} (bound {REL_BOUND:.0e})")
    if K > 1:  # the reset shows: at RESET_CALL row 1 is the new chunk alone, row 0 is not
        new = chunks[RESET_CALL].numpy()[:, :h, :A]
        assert np.array_equal(outs[RESET_CALL][1], new[1]) and not np.array_equal(outs[RESET_CALL][0], new[0])


def test_kernel_f16_chunks_and_the_smallest_ring(engine):
    """The controller's a_hat is f16 with rows padded to 8: the f16 entry point against the rule on the same (exactly representable) values.
    Then B = 1, T = 3, A = 1, h = 2: the smallest shape with an evicted slot and a target step only part of the ring covers."""
    B, T, A, ld, h = 2, 20, 7, 8, 7
    chunks = _chunks(B, T, A, ld, seed=3).half().float()
    chunks[..., A:] = 60000.0
    outs, fed = _run_kernel(engine, chunks, A, h, 3, dtype=torch.float16, reset_row=1)
    _check(outs, fed, chunks, A, h, 3)
    small = _chunks(1, 3, 1, 1, seed=4)
    outs, fed = _run_kernel(engine, small, 1, 2, 2)
    _check(outs, fed, small, 1, 2, 2)
    more, fed2 = _run_kernel(engine, small, 1, 2, 5)  # more slots than chunks that can cover a step: the same actions
    _check(more, fed2, small, 1, 2, 5)


def test_same_sequence_gives_the_same_bits(engine):
    B, T, A, ld, h, K = 2, 20, 8, 16, 7, 3
    chunks = _chunks(B, T, A, ld, seed=21)
    a, _ = _run_kernel(engine, chunks, A, h, K, reset_row=1)
    b, _ = _run_kernel(engine, chunks, A, h, K, reset_row=1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("h", [5, 20])
def test_one_slot_returns_the_head_of_the_new_chunk(engine, h):
    B, T, A, ld = 2, 20, 8, 16
    chunks = _chunks(B, T, A, ld, seed=30 + h, n=6)
    outs, _ = _run_kernel(engine, chunks, A, h, 1)
    for c in range(6):
        assert np.array_equal(outs[c], chunks[c].numpy()[:, :h, :A]), f"call {c}"


def test_refusals(engine):
    """Argument checks only: every call below is refused before a launch."""
    B, T, A, ld = 2, 20, 8, 16
    chunk = torch.zeros(B, T, ld, device="cuda")
    steps, reset = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    state = engine.action_ensemble_state(B, T, A, 20)
    for h, K, what in ((0, 20, "execution horizon h"), (21, 20, "execution horizon h"), (5, 3, r"K \(3\)"), (7, 2, r"K \(2\)")):
        with pytest.raises(GenimaHipError, match=what):
            engine.action_ensemble(chunk, state, steps, reset, h, K, A=A)
    with pytest.raises(GenimaHipError):
        engine.action_ensemble(chunk, state[:64], steps, reset, 5, 4, A=A)  # a state blob too small for the shape
    with pytest.raises(GenimaHipError):
        engine.action_ensemble(chunk, state, steps, reset, 5, 4, A=ld + 1)  # ld < A
    from genima_amd.engine import Engine

    R = Engine("cuda", record=True)
    with pytest.raises(GenimaHipError, match="segment"):
        with R.segment("s"):
            R.action_ensemble(chunk, state, steps, reset, 5, 4, A=A, name="o")
    assert R.num_ops == 0


# ---- controller ---------------------------------------------------------------------------------------------------------------------------
def _agent(graph=False):
    cfg, ccfg = configs.TINY_ACT_POLICY, configs.TINY_ACT_CLIP_TEXT
    sd = weights.round_to(weights.synth_state_dict(act_schema(cfg), 31), torch.float16)
    csd = weights.round_to(weights.synth_state_dict(schema.clip_text_schema(ccfg), 32), torch.float16)
    agent = GenimaACT(cfg, sd, ccfg, csd, device="cuda")
    if graph:
        agent.enable_hip_graph(True)
    return agent, cfg, ccfg


def _observations(cfg, ccfg, n=4, B=2):
    g = torch.Generator().manual_seed(5)
    cams = ["left_shoulder", "right_shoulder", "front", "wrist"][: cfg["num_views"]]
    S, Vc = cfg["image_size"], ccfg["vocab_size"]
    toks = torch.zeros(B, 1, 77, dtype=torch.int32)
    toks[:, 0, :6] = torch.tensor([Vc - 2, 11, 12, 13, 14, Vc - 1], dtype=torch.int32)
    many = []
    for _ in range(n):
        obs = {f"{c}_rgb": torch.randint(0, 256, (B, 1, 3, S, S), generator=g, dtype=torch.uint8) for c in cams}
        obs["low_dim_state"] = torch.randn(B, 1, cfg["state_dim"], generator=g)
        obs["lang_tokens"] = toks
        many.append(obs)
    return many


@pytest.fixture(scope="module")
def controller_case():
    """One agent, four observations, the plain chunks of each (computed once, before any execution mode was set) and the op-free program."""
    agent, cfg, ccfg = _agent()
    obs = _observations(cfg, ccfg)
    plain = [agent.act(o, step=0, eval_mode=True).cpu().numpy() for o in obs]
    assert len(agent._progs) == 1
    kinds = [m["kind"] for m in next(iter(agent._progs.values())).engine.meta]
    return types.SimpleNamespace(agent=agent, cfg=cfg, ccfg=ccfg, obs=obs, plain=plain, kinds=kinds)


def _ensembled_calls(agent, obs, h, reset_before=None):
    outs = []
    for i, o in enumerate(obs):
        if i == reset_before:
            agent.reset_execution()
        outs.append(agent.act(o, step=i * h, eval_mode=True).cpu().numpy())
    return outs


def test_controller_default_is_untouched(controller_case):
    c = controller_case
    agent = c.agent
    assert "action_ensemble" not in c.kinds, "with nothing set no op is recorded"
    agent.set_execution(5, True)
    a = agent.act(c.obs[0], step=0, eval_mode=True)
    assert a.shape == (2, 5, c.cfg["action_dim"]) and a.dtype == torch.float32
    assert len(agent._progs) == 2, "the execution mode keys a program of its own"
    exe = [io for io in agent._progs.values() if io.exec is not None][0].engine
    assert [m["kind"] for m in exe.meta] == c.kinds + ["action_ensemble"], "the same forward, one op appended"
    assert all(not (s["first"] <= exe.num_ops - 1 < s["last"]) for s in exe.segments.values()), "outside every guarded segment"
    agent.set_execution()
    for o, want in zip(c.obs, c.plain):
        got = agent.act(o, step=3, eval_mode=True)
        assert got.shape == (2, c.cfg["num_queries"], c.cfg["action_dim"])
        assert np.array_equal(got.cpu().numpy(), want)


def test_controller_ensembles_its_chunks(controller_case):
    c = controller_case
    T, A, h = c.cfg["num_queries"], c.cfg["action_dim"], 5
    c.agent.set_execution(h, True)
    outs = _ensembled_calls(c.agent, c.obs, h)
    ref = EnsembleRef(2, T, A, 4, h, 0.01)
    for i, (got, chunk) in enumerate(zip(outs, c.plain)):
        want = ref(chunk, [i * h] * 2)
        err = float(np.abs(got.astype(np.float64) - want).max()) / float(np.abs(chunk).max())
        print(f"controller call {i}: |out - ref| / max|chunk| = {err:.3e}")
        assert got.shape == (2, h, A) and err <= REL_BOUND
    assert not np.array_equal(outs[3], c.plain[3][:, :h]), "the fourth call averages four chunks (else this test proves nothing)"
    # steps as a tensor [B], rows at different environment steps; the history restarts with set_execution
    c.agent.set_execution(h, True)
    ref = EnsembleRef(2, T, A, 4, h, 0.01)
    for i, (o, chunk) in enumerate(zip(c.obs, c.plain)):
        steps = torch.tensor([i * h, 40 + i * h])
        got = c.agent.act(o, step=steps if i % 2 else steps.cuda(), eval_mode=True).cpu().numpy()
        assert np.abs(got.astype(np.float64) - ref(chunk, steps.tolist())).max() <= REL_BOUND * np.abs(chunk).max()
    c.agent.set_execution()


def test_controller_reset_restarts_the_history(controller_case):
    c = controller_case
    h = 5
    c.agent.set_execution(h, True)
    outs = _ensembled_calls(c.agent, c.obs, h, reset_before=2)
    assert np.array_equal(outs[0], c.plain[0][:, :h]), "an empty history: the new chunk alone, bit for bit"
    assert not np.array_equal(outs[1], c.plain[1][:, :h])
    assert np.array_equal(outs[2], c.plain[2][:, :h]), "after reset_execution() the third call stands alone again"
    assert not np.array_equal(outs[3], c.plain[3][:, :h])
    # one row only
    c.agent.set_execution(h, True)
    c.agent.act(c.obs[0], step=0)
    c.agent.reset_execution([1])
    out = c.agent.act(c.obs[1], step=h).cpu().numpy()
    assert np.array_equal(out[1], c.plain[1][1, :h]) and not np.array_equal(out[0], c.plain[1][0, :h])
    c.agent.set_execution()


def test_controller_hip_graph_replay_equals_eager(controller_case):
    c = controller_case
    h = 5
    c.agent.set_execution(h, True)
    eager = _ensembled_calls(c.agent, c.obs, h, reset_before=3)
    c.agent.set_execution()
    gagent, _, _ = _agent(graph=True)
    plain = gagent.act(c.obs[0], step=0).cpu().numpy()
    assert np.array_equal(plain, c.plain[0]), "the captured default program returns the eager chunk"
    gagent.set_execution(h, True)
    graph = _ensembled_calls(gagent, c.obs, h, reset_before=3)
    io = [p for p in gagent._progs.values() if p.exec is not None][0]
    assert io.stream is not None and io.engine.captured
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert np.array_equal(a, b), f"call {i}: hipGraph replay differs from the eager replay"


def test_act_tiled_takes_the_step():
    fam = configs.family("tiny")
    agent = GenimaACT(fam["act"], None, fam["act_text"], None, device="cuda", seed=0)
    B, Vc = 2, fam["act_text"]["vocab_size"]
    tiled = torch.from_numpy(weights.counter_bytes(9, "act", B * 128 * 128 * 3).reshape(B, 128, 128, 3)).cuda()
    state = torch.randn(B, 1, fam["act"]["state_dim"], generator=torch.Generator().manual_seed(7)).cuda()
    toks = torch.zeros(B, 1, 77, dtype=torch.int32)
    toks[:, 0, :5] = torch.tensor([Vc - 2, 5, 6, 7, Vc - 1], dtype=torch.int32)
    whole = agent.act_tiled(tiled, state, toks).float().cpu().numpy()
    agent.set_execution(7, True)
    first = agent.act_tiled(tiled, state, toks, step=0).cpu().numpy()
    second = agent.act_tiled(tiled, state, toks, step=7).cpu().numpy()
    assert first.shape == (B, 7, fam["act"]["action_dim"]) and np.array_equal(first, whole[:, :7])
    ref = EnsembleRef(B, whole.shape[1], whole.shape[2], 3, 7, 0.01)
    ref(whole, [0, 0])
    assert np.abs(second.astype(np.float64) - ref(whole, [7, 7])).max() <= REL_BOUND * np.abs(whole).max()


# ---- harness --------------------------------------------------------------------------------------------------------------------------------
CAMERAS = ["front", "left_shoulder", "right_shoulder", "wrist"]


def test_control_step_executes_a_horizon():
    from genima_amd.agent import SDControlNetAgent

    cfg = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt="synthetic:tiny", device="cuda", image_resolution=512, vae_slicing=False,
                                upcast_vae=False, fused_projections=True, enable_xformers_memory_efficient_attention=True,
                                show_diffusion_progress=False, torch_compile=False, autoencoder="")
    dagent = SDControlNetAgent(cfg)
    acfg, ccfg = configs.ACT_POLICY, dict(configs.TINY_ACT_CLIP_TEXT, projection_dim=512)
    sd = weights.round_to(weights.synth_state_dict(act_schema(acfg), 31), torch.float16)
    csd = weights.round_to(weights.synth_state_dict(schema.clip_text_schema(ccfg), 32), torch.float16)
    cagent = GenimaACT(acfg, sd, ccfg, csd, device="cuda")
    obs = {f"{cam}_rgb": weights.counter_bytes(40 + i, "harness", 3 * 256 * 256).reshape(1, 3, 256, 256) for i, cam in enumerate(CAMERAS)}
    obs["low_dim_state"] = np.linspace(-1, 1, 8, dtype=np.float32).reshape(1, 8)
    toks = np.zeros((1, 1, 77), dtype=np.int32)
    toks[:, 0, :5] = [ccfg["vocab_size"] - 2, 5, 6, 7, ccfg["vocab_size"] - 1]
    obs["lang_tokens"] = toks

    def step(episode_step, **kw):
        gen = [torch.Generator(device="cuda").manual_seed(2)]
        return harness.control_step(dagent, cagent, obs, "open the box", CAMERAS, 1, gen, 5, 0.0, "cuda", episode_step=episode_step, **kw)[0]

    whole = step(0)
    assert whole.shape == (20, 8)
    first = step(0, execution_horizon=5, temporal_agg=True)
    assert first.shape == (5, 8) and first.dtype == np.float32
    assert np.array_equal(first, whole[:5]), "first step of an episode: nothing to average with"
    second = step(5, execution_horizon=5, temporal_agg=True)
    ref = EnsembleRef(1, 20, 8, 4, 5, 0.01)
    ref(whole[None], [0])
    assert np.abs(second.astype(np.float64) - ref(whole[None], [5])[0]).max() <= REL_BOUND * np.abs(whole).max()
    assert not np.array_equal(second, whole[:5])
    again = step(0, execution_horizon=5, temporal_agg=True)
    assert np.array_equal(again, whole[:5]), "episode_step == 0 starts a new history"
    assert cagent.execution == (5, 4, 0.01)
    assert step(10).shape == (5, 8), "the defaults leave a mode set on the controller alone"
    cagent.set_execution()
    assert np.array_equal(step(0), whole), "with nothing set the defaults return the whole chunk as before"
