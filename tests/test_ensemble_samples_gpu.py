"""-m gpu: R sampled chunks combined on the device (mean or medoid) and ensembled (csrc/ensemble.hip, gn_action_ensemble_samples_f16 and
gn_openloop_exec_actions_samples) against the float64 restatement (tests/ensemble_samples_ref.py) -- the kernels through the engine, then the
controller (eager replay and hipGraph replay) and the harness.

Bound of every comparison of actions with the f64 rule: |out - ref| <= 1e-5 * max|chunk|: tests/test_ensemble_gpu.py's derived ~2.5e-6 for the
weighted mean, plus (R + 1) * 2^-24 <= 4e-7 for the sample mean at R <= 5.  Medoid picks must EQUAL the reference's: the inputs
(ensemble_samples_ref.sample_chunks) keep the runner-up at least 1e-3 of D away, or tie exactly -- tests/test_ensemble_samples_cpu.py asserts
that for every case.  The spread is held to 1e-5 relative."""
import types

import numpy as np
import pytest
import torch

import ensemble_samples_ref as SR
from genima_amd import configs, harness, schema, weights
from genima_amd._lib import GenimaHipError
from genima_amd.act import GenimaACT, act_schema
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu

REL_BOUND = 1e-5
CALLS, RESET_CALL = 30, 11
SHAPES = ((2, 3, 20, 8, 16), (1, 5, 7, 3, 5), (2, 1, 20, 8, 16), (1, 2, 20, 8, 16))  # (B, R, T, A, ld)
_INPUTS = {}


def _inputs(shape):
    """The 30 calls of a shape, made once and shared: f32 numpy [30, B, R, T, ld] of f16-representable values."""
    if shape not in _INPUTS:
        _INPUTS[shape] = SR.sample_chunks(*shape, seed=7)
    return _INPUTS[shape]


def _settings(T):
    """h in {1, 7, T} with K = 1 and K = ceil(T / h)."""
    out = []
    for h in sorted({1, min(7, T), T}):
        for K in sorted({1, -(-T // h)}):
            out.append((h, K))
    return out


def _run(E, x, A, h, K, rule, layout="BR", reset_row=None, m=0.01):
    """The sequence through the eager engine: steps advance by h from (0, 1000, ..), ``reset_row`` is reset at call RESET_CALL.
    -> (outs [n][B, h, A], picks [n][B], spreads [n][B], final state bytes, fed)."""
    n, B, R, T, ld = x.shape
    state = E.action_ensemble_state(B, T, A, K)
    pick, spread = torch.full((B,), 77, dtype=torch.int32, device="cuda"), torch.full((B,), -5.0, device="cuda")
    outs, picks, spreads, fed = [], [], [], []
    for c in range(n):
        steps = np.arange(B, dtype=np.int64) * 1000 + c * h
        reset = np.zeros(B, dtype=np.uint8)
        if reset_row is not None and c == RESET_CALL:
            reset[reset_row] = 1
        dev = torch.from_numpy(x[c]).to("cuda", torch.float16)  # [B, R, T, ld]
        if layout == "RB":  # the same values in the evaluator's layout: samples outermost
            dev = dev.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
        elif layout == "flat":  # the controller's: rows b * R + r
            dev = dev.reshape(B * R, T, ld)
        out = E.action_ensemble(dev, state, torch.from_numpy(steps.astype(np.int32)).cuda(), torch.from_numpy(reset).cuda(), h, K, m, A=A, samples=R,
                                combine=rule, pick=pick, spread=spread)
        outs.append(out.cpu().numpy())
        picks.append(pick.cpu().numpy().copy())
        spreads.append(spread.cpu().numpy().copy())
        fed.append((steps, reset))
    return outs, picks, spreads, state.cpu().numpy(), fed


def _check(x, A, h, K, rule, outs, picks, spreads, fed, m=0.01):
    n, B, R, T, _ = x.shape
    ref = SR.EnsembleSamplesRef(B, R, T, A, K, h, m, rule)
    worst = worst_spread = 0.0
    for c in range(n):
        want, want_pick, want_spread = ref(x[c], fed[c][0], fed[c][1])
        assert outs[c].shape == (B, h, A) and outs[c].dtype == np.float32
        assert np.array_equal(picks[c], want_pick), f"call {c}: picks {picks[c]} != {want_pick}"
        err = float(np.abs(outs[c].astype(np.float64) - want).max()) / float(np.abs(x[c][..., :A]).max())
        worst = max(worst, err)
        assert err <= REL_BOUND, f"call {c}: |out - ref| / max|chunk| = {err:.3e} > {REL_BOUND:.0e}"
        nz = want_spread > 0
        assert np.array_equal(spreads[c][~nz], want_spread[~nz].astype(np.float32))
        if nz.any():
            serr = float((np.abs(spreads[c][nz].astype(np.float64) - want_spread[nz]) / want_spread[nz]).max())
            worst_spread = max(worst_spread, serr)
            assert serr <= 1e-5, f"call {c}: spread off by {serr:.3e} relative"
    return worst, worst_spread


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dR%dT%dA%dld%d" % s)
@pytest.mark.parametrize("rule", SR.RULES)
def test_kernel_matches_the_f64_rule_picks_and_spread(engine, shape, rule):
    B, R, T, A, ld = shape
    x = _inputs(shape)
    for h, K in _settings(T):
        outs, picks, spreads, _, fed = _run(engine, x, A, h, K, rule, reset_row=B - 1)
        worst, worst_spread = _check(x, A, h, K, rule, outs, picks, spreads, fed)
        print(f"{rule} B={B} R={R} T={T} h={h} K={K}: worst |out - ref| / max|chunk| = {worst:.3e} (bound {REL_BOUND:.0e}), spread {worst_spread:.3e} relative")
        if rule == "mean":
            assert all((p == -1).all() for p in picks)
        elif R >= 3:
            assert picks[SR.TIE_CALL][0] == 1, "two identical best samples: the lower index"
            assert len({int(p[0]) for p in picks}) > 1, "the medoid moves between samples (else this test proves little)"


@pytest.mark.parametrize("rule", SR.RULES)
def test_one_sample_is_the_plain_op_bit_for_bit(engine, rule):
    shape = (2, 1, 20, 8, 16)
    B, R, T, A, ld = shape
    x = _inputs(shape)
    for h, K in _settings(T):
        outs, picks, spreads, state, fed = _run(engine, x, A, h, K, rule, reset_row=1)
        plain_state = engine.action_ensemble_state(B, T, A, K)
        for c in range(CALLS):
            steps, reset = fed[c]
            want = engine.action_ensemble(torch.from_numpy(x[c][:, 0]).to("cuda", torch.float16), plain_state, torch.from_numpy(steps.astype(np.int32)).cuda(),
                                          torch.from_numpy(reset).cuda(), h, K, 0.01, A=A)
            assert outs[c].tobytes() == want.cpu().numpy().tobytes(), (h, K, c)
            assert (picks[c] == (-1 if rule == "mean" else 0)).all() and (spreads[c] == 0).all()
        assert state.tobytes() == plain_state.cpu().numpy().tobytes(), f"h={h} K={K}: the state bytes differ from gn_action_ensemble_f16's"


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "B%dR%dT%dA%dld%d" % s)
def test_the_mean_entering_the_ring_is_the_f32_sum_in_sample_order(engine, shape):
    """K = 1, h = T: the output IS the combined chunk."""
    B, R, T, A, ld = shape
    x = _inputs(shape)
    outs, _, _, _, _ = _run(engine, x, A, T, 1, "mean")
    inv_R = np.float32(1.0 / R)
    for c in range(CALLS):
        s = np.zeros((B, T, A), dtype=np.float32)
        for r in range(R):
            s = (s + x[c][:, r, :, :A]).astype(np.float32)
        assert np.array_equal(outs[c], (s * inv_R).astype(np.float32)), c


@pytest.mark.parametrize("rule", SR.RULES)
def test_layouts_and_repeats_give_the_same_bits(engine, rule):
    shape = SHAPES[0]
    B, R, T, A, ld = shape
    x = _inputs(shape)
    a = _run(engine, x, A, 7, 3, rule, reset_row=1)
    for layout in ("BR", "RB", "flat"):  # "BR" again: the same sequence twice
        b = _run(engine, x, A, 7, 3, rule, layout=layout, reset_row=1)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(a[0], b[0])), layout
        assert all(np.array_equal(p, q) for p, q in zip(a[1], b[1])) and all(p.tobytes() == q.tobytes() for p, q in zip(a[2], b[2])), layout
        assert a[3].tobytes() == b[3].tobytes(), layout


@pytest.mark.parametrize("rule", SR.RULES)
@pytest.mark.parametrize("agg", [False, True])
def test_table_replay_equals_the_controller_side_kernel(engine, rule, agg):
    """Two episodes of 9 and 14 transitions, h = 5: gn_openloop_exec_actions_samples over the [R, N] table against gn_action_ensemble_samples_f16
    called at t = 0, 5, 10 of each episode after a reset -- bit for bit, picks included; and against the f64 replay within the bound."""
    R, T, A, ld, h, lengths = 3, 20, 8, 16, 5, (9, 14)
    N = sum(lengths)
    x = _inputs(SHAPES[0])  # [30, 2, 3, T, ld]: 60 (call, row) cases, of which the first N are the transitions
    table = np.ascontiguousarray(x.reshape(60, R, T, ld)[:N].transpose(1, 0, 2, 3))  # [R, N, T, ld]
    first = np.concatenate([np.full(L, f, dtype=np.int32) for f, L in zip((0, lengths[0]), lengths)])
    dev = torch.from_numpy(table).to("cuda", torch.float16)
    n_calls = torch.zeros(N, dtype=torch.int32, device="cuda")
    res = engine.openloop_exec_actions_samples(dev, torch.from_numpy(first).cuda(), h, agg, 0.01, combine=rule, A=A, n_calls=n_calls, first_tr_host=first,
                                               pick=torch.full((N,), 9, dtype=torch.int32, device="cuda"))
    got, got_picks = res[0].cpu().numpy(), res[1].cpu().numpy()
    K = -(-T // h) if agg else 1
    for f, L in zip((0, lengths[0]), lengths):
        state = engine.action_ensemble_state(1, T, A, K)
        pick = torch.zeros(1, dtype=torch.int32, device="cuda")
        for t in range(0, L, h):
            out = engine.action_ensemble(dev[:, f + t].unsqueeze(0), state, torch.tensor([t], dtype=torch.int32, device="cuda"),
                                         torch.tensor([t == 0], dtype=torch.uint8, device="cuda"), h, K, 0.01, A=A, samples=R, combine=rule, pick=pick).cpu().numpy()
            assert int(pick.item()) == int(got_picks[f + t])
            for j in range(min(h, L - t)):
                assert got[f + t + j].tobytes() == out[0, j].tobytes(), (f, t, j)
    want, want_picks = SR.replay_table(table[..., :A], first, h, agg, 0.01, rule)
    assert np.array_equal(got_picks, want_picks)
    assert np.abs(got.astype(np.float64) - want).max() <= REL_BOUND * np.abs(table[..., :A]).max()
    calls = n_calls.cpu().numpy()
    assert calls.min() == 1 and calls.max() == (3 if agg else 1), "step 10 .. 13 of the longer episode: the calls at 0, 5 and 10"
    if agg:
        plain = engine.openloop_exec_actions(dev[0], torch.from_numpy(first).cuda(), h, agg, 0.01, A=A).cpu().numpy()
        assert not np.array_equal(plain, got), "combining changes what is executed"


def _sentinels(B, T, A, K, h):
    return (torch.full((B, h, A), 123.0, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"), torch.full((B,), -5.0, device="cuda"))


def test_refusals_launch_nothing(engine):
    """Every refusal: a non-zero status, and outputs, picks, spreads and the state exactly as they were."""
    B, R, T, A, ld, K, h = 2, 3, 20, 8, 16, 4, 5
    lib, ctx = engine.lib, engine._ctx
    chunk = torch.from_numpy(_inputs(SHAPES[0])[0]).to("cuda", torch.float16)
    steps, reset = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    state = engine.action_ensemble_state(B, T, A, K)
    state.fill_(0x5A)
    out, pick, spread = _sentinels(B, T, A, K, h)
    f32 = lambda v: float(np.float32(v))
    ok = dict(chunk=chunk.data_ptr(), bs=R * T * ld, ss=T * ld, R=R, inv_R=f32(1.0 / R), combine=1, state=state.data_ptr(), steps=steps.data_ptr(),
              reset=reset.data_ptr(), out=out.data_ptr(), pick=pick.data_ptr(), spread=spread.data_ptr(), B=B, T=T, A=A, ld=ld, K=K, h=h, m=0.01)
    bad = (dict(h=0), dict(h=T + 1), dict(K=3), dict(ld=A - 1), dict(m=-1.0), dict(m=float("nan")), dict(B=0), dict(chunk=None), dict(state=None),
           dict(steps=None), dict(reset=None), dict(out=None), dict(state=state.data_ptr() + 4), dict(out=out.data_ptr() + 2), dict(steps=steps.data_ptr() + 2),
           dict(R=0), dict(R=65, inv_R=f32(1.0 / 65)), dict(R=64, inv_R=f32(1.0 / 64), T=25, K=1, h=1),
           dict(inv_R=float(np.nextafter(np.float32(1.0 / R), np.float32(1)))), dict(inv_R=0.33333), dict(combine=2), dict(combine=-1),
           dict(chunk=chunk.data_ptr() + 1), dict(pick=pick.data_ptr() + 2), dict(spread=spread.data_ptr() + 2),
           dict(ss=(T - 1) * ld + A - 1), dict(bs=2 * T * ld + (T - 1) * ld + A - 1), dict(ss=-T * ld), dict(bs=-R * T * ld), dict(bs=T * ld, ss=T * ld))
    for kw in bad:
        a = dict(ok, **kw)
        rc = lib.gn_action_ensemble_samples_f16(ctx, a["chunk"], a["bs"], a["ss"], a["R"], a["inv_R"], a["combine"], a["state"], a["steps"], a["reset"], a["out"],
                                                a["pick"], a["spread"], a["B"], a["T"], a["A"], a["ld"], a["K"], a["h"], a["m"])
        assert rc != 0, kw
    engine.synchronize()
    assert (out == 123.0).all() and (pick == 77).all() and (spread == -5.0).all() and (state == 0x5A).all()
    # the table replay's
    N = 6
    table = chunk.reshape(N, T, ld).unsqueeze(0).expand(R, N, T, ld).contiguous()
    first = torch.zeros(N, dtype=torch.int32, device="cuda")
    ex, tp = torch.full((N, A), 123.0, device="cuda"), torch.full((N,), 77, dtype=torch.int32, device="cuda")
    ok = dict(chunks=table.data_ptr(), ns=T * ld, ss=N * T * ld, R=R, inv_R=f32(1.0 / R), combine=1, first=first.data_ptr(), ex=ex.data_ptr(), pick=tp.data_ptr(),
              N=N, T=T, A=A, ld=ld, h=h, m=0.01)
    bad = (dict(chunks=None), dict(first=None), dict(ex=None), dict(N=0), dict(A=1), dict(ld=A - 1), dict(h=0), dict(h=T + 1), dict(m=-1.0), dict(R=0), dict(R=65),
           dict(inv_R=0.33333), dict(combine=2), dict(pick=None), dict(pick=tp.data_ptr() + 2), dict(chunks=table.data_ptr() + 1), dict(ss=T * ld),
           dict(ns=T * ld - ld), dict(ss=-1))
    for kw in bad:
        a = dict(ok, **kw)
        rc = lib.gn_openloop_exec_actions_samples(ctx, a["chunks"], a["ns"], a["ss"], a["R"], a["inv_R"], a["combine"], a["first"], a["ex"], None, a["pick"], a["N"],
                                                  a["T"], a["A"], a["ld"], a["h"], 1, a["m"])
        assert rc != 0, kw
    engine.synchronize()
    assert (ex == 123.0).all() and (tp == 77).all()
    # the wrappers
    with pytest.raises(GenimaHipError, match="samples"):
        engine.action_ensemble(chunk, state, steps, reset, h, K, A=A, samples=0)
    with pytest.raises(GenimaHipError, match="combine"):
        engine.action_ensemble(chunk, state, steps, reset, h, K, A=A, samples=R, combine="median")
    with pytest.raises(GenimaHipError, match="belong to samples"):
        engine.action_ensemble(chunk[:, 0], state, steps, reset, h, K, A=A, combine="medoid")
    with pytest.raises(GenimaHipError):
        engine.action_ensemble(chunk.float(), state, steps, reset, h, K, A=A, samples=R)  # the sample op takes the controller's f16
    with pytest.raises(RuntimeError, match="eager"):
        Engine("cuda", record=True).openloop_exec_actions_samples(table, first, h)


def test_the_recorded_op_is_refused_inside_a_guarded_segment():
    B, R, T, A, ld = 2, 3, 20, 8, 16
    chunk = torch.zeros(B * R, T, ld, dtype=torch.float16, device="cuda")
    steps, reset = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    rec = Engine("cuda", record=True)
    state = rec.action_ensemble_state(B, T, A, 4)
    with pytest.raises(GenimaHipError, match="segment"):
        with rec.segment("s"):
            rec.action_ensemble(chunk, state, steps, reset, 5, 4, A=A, name="o", samples=R)
    assert rec.num_ops == 0
    out = rec.action_ensemble(chunk, state, steps, reset, 5, 4, A=A, name="o", samples=R, combine="medoid")
    assert rec.num_ops == 1 and rec.meta[-1]["kind"] == "action_ensemble_samples" and out.shape == (B, 5, A)
    rec.run()
    rec.synchronize()
    assert (out == 0).all()


# ---- controller ---------------------------------------------------------------------------------------------------------------------------
B_CTL, R_CTL = 2, 3


def _agent(graph=False):
    cfg, ccfg = configs.TINY_ACT_POLICY, configs.TINY_ACT_CLIP_TEXT
    sd = weights.round_to(weights.synth_state_dict(act_schema(cfg), 31), torch.float16)
    csd = weights.round_to(weights.synth_state_dict(schema.clip_text_schema(ccfg), 32), torch.float16)
    agent = GenimaACT(cfg, sd, ccfg, csd, device="cuda")
    if graph:
        agent.enable_hip_graph(True)
    return agent, cfg, ccfg


def _observations(cfg, ccfg, n=4, rows=B_CTL * R_CTL):
    g = torch.Generator().manual_seed(5)
    cams = ["left_shoulder", "right_shoulder", "front", "wrist"][: cfg["num_views"]]
    S, Vc = cfg["image_size"], ccfg["vocab_size"]
    toks = torch.zeros(rows, 1, 77, dtype=torch.int32)
    toks[:, 0, :6] = torch.tensor([Vc - 2, 11, 12, 13, 14, Vc - 1], dtype=torch.int32)
    many = []
    for _ in range(n):
        obs = {f"{c}_rgb": torch.randint(0, 256, (rows, 1, 3, S, S), generator=g, dtype=torch.uint8) for c in cams}
        obs["low_dim_state"] = torch.randn(rows, 1, cfg["state_dim"], generator=g)
        obs["lang_tokens"] = toks
        many.append(obs)
    return many


@pytest.fixture(scope="module")
def controller_case():
    """One agent, four observations of B * R rows, and the plain chunks of each (computed once, before any execution mode was set)."""
    agent, cfg, ccfg = _agent()
    obs = _observations(cfg, ccfg)
    plain = [agent.act(o, step=0, eval_mode=True).cpu().numpy() for o in obs]
    kinds = [m["kind"] for m in next(iter(agent._progs.values())).engine.meta]
    return types.SimpleNamespace(agent=agent, cfg=cfg, ccfg=ccfg, obs=obs, plain=plain, kinds=kinds)


def _calls(agent, obs, h, reset_before=None):
    outs = []
    for i, o in enumerate(obs):
        if i == reset_before:
            agent.reset_execution()
        outs.append(agent.act(o, step=i * h, eval_mode=True).cpu().numpy())
    return outs


@pytest.mark.parametrize("rule", SR.RULES)
def test_controller_combines_and_ensembles_its_chunks(controller_case, rule):
    c = controller_case
    T, A, h = c.cfg["num_queries"], c.cfg["action_dim"], 5
    c.agent.set_execution(h, True, samples=R_CTL, combine=rule)
    assert c.agent.execution == (h, 4, 0.01) and c.agent.execution_samples == (R_CTL, rule)
    ref = SR.EnsembleSamplesRef(B_CTL, R_CTL, T, A, 4, h, 0.01, rule)
    for i, (o, chunk) in enumerate(zip(c.obs, c.plain)):
        got = c.agent.act(o, step=i * h, eval_mode=True)
        assert got.shape == (B_CTL, h, A) and got.dtype == torch.float32
        rows = chunk.reshape(B_CTL, R_CTL, T, A)
        last = c.agent.last_samples
        assert set(last) == {"pick", "spread"} and last["pick"].is_cuda and last["spread"].is_cuda
        got_pick = last["pick"].cpu().numpy()
        if rule == "medoid":  # the controller's own chunks keep no built-in margin: a pick is held to what f32 can tell apart (1e-3 of D)
            for b in range(B_CTL):
                D = SR.medoid_distances(rows[b])
                group, margin = SR.medoid_margin(rows[b])
                assert D[got_pick[b]] <= D.min() * (1 + 1e-3) and (margin < 1e-3 or got_pick[b] == group[0]), (i, b, D, got_pick)
        want, want_pick, want_spread = ref(rows, [i * h] * B_CTL, picks=got_pick)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) / float(np.abs(chunk).max())
        print(f"controller {rule} call {i}: |out - ref| / max|chunk| = {err:.3e}")
        assert err <= REL_BOUND
        assert np.array_equal(got_pick, want_pick)
        assert np.abs(last["spread"].cpu().numpy() - want_spread).max() <= 1e-5 * want_spread.max()
    exe = [io for io in c.agent._progs.values() if io.samples == (R_CTL, rule)]
    assert len(exe) == 1 and [m["kind"] for m in exe[0].engine.meta] == c.kinds + ["action_ensemble_samples"], "the same forward, one op appended"
    assert exe[0].ens_state.numel() == exe[0].engine.lib.gn_action_ensemble_state_bytes(B_CTL, T, A, 4), "one ring per b, not per row"
    c.agent.set_execution()
    assert c.agent.last_samples is None
    for o, want in zip(c.obs, c.plain):  # the default mode is untouched
        assert np.array_equal(c.agent.act(o, step=3, eval_mode=True).cpu().numpy(), want)


def test_controller_samples_alone_reset_and_row_count(controller_case):
    c = controller_case
    T, A = c.cfg["num_queries"], c.cfg["action_dim"]
    c.agent.set_execution(samples=R_CTL)
    whole = c.agent.act(c.obs[0], step=0).cpu().numpy()
    s = np.zeros((B_CTL, T, A), dtype=np.float32)
    for r in range(R_CTL):
        s = (s + c.plain[0].reshape(B_CTL, R_CTL, T, A)[:, r]).astype(np.float32)
    assert whole.shape == (B_CTL, T, A) and np.array_equal(whole, (s * np.float32(1.0 / R_CTL)).astype(np.float32)), "samples alone: h = T, K = 1, the mean chunk"
    h = 5
    c.agent.set_execution(h, True, samples=R_CTL)
    outs = _calls(c.agent, c.obs, h, reset_before=2)
    c.agent.reset_execution()
    again = c.agent.act(c.obs[0], step=0).cpu().numpy()
    assert np.array_equal(outs[0], whole[:, :h]) and np.array_equal(again, outs[0]), "an empty history: the combined chunk alone, bit for bit"
    assert not np.array_equal(outs[1], c.agent.set_execution(samples=R_CTL).act(c.obs[1], step=0).cpu().numpy()[:, :h]), "the second call averaged two chunks"
    c.agent.set_execution(h, True, samples=4)
    with pytest.raises(GenimaHipError, match="no multiple of samples"):
        c.agent.act(c.obs[0], step=0)
    c.agent.set_execution()


def test_controller_hip_graph_replay_equals_eager(controller_case):
    c = controller_case
    h = 5
    c.agent.set_execution(h, True, samples=R_CTL, combine="medoid")
    eager = _calls(c.agent, c.obs, h, reset_before=3)
    eager_pick = c.agent.last_samples["pick"].cpu().numpy()
    c.agent.set_execution()
    gagent, _, _ = _agent(graph=True)
    gagent.set_execution(h, True, samples=R_CTL, combine="medoid")
    graph = _calls(gagent, c.obs, h, reset_before=3)
    io = [p for p in gagent._progs.values() if p.samples is not None][0]
    assert io.stream is not None and io.engine.captured
    for i, (a, b) in enumerate(zip(eager, graph)):
        assert a.tobytes() == b.tobytes(), f"call {i}: hipGraph replay differs from the eager replay"
    assert np.array_equal(gagent.last_samples["pick"].cpu().numpy(), eager_pick)


# ---- harness --------------------------------------------------------------------------------------------------------------------------------
CAMERAS = ["front", "left_shoulder", "right_shoulder", "wrist"]


def test_control_step_with_samples():
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
        out = harness.control_step(dagent, cagent, obs, "open the box", CAMERAS, 1, gen, 5, 0.0, "cuda", episode_step=episode_step, **kw)
        return out, gen[0].get_state()

    (whole, _, _, img0), state1 = step(0)
    (one, obs_after, _, img1), state_r1 = step(0, samples=1)
    assert one.shape == (20, 8) and one.tobytes() == whole.tobytes(), "R = 1 is the call without samples, bit for bit"
    assert len(img1) == 1 and np.array_equal(np.asarray(img1[0]), np.asarray(img0[0])) and torch.equal(state_r1, state1), "and draws what it draws"
    (two, obs_after, _, imgs), state2 = step(0, execution_horizon=5, temporal_agg=True, samples=2, combine="medoid")
    assert two.shape == (5, 8) and two.dtype == np.float32 and len(imgs) == 2 and obs_after["front_rgb"].shape[0] == 2
    assert not np.array_equal(np.asarray(imgs[0]), np.asarray(imgs[1])), "sequential draws from one stream: the samples see different noise"
    assert cagent.execution == (5, 4, 0.01) and cagent.execution_samples == (2, "medoid")
    # the generator moved on by R draws: two calls without samples on one generator leave it where samples=2 leaves it
    gen = [torch.Generator(device="cuda").manual_seed(2)]
    cagent.set_execution()
    for _ in range(2):
        harness.control_step(dagent, cagent, obs, "open the box", CAMERAS, 1, gen, 5, 0.0, "cuda")
    assert torch.equal(gen[0].get_state(), state2) and not torch.equal(state2, state1)
    cagent.set_execution()
    assert step(0)[0][0].tobytes() == whole.tobytes(), "with nothing set the defaults return the whole chunk as before"
