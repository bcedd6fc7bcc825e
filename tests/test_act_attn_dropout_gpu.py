"""-m gpu: attention-probability dropout from the tape to the ACT update (training.Graph.attention, act_training.ACTTrainer(attn_dropout),
GenimaACT.update's ``attn_dropout`` config key), on the tiny ACT config of tests/test_act_training_gpu.py:
  (1) attn_dropout = 0.0 is the trainer without the argument, bit for bit; (2) at 0.1 the update is a function of the trainer seed, its
  per-call seeds are distinct within and between steps, the loss is finite; (3) Graph.attention at D = 64: the flash route and the
  materialised route evaluate one mask and sit inside their f64 bounds (tests/attention_dropout_ref.py); (4) the mask reaches the loss;
  (5) the agent's config key (and a trainer_kw of the same name) reaches the trainer."""
import pytest
import torch

import attention_dropout_ref as DR
import attention_ref as R
from act_ops_ref import bits_equal
from genima_amd import configs, weights
from genima_amd.act_training import ACTTrainer, act_train_schema, attn_call_seed
from genima_amd.training import Graph, Var
from util import q16

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32


def _setup(seed=0):
    cfg, ccfg = dict(configs.TINY_ACT_POLICY, kl_weight=10.0), configs.TINY_ACT_CLIP_TEXT
    sd = weights.round_to(weights.synth_state_dict(act_train_schema(cfg), 61), torch.float16)
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = sd[k].abs() + 0.5
    g = torch.Generator().manual_seed(seed)
    B, V, S = 2, cfg["num_views"], cfg["image_size"]
    images = torch.randint(0, 256, (B, V, S, S, 3), generator=g, dtype=torch.uint8).cuda()
    qpos = q16(torch.randn(B, cfg["state_dim"], generator=g))
    task = q16(torch.randn(B, cfg["lang_dim"], generator=g) * 0.5)
    actions = q16(torch.randn(B, cfg["num_queries"], cfg["action_dim"], generator=g))
    eps = torch.randn(B, cfg["latent_dim"], generator=g)
    return cfg, ccfg, sd, (images, qpos, task, actions, eps)


def _trainer(engine, cfg, ccfg, sd, **kw):
    return ACTTrainer(engine, cfg, sd, ccfg, None, loss_scale=256.0, **kw)


def _fb(tr, batch):
    """One forward_backward -> (out4, flat gradient), both cloned on the host."""
    out4 = tr.forward_backward(*batch).cpu().clone()
    return out4, tr.cn.grad.cpu().clone()


def test_zero_is_the_trainer_without_the_argument(engine):
    """attn_dropout = 0.0 runs no new code: out4 and the flat gradient have the bits of a trainer built without the argument (the other
    dropouts on, drawn from the trainer's generator as before)."""
    cfg, ccfg, sd, batch = _setup()
    a = _fb(_trainer(engine, cfg, ccfg, sd, seed=3), batch)
    tr = _trainer(engine, cfg, ccfg, sd, seed=3, attn_dropout=0.0)
    b = _fb(tr, batch)
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]) and tr.last_attn_seeds == []


def test_update_is_a_function_of_the_trainer_seed(engine):
    cfg, ccfg, sd, batch = _setup()
    n_calls = 2 * cfg["enc_layers"] + 2 * cfg["dec_layers"]  # CVAE encoder + encoder self-attention, decoder self- + cross-attention
    t1, t2, t3 = (_trainer(engine, cfg, ccfg, sd, seed=s, attn_dropout=0.1, dropout=0.0, state_dropout=0.0) for s in (3, 3, 4))
    (o1, g1), (o2, g2), (o3, g3) = (_fb(t, batch) for t in (t1, t2, t3))
    assert bits_equal(o1, o2) and bits_equal(g1, g2), "one seed, one update"
    assert not bits_equal(g1, g3), "another seed, other masks"
    assert torch.isfinite(o1).all() and torch.isfinite(g1).all()
    s0 = list(t1.last_attn_seeds)
    assert len(s0) == n_calls and s0 == t2.last_attn_seeds and s0 == [attn_call_seed(3, 0, i) for i in range(n_calls)]
    t1.optimizer_step()
    m = t1.update(*batch)
    s1 = list(t1.last_attn_seeds)
    assert t1.opt_step == 2 and len(set(s0 + s1)) == 2 * n_calls, "distinct within a step and between two steps"
    assert s1 == [attn_call_seed(3, 1, i) for i in range(n_calls)]
    assert all(v == v and abs(v) < 1e6 for v in m.values())


# (Nq, Nk_rows, Nk), p, seed
GRAPH_CASES = [((24, 264, 258), 0.1, DR.SEEDS[0]), ((136, 72, 72), 0.5, DR.SEEDS[1])]


@pytest.mark.parametrize("shape,p,seed", GRAPH_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_graph_attention_both_routes(engine, shape, p, seed):
    """Graph.attention(dropout=(p, seed)) at D = 64 with flash_bwd on and off: the same forward bits; o inside fwd_bound; the flash
    route's dq / dk / dv inside bwd_bounds of the f64 backward on the kernel's own o and lse, the materialised route's inside
    gemm_route_bounds of the exact gradient -- both with the numpy mask of the same seed."""
    Nq, Nkr, Nk = shape
    q, k, v, d_o = DR.make_inputs(Nq, Nkr, Nk)
    keep = DR.keep_tensor(seed, p, DR.B, DR.HEADS, Nq, Nk)
    got = {}
    for flash in (True, False):
        g = Graph(engine)
        g.flash_bwd = flash
        qv, kv, vv = Var(q.cuda()), Var(k.cuda()), Var(v.cuda())
        out = g.attention(qv, 0, kv, 0, vv, DR.HEADS, Nk, dropout=(p, seed))
        o = out.t.clone()
        out.cell[0] = d_o.cuda()
        g.backward()
        got[flash] = dict(o=o.cpu(), dq=qv.grad.cpu(), dk=kv.grad[:, :Nk].cpu(), dv=vv.grad[:, :Nk].cpu())
    assert bits_equal(got[True]["o"], got[False]["o"])
    fref, fbound = DR.fwd_bound(q, k, v, DR.HEADS, Nk, 0.125, keep, p)
    R.assert_within(got[True]["o"], fref.o, fbound, "o")
    # the lse the flash route's backward was handed: the same kernel on the same q, k (it does not depend on V or on the mask)
    lse = torch.empty((DR.B, DR.HEADS, Nq), dtype=F32, device="cuda")
    vt = torch.zeros((DR.B, DR.HEADS * 64, (Nk + 63) // 64 * 64), dtype=F16, device="cuda")
    engine.attention(q.cuda(), k.cuda()[:, :Nk], vt, DR.HEADS, Nk=Nk, lse=lse, dropout=(p, seed))
    ref = DR.bwd_ref(q, k, v, d_o, DR.HEADS, Nk, 0.125, keep, p, o16=got[True]["o"], lse2=lse.cpu())
    DR.assert_all(got[True], ref, DR.bwd_bounds(ref), f"flash {shape}", ("dq", "dk", "dv"))
    exact = DR.bwd_ref(q, k, v, d_o, DR.HEADS, Nk, 0.125, keep, p)
    DR.assert_all(got[False], exact, DR.gemm_route_bounds(exact, 0.125, Nq, Nk), f"materialised {shape}", ("dq", "dk", "dv"))


def test_the_mask_reaches_the_loss(engine):
    """Mean loss over a fixed batch, every other dropout off and eps given: attn_dropout 0.5 differs from 0.0."""
    cfg, ccfg, sd, batch = _setup(2)
    loss = {}
    for pa in (0.0, 0.5):
        tr = _trainer(engine, cfg, ccfg, sd, seed=5, attn_dropout=pa, dropout=0.0, state_dropout=0.0)
        loss[pa] = float(tr.forward_backward(*batch)[0])
    print("loss at attn_dropout 0.0 / 0.5:", loss)
    assert loss[0.0] == loss[0.0] and loss[0.5] == loss[0.5] and loss[0.0] != loss[0.5]


def test_agent_config_key_reaches_the_trainer():
    """``GenimaACT.update`` hands the config key ``attn_dropout`` to its trainer (default 0.0; a trainer_kw of the same name overrides it):
    one update each from a RoboBase-shaped replay batch, finite metrics, one seed per attention call at 0.1 and none at 0.0."""
    import numpy as np

    from genima_amd.act import GenimaACT

    ccfg = configs.TINY_ACT_CLIP_TEXT
    base = dict(configs.TINY_ACT_POLICY, data_augmentation=False)
    B, S, Tq = 2, base["image_size"], base["num_queries"]
    g = torch.Generator().manual_seed(8)
    toks = np.zeros((B, 1, 77), dtype=np.int32)
    toks[:, 0, :5] = [ccfg["vocab_size"] - 2, 3, 4, 5, ccfg["vocab_size"] - 1]
    batch = {f"{c}_rgb": torch.randint(0, 256, (B, 1, 3, S, S), generator=g, dtype=torch.uint8).numpy() for c in ("left_shoulder", "right_shoulder", "front", "wrist")}
    batch.update(low_dim_state=torch.randn(B, 1, base["state_dim"], generator=g).numpy(), lang_tokens=toks,
                 action=torch.rand(B, Tq, base["action_dim"], generator=g).numpy())
    n_calls = 2 * base["enc_layers"] + 2 * base["dec_layers"]
    for cfg, kw, want in ((dict(base, attn_dropout=0.1), {}, 0.1), (base, {}, 0.0), (dict(base, attn_dropout=0.1), dict(attn_dropout=0.0), 0.0)):
        agent = GenimaACT(cfg, None, ccfg, None, device="cuda", seed=4)
        m = agent.update(iter([batch]), 0, **kw)
        assert agent._trainer.p_attn == want and len(agent._trainer.last_attn_seeds) == (n_calls if want > 0 else 0)
        assert all(v == v for v in m.values())
