"""-m gpu: the loss read-outs on the tiny family (the sizes of tests/test_sphere_loss_trainer_gpu.py): ``attach_frozen(loss_parts=)`` leaves the
step's bits alone and fills a table that equals tests/loss_parts_ref.py on the inputs the wrapper was handed; the summary, the loop hook;
``eval_loss`` repeats itself bit for bit, leaves the trainer's state alone and agrees with the CPU oracle's forward loss.

Bars.  Table against the reference: tests/test_loss_parts_kernels_gpu.py's derived bound (A, P, n exact).  ``eval_loss`` against the oracle:
the loss bar of tests/test_sphere_loss_trainer_gpu.py's autograd test, 2e-3 relative to the fp32 oracle."""
import functools
import json

import numpy as np
import pytest
import torch

from genima_amd import configs, schema, train_loop, weights
from genima_amd import train_ops as T
from genima_amd.engine import Engine
from genima_amd.packing import pack_state_dict
from genima_amd.scheduler import DDPMScheduler
from genima_amd.training import ControlNetTrainer
from oracle import sd_torch as O
import loss_parts_ref as P
import sphere_loss_ref as R

pytestmark = pytest.mark.gpu

FAM = configs.family("tiny")
SEED, RES, LAT, C, NTT = 5, 256, 32, 4, 1000
BAR = 4 * LAT * LAT * C * P.U  # sums of table entries against the reference's: the kernel test's bound at its ceiling, 4 N 2^-53


def _synth(sch, s):
    return weights.round_to(weights.synth_state_dict(sch, s), torch.float16)


@functools.lru_cache(maxsize=None)
def _state_dicts():
    return _synth(schema.unet_schema(FAM["unet"]), 1), _synth(schema.controlnet_schema(FAM["controlnet"]), 2)


@functools.lru_cache(maxsize=None)
def _grid(seed=11, B=2):
    target, cond = R.byte_grid_pair(B, RES, RES, seed=seed)
    share = R.marked_share(R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30))
    assert 0.01 <= share <= 0.5, share
    return target, cond


def _batch(seed=11, B=2):
    target, cond = _grid(seed, B)
    g = torch.Generator().manual_seed(9)
    return dict(pixel_values=torch.from_numpy(target), conditioning_pixel_values=torch.from_numpy(cond), input_ids=torch.randint(0, 1000, (B, 77), generator=g))


def _trainer(parts=0, weight=0.0, augmentations=None, **kw):
    usd, csd = _state_dicts()
    tr = ControlNetTrainer(Engine("cuda:0"), FAM["unet"], FAM["controlnet"], pack_state_dict(usd, "cuda"), csd, lr=1e-4, loss_scale=4096.0, **kw)
    tr.attach_frozen(FAM["vae"], pack_state_dict(_synth(schema.vae_schema(FAM["vae"]), 3), "cuda"), FAM["text"],
                     pack_state_dict(_synth(schema.clip_text_schema(FAM["text"]), 4), "cuda"), DDPMScheduler(), seed=SEED, augmentations=augmentations,
                     sphere_loss_weight=weight, loss_parts=parts)
    return tr


def _record(monkeypatch, tr):
    """Wrap the wrapper and the front: -> (calls: the host copies of what mse_loss_parts was handed, ts: the timesteps the front drew)."""
    calls, ts = [], []
    real, front = T.mse_loss_parts, tr._front

    def parts(E, pred, target, mask, bucket, table, C_valid):
        calls.append(dict(pred=pred.cpu().numpy(), target=target.cpu().numpy(), mask=None if mask is None else mask.cpu().numpy(),
                          bucket=bucket.cpu().numpy(), C=C_valid, mask_obj=mask))
        return real(E, pred, target, mask, bucket, table, C_valid)

    def fr(batch):
        out = front(batch)
        ts.append(out[2].clone())
        return out
    monkeypatch.setattr(T, "mse_loss_parts", parts)
    monkeypatch.setattr(tr, "_front", fr)
    return calls, ts


def _ref_table(calls, rows):
    ref = np.zeros((rows, 5))
    for c in calls:
        P.table_add(ref, c["pred"], c["target"], c["mask"], c["bucket"], c["C"])
    return ref


def _adds(calls, rows):
    return [sum(int((np.clip(c["bucket"], 0, rows - 1) == r).sum()) for c in calls) for r in range(rows)]


def test_off_calls_neither_entry_point(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the loss-parts ops must not run with loss_parts == 0")
    tr = _trainer(0)
    monkeypatch.setattr(T, "mse_loss_parts", boom)
    monkeypatch.setattr(tr.E.lib, "gn_mse_loss_parts", boom)
    monkeypatch.setattr(tr.E.lib, "gn_mse_loss_parts_workspace_bytes", boom)
    assert len(tr._front(_batch())) == 8  # the front's outputs as they were
    loss = float(tr.train_step(_batch()))
    assert loss == loss and tr.loss_parts == 0 and tr._parts_table is None
    with pytest.raises(ValueError):
        tr.loss_parts_summary()


def test_on_keeps_the_bits_and_fills_the_reference_table(monkeypatch):
    on, off = _trainer(4), _trainer(0)
    calls, ts = _record(monkeypatch, on)
    l_on = [float(on.train_step(_batch())) for _ in range(3)]
    l_off = [float(off.train_step(_batch())) for _ in range(3)]
    print(f"losses with loss_parts=4 {l_on}, without {l_off}")
    assert l_on == l_off and all(x == x for x in l_on)
    assert torch.equal(on.cn.master, off.cn.master) and torch.equal(on.cn.half, off.cn.half) and torch.equal(on.cn.exp_avg, off.cn.exp_avg)
    assert len(calls) == 3 and len(ts) == 3
    for c, t in zip(calls, ts):
        assert c["bucket"].tolist() == (t * 4 // NTT).tolist() and c["bucket"].dtype == np.int32
        assert c["mask"].shape == (2, RES, RES, 8) and c["pred"].shape == (2, LAT, LAT, 8) and c["C"] == C
        assert 0.01 <= R.marked_share(c["mask"]) <= 0.5
    got = on._parts_table.cpu().numpy()
    ref = _ref_table(calls, 5)
    assert got[:, 4].sum() == 6.0 and got[4, 4] == 0.0
    P.assert_table_close(got, ref, LAT, LAT, _adds(calls, 5))
    # the summary: one read, the table's own numbers, then zero
    s = on.loss_parts_summary(reset=True)
    tot = ref[:4].sum(axis=0)
    assert s["n"] == 6 and s["dropped"] == 0 and len(s["by_t"]) == 4
    assert [(r["t_lo"], r["t_hi"]) for r in s["by_t"]] == [(0, 249), (250, 499), (500, 749), (750, 999)]
    assert [r["n"] for r in s["by_t"]] == [int(v) for v in ref[:4, 4]]
    assert abs(s["loss"] - (tot[0] + tot[1]) / (C * tot[3])) <= BAR * s["loss"]
    assert abs(s["loss_sphere"] - tot[0] / (C * tot[2])) <= BAR * s["loss_sphere"] and s["sphere_area"] == tot[2] / tot[3]
    # the mean of the three step losses is the table's loss (each step's f32 loss within gn_mse_loss's bound of its own f64 value)
    assert abs(s["loss"] - float(np.mean(l_on))) <= (2 * LAT * LAT * C + 8) * 2.0 ** -24 * s["loss"]
    assert not bool(on._parts_table.any())
    z = on.loss_parts_summary()
    assert z["n"] == 0 and z["loss"] is None


def test_weighted_step_shares_the_mask_and_splits_the_unweighted_error(monkeypatch):
    augs = "affine,crop"
    tr, plain = _trainer(4, weight=4.0, augmentations=augs), _trainer(0, weight=4.0, augmentations=augs)
    calls, _ = _record(monkeypatch, tr)
    pooled, pool = [], T.loss_weight_pool

    def rec_pool(E, mask, *a, **k):
        pooled.append(mask)
        return pool(E, mask, *a, **k)
    monkeypatch.setattr(T, "loss_weight_pool", rec_pool)
    l_w = [float(tr.train_step(_batch())) for _ in range(2)]
    monkeypatch.setattr(T, "loss_weight_pool", pool)
    l_p = [float(plain.train_step(_batch())) for _ in range(2)]
    assert l_w == l_p and torch.equal(tr.cn.master, plain.cn.master)  # the weighted step's own bits, parts on or off
    assert len(pooled) == 2 and all(c["mask_obj"] is m for c, m in zip(calls, pooled))  # one mask, after the augmentations, for both consumers
    target, cond = _grid()
    before = R.change_mask(target, cond, 127.5, 127.5, 255.0, 0.0, 30)
    assert not np.array_equal(calls[0]["mask"], before) and 0.0 < R.marked_share(calls[0]["mask"]) < 1.0
    got = tr._parts_table.cpu().numpy()
    P.assert_table_close(got, _ref_table(calls, 5), LAT, LAT, _adds(calls, 5))
    # unweighted: the table's loss is the PLAIN mean of (pred - target)^2 on the handed tensors, which the weighted step's loss is not
    s = tr.loss_parts_summary()
    plain_mean = np.mean([P.total_sq_error(c["pred"], c["target"], C) / (2 * LAT * LAT * C) for c in calls])
    assert abs(s["loss"] - plain_mean) <= BAR * plain_mean
    assert abs(float(np.mean(l_w)) - plain_mean) > 1e-4 * plain_mean


def test_every_micro_batch_counts():
    tr = _trainer(4, gradient_accumulation_steps=2)
    synced = []
    for _ in range(2):
        tr.train_step(_batch())
        synced.append(tr.sync_gradients)
    assert synced == [False, True] and tr.opt_step == 1
    s = tr.loss_parts_summary(reset=False)
    assert s["n"] == 4 and sum(r["n"] for r in s["by_t"]) == 4
    assert tr.loss_parts_summary()["n"] == 4  # reset=False left it


def test_replayed_step_refuses_the_parts():
    usd, csd = _state_dicts()
    tr = ControlNetTrainer(Engine("cuda:0"), FAM["unet"], FAM["controlnet"], pack_state_dict(usd, "cuda"), csd, hip_graph=True)
    with pytest.raises(ValueError):
        tr.attach_frozen(None, None, None, None, DDPMScheduler(), loss_parts=4)
    with pytest.raises(ValueError):
        tr.step(*([None] * 7), loss_parts=(None, None))
    with pytest.raises(ValueError):
        tr.eval_loss(_batch(), [999])


def test_train_loop_logs_and_resets(tmp_path):
    tr = _trainer(4)
    lines = []
    loop = train_loop.TrainLoop(tr, str(tmp_path), max_train_steps=4, checkpointing_steps=1000, loss_parts_steps=2, log=lines.append)
    assert loop.run([_batch()] * 4) == 4
    recs = [json.loads(x) for x in lines]
    assert [r["step"] for r in recs] == [2, 4]
    for r in recs:  # two steps of two samples each: the table was reset between the lines
        assert r["n"] == 4 and r["dropped"] == 0 and r["loss"] > 0 and r["loss_sphere"] > 0 and r["loss_background"] > 0 and len(r["by_t"]) == 4
        assert 0.0 < r["sphere_area"] < 1.0
    assert tr.loss_parts_summary()["n"] == 0
    # loss_parts_steps on a trainer with the option off logs nothing
    lines2 = []
    train_loop.TrainLoop(_trainer(0), str(tmp_path), max_train_steps=2, checkpointing_steps=1000, loss_parts_steps=1, log=lines2.append).run([_batch()] * 2)
    assert lines2 == []


def _state(tr):
    cn = tr.cn
    return dict(master=cn.master.clone(), half=cn.half.clone(), grad=cn.grad.clone(), m=cn.exp_avg.clone(), v=cn.exp_avg_sq.clone(),
                wt={k: v.clone() for k, v in cn._wt.items()}, gen_dev=tr._gen_dev.get_state().clone(), gen_cpu=tr._gen_cpu.get_state().clone(),
                scalars=(tr.opt_step, tr.loss_scale, tr._clean, tr.sched_step, tr._micro, tr.sync_gradients), last=dict(tr.last))


def _assert_same_state(a, b, last=True):
    for k in ("master", "half", "grad", "m", "v", "gen_dev", "gen_cpu"):
        assert torch.equal(a[k], b[k]), k
    assert a["wt"].keys() == b["wt"].keys() and all(torch.equal(a["wt"][k], b["wt"][k]) for k in a["wt"])
    assert a["scalars"] == b["scalars"]
    assert not last or a["last"].keys() == b["last"].keys() and all(a["last"][k] is b["last"][k] or a["last"][k] == b["last"][k] for k in a["last"])


def test_eval_loss_repeats_itself_and_leaves_the_trainer_alone():
    ts = (999, 599, 199)
    a, b = _trainer(0, gradient_accumulation_steps=2), _trainer(0, gradient_accumulation_steps=2)
    held = _batch(seed=12)
    t0 = a.eval_loss(held, ts, seed=3)
    t1 = a.eval_loss(held, ts, seed=3)
    assert tuple(t0.shape) == (4, 5) and t0.dtype == torch.float64
    assert np.array_equal(t0.cpu().numpy().view(np.uint64), t1.cpu().numpy().view(np.uint64))
    got = t0.cpu().numpy()
    assert got[:3, 4].tolist() == [2.0] * 3 and got[3].tolist() == [0.0] * 5 and (got[:3, 0] > 0).all() and (got[:3, 1] > 0).all()
    assert not np.array_equal(a.eval_loss(held, ts, seed=4).cpu().numpy()[:, :2], got[:, :2])  # another seed, another noise
    la, lb = [], []
    for i in range(3):  # the gradient of an open accumulation (after steps 1 and 3) is in the flat buffer while eval_loss runs
        la.append(float(a.train_step(_batch())))
        lb.append(float(b.train_step(_batch())))
        before = _state(a)
        if i == 0:
            assert float(before["grad"].abs().max()) > 0.0
        a.eval_loss(held, ts, seed=3)
        _assert_same_state(before, _state(a))
    print(f"losses with eval_loss between the steps {la}, without {lb}")
    assert la == lb and all(x == x for x in la)
    _assert_same_state(_state(a), _state(b), last=False)  # (two trainers: their last predictions are two tensors)
    # ... and the weights moved, so the held-out loss did too
    assert a.opt_step == 1 and not np.array_equal(a.eval_loss(held, ts, seed=3).cpu().numpy()[:, :2], got[:, :2])


def test_eval_loss_against_the_oracle_forward(monkeypatch):
    usd, csd = _state_dicts()
    tr = _trainer(0)
    seen = {}
    lat_fn, text_fn = tr._front_latents, tr._front_text

    def rec_lat(*a, **k):
        out = lat_fn(*a, **k)
        seen.update(cond8=out[2], lat8=out[4], noise8=out[5])
        return out

    def rec_text(*a, **k):
        out = text_fn(*a, **k)
        seen.update(ctx=out[0])
        return out
    monkeypatch.setattr(tr, "_front_latents", rec_lat)
    monkeypatch.setattr(tr, "_front_text", rec_text)
    t = 599
    table = tr.eval_loss(_batch(seed=12), [t], seed=1).cpu().numpy()
    s = T.summarize_parts(table, C, [t])
    nchw = lambda x, c: x[..., :c].permute(0, 3, 1, 2).float().cpu().contiguous()  # noqa: E731
    lat, noise, cond, ctx = nchw(seen["lat8"], 4), nchw(seen["noise8"], 4), nchw(seen["cond8"], 3), seen["ctx"].float().cpu()
    tt = torch.tensor([t, t])
    sa, s1 = DDPMScheduler().add_noise_coeffs(tt)
    with torch.no_grad():
        noisy = sa.view(-1, 1, 1, 1) * lat + s1.view(-1, 1, 1, 1) * noise
        down, mid = O.controlnet_forward(csd, FAM["controlnet"], noisy, tt.float(), ctx, cond)
        pred = O.unet_forward(usd, FAM["unet"], noisy, tt.float(), ctx, down, mid)
        l32 = float(((pred.float() - noise) ** 2).mean())
    print(f"eval_loss at t = {t}: {s['loss']!r} (sphere {s['loss_sphere']!r}, background {s['loss_background']!r}), fp32 oracle {l32!r}")
    assert s["n"] == 2 and s["by_t"][0]["t"] == t and s["by_t"][0]["loss"] == s["loss"]
    assert abs(s["loss"] - l32) <= 2e-3 * l32


def test_loss_validator_sums_its_batches():
    tr = _trainer(0)
    b1, b2 = _batch(seed=12), _batch(seed=13)
    ts = (999, 199)
    lines = []
    validate = train_loop.loss_validator(tr, [b1, b2], timesteps=ts, seed=2, log=lines.append)
    line = validate(7)
    both = (tr.eval_loss(b1, ts, seed=2) + tr.eval_loss(b2, ts, seed=2)).cpu().numpy()
    want = dict(step=7, **T.summarize_parts(both, C, ts))
    assert json.loads(lines[0]) == line and line["select"] == line["loss"] and line.keys() == want.keys() | {"select"}

    def same(a, b):
        """Counts, names and Nones exactly.  Floats: an entry of the validator's table is ((a0 + a1) + b0) + b1 per row, the sum of the
        two tables (a0 + a1) + (b0 + b1) -- three roundings of non-negative terms each way, and a loss is a quotient of two such sums
        and their products with C (four more roundings a side): 2 * (2 * 3 + 4) = 20 u relative."""
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, list):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, float) and isinstance(b, float):
            return abs(a - b) <= 20 * P.U * abs(b)
        return type(a) is type(b) and a == b
    assert same({k: v for k, v in line.items() if k != "select"}, want), (line, want)
    assert line["n"] == 8 and [r["t"] for r in line["by_t"]] == [999, 199] and [r["n"] for r in line["by_t"]] == [4, 4]
    validate(9)
    assert [h["step"] for h in validate.history] == [7, 9] and validate.history[1]["loss"] == line["loss"]
