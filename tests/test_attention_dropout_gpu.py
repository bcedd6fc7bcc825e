"""-m gpu: attention-probability dropout inside the flash kernels (gn_attention_dropout_fwd / _bwd / _apply; csrc/attention.hip,
csrc/attention_bwd.hip) against the numpy mask and the f64 references of tests/attention_dropout_ref.py, PER ELEMENT, at the bounds derived
there.  heads = 2, B = 2, f16 inputs from a fixed generator; shapes (Nq, Nk_rows, Nk valid) of attention_dropout_ref.SHAPES, p in {0.1, 0.5},
seeds with high bits set.
  (1) the keep bytes of gn_attention_dropout_apply are the numpy mask, and its in-place form is f16(f32(x) * inv_keep) o keep, bit for bit;
  (2) forward o per element; (3) lse the bits of the plain kernel; (4) p = 0 through the new entry points gives the plain entry points'
  bits; (5) backward delta / dq / dk / dv per element on the dropout forward's own o and lse; (6) reruns and other seeds; (7) the padded
  rows of dk / dv; (8) dO = 0.
Each (shape, p, seed) runs the kernels once (``_run``); the tests share the result.
Largest err / bound measured on MI355X (printed with -s): see DESIGN.md section 3.8."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_dropout_ref as DR
import attention_ref as R
from act_ops_ref import bits_equal
from genima_amd._lib import AttnBwdDesc, AttnDesc, attn_dropout_desc, check

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SENTINEL = 0x7BCD  # a finite f16 bit pattern no result of these tests takes
B, HEADS = DR.B, DR.HEADS

# (shape, D, p, seed): every D = 64 shape at both p, the seeds taken in turn; D = 32 forward only
CASES = [(s, 64, p, DR.SEEDS[(i + j) % len(DR.SEEDS)]) for i, s in enumerate(DR.SHAPES) for j, p in enumerate(DR.PS)]
CASES_D32 = [(DR.SHAPE_D32, 32, p, DR.SEEDS[j]) for j, p in enumerate(DR.PS)]


def case_id(c):
    (Nq, Nkr, Nk), D, p, seed = c
    return f"{Nq}x{Nkr}x{Nk}-D{D}-p{p}-{seed:#x}"


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def sent16(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(F16)


def is_sentinel(t) -> bool:
    return bool((t.contiguous().view(torch.int16) == SENTINEL).all())


def raw_fwd(engine, q, k, v, Nk, D, drop):
    """gn_attention_dropout_fwd (drop = (p, seed)) or, with drop None, gn_attention_fwd forced to attention.hip's 4-wave x 32-row kernel
    (variant 0, restored afterwards) -> (o, lse) on the device.  V^T is padded to 64 columns with NaN (never trusted)."""
    Bq, Nq, Cc = q.shape
    qd, kd = q.cuda(), k.cuda()[:, :Nk]
    vt = nan16(Bq, Cc, (Nk + 63) // 64 * 64)
    vt[:, :, :Nk] = v.cuda()[:, :Nk].transpose(1, 2)
    o = nan16(Bq, Nq, Cc)
    lse = torch.full((Bq, HEADS, Nq), float("nan"), dtype=F32, device="cuda")
    d = AttnDesc()
    d.q, d.k, d.vt, d.o, d.lse = qd.data_ptr(), kd.data_ptr(), vt.data_ptr(), o.data_ptr(), lse.data_ptr()
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = qd.stride(0), kd.stride(0), vt.stride(0), o.stride(0)
    d.q_rs, d.k_rs, d.vt_rs, d.o_rs = qd.stride(1), kd.stride(1), vt.stride(1), o.stride(1)
    d.B, d.heads, d.Nq, d.Nk, d.D, d.causal, d.scale, d.v_rowmajor = Bq, HEADS, Nq, Nk, D, 0, float(D) ** -0.5, 0
    if drop is None:
        prev = engine.lib.gn_attention_set_variant(0)
        try:
            check(engine.lib.gn_attention_fwd(engine._ctx, C.byref(d)), "gn_attention_fwd")
        finally:
            engine.lib.gn_attention_set_variant(prev)
    else:
        dr = attn_dropout_desc(*drop)
        check(engine.lib.gn_attention_dropout_fwd(engine._ctx, C.byref(d), C.byref(dr)), "gn_attention_dropout_fwd")
    engine.synchronize()
    return o, lse


def raw_bwd(engine, q, k, v, o, d_o, lse, Nk, drop, dk=None, dv=None):
    """gn_attention_dropout_bwd (drop = (p, seed)) or gn_attention_bwd (drop None) on NaN-filled outputs (dk / dv may be given)
    -> dict of device tensors dq, dk, dv (all Nk_rows rows), delta."""
    qd, kd, vd, od, gd, ld = (t.cuda() for t in (q, k, v, o, d_o, lse))
    Bq, Nq, Cc = q.shape
    dq = nan16(*q.shape)
    dk = nan16(*k.shape) if dk is None else dk
    dv = nan16(*v.shape) if dv is None else dv
    delta = torch.full((Bq, HEADS, Nq), float("nan"), dtype=F32, device="cuda")
    d = AttnBwdDesc()
    d.q, d.k, d.v, d.o, d.d_o = (t.data_ptr() for t in (qd, kd, vd, od, gd))
    d.lse, d.delta = ld.data_ptr(), delta.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.q_bs, d.k_bs, d.v_bs, d.o_bs, d.do_bs, d.dq_bs, d.dk_bs, d.dv_bs = (t.stride(0) for t in (qd, kd, vd, od, gd, dq, dk, dv))
    d.q_rs, d.k_rs, d.v_rs, d.o_rs, d.do_rs, d.dq_rs, d.dk_rs, d.dv_rs = (t.stride(1) for t in (qd, kd, vd, od, gd, dq, dk, dv))
    d.B, d.heads, d.Nq, d.Nk, d.Nk_rows, d.D, d.scale = Bq, HEADS, Nq, Nk, k.shape[1], 64, 0.125
    if drop is None:
        check(engine.lib.gn_attention_bwd(engine._ctx, C.byref(d)), "gn_attention_bwd")
    else:
        dr = attn_dropout_desc(*drop)
        check(engine.lib.gn_attention_dropout_bwd(engine._ctx, C.byref(d), C.byref(dr)), "gn_attention_dropout_bwd")
    engine.synchronize()
    return dict(dq=dq, dk=dk, dv=dv, delta=delta)


_RUNS: dict = {}


def _run(engine, case):
    """Inputs, the kernels' outputs (forward; at D = 64 the backward on that forward's own o and lse) and the keep tensor of a case, once."""
    key = case_id(case)
    if key not in _RUNS:
        (Nq, Nkr, Nk), D, p, seed = case
        q, k, v, d_o = DR.make_inputs(Nq, Nkr, Nk, D)
        o, lse = raw_fwd(engine, q, k, v, Nk, D, (p, seed))
        r = dict(q=q, k=k, v=v, d_o=d_o, o=o.cpu(), lse=lse.cpu(), keep=DR.keep_tensor(seed, p, B, HEADS, Nq, Nk))
        if D == 64:
            r["bwd"] = {n: t.cpu() for n, t in raw_bwd(engine, q, k, v, r["o"], d_o, r["lse"], Nk, (p, seed)).items()}
        _RUNS[key] = r
    return _RUNS[key]


# ---- (1) the mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + CASES_D32, ids=case_id)
def test_keep_bytes_are_the_numpy_mask(engine, case):
    """gn_attention_dropout_apply with keep_out: bytes 0 / 1 equal to the numpy mask for i < Nq, j < Nk; the columns [Nk, Nk_rows) and the
    bytes behind the last row keep their sentinel.  In place: f16(f32(x) * inv_keep) where kept, +0 where dropped, pad columns untouched."""
    (Nq, Nkr, Nk), D, p, seed = case
    BH = B * HEADS
    dr = attn_dropout_desc(p, seed)
    buf = torch.full((BH * Nq * Nkr + Nkr,), 0xAB, dtype=torch.uint8, device="cuda")
    check(engine.lib.gn_attention_dropout_apply(engine._ctx, None, BH, Nq, Nk, Nkr, C.byref(dr), buf.data_ptr()), "gn_attention_dropout_apply")
    got = buf[:BH * Nq * Nkr].view(BH, Nq, Nkr).cpu().numpy()
    want = DR.keep_mask(seed, p, BH, Nq, Nk)
    assert np.array_equal(got[:, :, :Nk], want.astype(np.uint8)), f"{int((got[:, :, :Nk] != want).sum())} mask bytes differ"
    assert (got[:, :, Nk:] == 0xAB).all() and bool((buf[BH * Nq * Nkr:] == 0xAB).all()), "a byte outside the valid range was written"
    g = torch.Generator().manual_seed(5)
    x = torch.randn(BH, Nq, Nkr, generator=g).to(F16)
    xd = torch.cat([x.flatten(), torch.zeros(Nkr, dtype=F16)]).cuda()
    xd[BH * Nq * Nkr:] = sent16(Nkr)
    check(engine.lib.gn_attention_dropout_apply(engine._ctx, xd.data_ptr(), BH, Nq, Nk, Nkr, C.byref(dr), None), "gn_attention_dropout_apply")
    y = xd[:BH * Nq * Nkr].view(BH, Nq, Nkr).cpu()
    ref = torch.where(torch.from_numpy(want), (x[:, :, :Nk].to(F32) * torch.tensor(dr.inv_keep, dtype=F32)).to(F16), torch.zeros((), dtype=F16))
    assert bits_equal(y[:, :, :Nk], ref) and bits_equal(y[:, :, Nk:], x[:, :, Nk:]) and is_sentinel(xd[BH * Nq * Nkr:])


# ---- (2), (3) the forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + CASES_D32, ids=case_id)
def test_forward_o_per_element(engine, case):
    """o within attention_dropout_ref.fwd_bound of the f64 forward with the numpy mask, every element.  (One mismatched mask element moves
    an output by about |v| / Nk: far outside.)"""
    (Nq, Nkr, Nk), D, p, seed = case
    r = _run(engine, case)
    ref, bound = DR.fwd_bound(r["q"], r["k"], r["v"], HEADS, Nk, D ** -0.5, r["keep"], p)
    R.assert_within(r["o"], ref.o, bound, f"o {case_id(case)}")


@pytest.mark.parametrize("case", CASES + CASES_D32, ids=case_id)
def test_lse_is_the_plain_kernels(engine, case):
    """The row statistics are taken on the undropped P: lse has the bits gn_attention_fwd (variant 0) writes."""
    (Nq, Nkr, Nk), D, p, seed = case
    r = _run(engine, case)
    _, lse = raw_fwd(engine, r["q"], r["k"], r["v"], Nk, D, None)
    assert bits_equal(r["lse"], lse)


# ---- (4) p = 0 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,D", [(s, 64) for s in DR.SHAPES] + [(DR.SHAPE_D32, 32)], ids=str)
def test_p_zero_is_the_plain_entry_points(engine, shape, D):
    """threshold 0, inv_keep 1 through gn_attention_dropout_fwd / _bwd / _apply: o, lse, dq, dk, dv, delta bit-identical to the plain entry
    points (the plain forward forced to variant 0), and apply leaves x as it is."""
    Nq, Nkr, Nk = shape
    q, k, v, d_o = DR.make_inputs(Nq, Nkr, Nk, D)
    o0, lse0 = raw_fwd(engine, q, k, v, Nk, D, None)
    o1, lse1 = raw_fwd(engine, q, k, v, Nk, D, (0.0, DR.SEEDS[0]))
    assert bits_equal(o0, o1) and bits_equal(lse0, lse1)
    if D == 64:
        b0 = raw_bwd(engine, q, k, v, o0.cpu(), d_o, lse0.cpu(), Nk, None)
        b1 = raw_bwd(engine, q, k, v, o0.cpu(), d_o, lse0.cpu(), Nk, (0.0, DR.SEEDS[1]))
        for n in ("dq", "dk", "dv", "delta"):
            assert bits_equal(b0[n], b1[n]), n
    x = torch.randn(B * HEADS, Nq, Nkr, generator=torch.Generator().manual_seed(6)).to(F16)
    xd = x.cuda()
    dr = attn_dropout_desc(0.0, DR.SEEDS[2])
    check(engine.lib.gn_attention_dropout_apply(engine._ctx, xd.data_ptr(), B * HEADS, Nq, Nk, Nkr, C.byref(dr), None), "gn_attention_dropout_apply")
    assert bits_equal(xd, x)


# ---- (5) the backward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_per_element(engine, case):
    """delta, dQ, dK, dV within attention_dropout_ref.bwd_bounds of the f64 backward evaluated on the dropout forward's own o and lse."""
    (Nq, Nkr, Nk), D, p, seed = case
    r = _run(engine, case)
    ref = DR.bwd_ref(r["q"], r["k"], r["v"], r["d_o"], HEADS, Nk, 0.125, r["keep"], p, o16=r["o"], lse2=r["lse"])
    got = dict(r["bwd"], dk=r["bwd"]["dk"][:, :Nk], dv=r["bwd"]["dv"][:, :Nk])
    DR.assert_all(got, ref, DR.bwd_bounds(ref), case_id(case), ("delta", "dq", "dk", "dv"))
    if Nkr > Nk:  # (7) the padding rows of this 128-key block come out as +0
        for n in ("dk", "dv"):
            assert not bool(r["bwd"][n][:, Nk:].contiguous().view(torch.int16).any()), f"{n}: padding rows +0"


# ---- (6) reruns, other seeds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[2], CASES[5]], ids=case_id)
def test_same_seed_same_bits_other_seed_other_o(engine, case):
    (Nq, Nkr, Nk), D, p, seed = case
    r = _run(engine, case)
    o, lse = raw_fwd(engine, r["q"], r["k"], r["v"], Nk, D, (p, seed))
    assert bits_equal(o, r["o"]) and bits_equal(lse, r["lse"])
    again = raw_bwd(engine, r["q"], r["k"], r["v"], r["o"], r["d_o"], r["lse"], Nk, (p, seed))
    for n in ("dq", "dk", "dv", "delta"):
        assert bits_equal(again[n], r["bwd"][n]), n
    for other in (seed ^ 1, seed ^ (1 << 40)):  # one bit of the low word, one of the high word
        o2, lse2 = raw_fwd(engine, r["q"], r["k"], r["v"], Nk, D, (p, other))
        assert not bits_equal(o2, r["o"]) and bits_equal(lse2, r["lse"])


# ---- (7) rows >= Nk of dk / dv -----------------------------------------------------------------------------------------------------------
def test_padding_rows_past_the_round_up(engine):
    """(Nq 64, Nk_rows 136, Nk 8), as tests/test_attention_bwd_gpu.py states for the plain kernels: rows 8 .. 127 of dk / dv are written as
    zeros, rows 128 .. 135 are left untouched; the live rows sit inside the bounds."""
    Nq, Nkr, Nk, p, seed = 64, 136, 8, 0.1, DR.SEEDS[0]
    q, k, v, d_o = DR.make_inputs(Nq, Nkr, Nk)
    o, lse = raw_fwd(engine, q, k, v, Nk, 64, (p, seed))
    dk, dv = sent16(*k.shape), sent16(*v.shape)
    got = raw_bwd(engine, q, k, v, o.cpu(), d_o, lse.cpu(), Nk, (p, seed), dk=dk, dv=dv)
    keep = DR.keep_tensor(seed, p, B, HEADS, Nq, Nk)
    ref = DR.bwd_ref(q, k, v, d_o, HEADS, Nk, 0.125, keep, p, o16=o.cpu(), lse2=lse.cpu())
    DR.assert_all(dict(got, dk=dk[:, :Nk], dv=dv[:, :Nk]), ref, DR.bwd_bounds(ref), "Nk_rows 136", ("delta", "dq", "dk", "dv"))
    for t in (dk, dv):
        assert not bool(t[:, Nk:128].contiguous().view(torch.int16).any()), "rows [Nk, round_up(Nk, 128)): zeros"
        assert is_sentinel(t[:, 128:]), "rows past round_up(Nk, 128) are left untouched"


# ---- (8) dO = 0 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=case_id)
def test_zero_upstream_gradient_gives_exact_zeros(engine, case):
    (Nq, Nkr, Nk), D, p, seed = case
    r = _run(engine, case)
    got = raw_bwd(engine, r["q"], r["k"], r["v"], r["o"], torch.zeros_like(r["d_o"]), r["lse"], Nk, (p, seed))
    for n in ("dq", "dk", "dv", "delta"):
        assert float(got[n].abs().max()) == 0.0, f"{n}: dO = 0 gives exact zeros"
