"""-m gpu: gn_attention_bwd (csrc/attention_bwd.hip: delta, dQ, dK / dV) and the lse of the attention forward kernels against the f64
references of tests/attention_ref.py, PER ELEMENT, at the bounds derived there:
  (a) the backward alone, handed the f64 forward's o / lse (rounded to f16 / f32), over the shapes and input families of bwd_cases();
  (b) layout: the trainer's fused q | k buffer, padded and mutually different strides, Nk_rows past round_up(Nk, 128), reruns, permutations;
  (c) the forward kernels' lse per element (variants 0 / 4 / 5, row-major V, the optimistic softmax's fallback, 77 keys);
  (d) each forward variant feeding the backward, against the reference evaluated on THAT forward's o and lse -- and what the forward's
      lse error does to the gradients;
  (e) every argument refusal of gn_attention_bwd.
Largest err / bound measured on MI355X (printed with -s): (a) delta 0.05, dq 0.85, dk 0.85, dv 0.87 (the q x 4 family; the CPU restatement of
the same arithmetic reaches 0.85 / 0.85 / 0.87); (c) lse 0.93, after the fallback 0.93 -- nearly all of it the evaluated rounding of c q to
f16; (d) dq 0.61, dk 0.46, dv 0.51.  The module (81 tests) takes 7 s."""
import ctypes as C

import pytest
import torch

import attention_ref as R
from act_ops_ref import bits_equal
from genima_amd import train_ops as T
from genima_amd._lib import AttnBwdDesc, GenimaHipError, check

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SCALE = R.D ** -0.5
SENTINEL = 0x7BCD  # a finite f16 bit pattern (6.4e4) no gradient of these tests takes


def dev(t):
    return t.cuda()


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def sent16(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(F16)


def is_sentinel(t) -> bool:
    return bool((t.contiguous().view(torch.int16) == SENTINEL).all())


def raw_bwd(engine, q, k, v, o, d_o, lse, delta, dq, dk, dv, heads, Nk, over=None):
    """gn_attention_bwd on [B, rows, ld] VIEWS (any row / batch stride, any column offset) -> rc; ``over`` overrides descriptor fields."""
    d = AttnBwdDesc()
    d.q, d.k, d.v, d.o, d.d_o = (t.data_ptr() for t in (q, k, v, o, d_o))
    d.lse, d.delta = lse.data_ptr(), delta.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.q_bs, d.k_bs, d.v_bs, d.o_bs, d.do_bs, d.dq_bs, d.dk_bs, d.dv_bs = (t.stride(0) for t in (q, k, v, o, d_o, dq, dk, dv))
    d.q_rs, d.k_rs, d.v_rs, d.o_rs, d.do_rs, d.dq_rs, d.dk_rs, d.dv_rs = (t.stride(1) for t in (q, k, v, o, d_o, dq, dk, dv))
    d.B, d.heads, d.Nq, d.Nk, d.Nk_rows, d.D, d.scale = q.shape[0], heads, q.shape[1], Nk, k.shape[1], R.D, SCALE
    for name, val in (over or {}).items():
        setattr(d, name, val)
    return engine.lib.gn_attention_bwd(engine._ctx, C.byref(d))


def run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk):
    """train_ops.attention_bwd on NaN-filled outputs, and the raw entry point once more for the delta scratch (train_ops keeps that to
    itself) -- whose dq / dk / dv must be the same bits.  -> dict of CPU tensors, dk / dv cut to the Nk live rows, plus the full ones."""
    B, Nq, Cc = q.shape
    qd, kd, vd, gd, od, ld = (dev(t) for t in (q, k, v, d_o, o16, lse32))
    dq, dk, dv = nan16(*q.shape), nan16(*k.shape), nan16(*v.shape)
    T.attention_bwd(engine, qd, 0, kd, 0, vd, od, gd, ld, heads, Nk, dq, dk, dv)
    delta = torch.full((B, heads, Nq), float("nan"), dtype=F32, device="cuda")
    dq2, dk2, dv2 = nan16(*q.shape), nan16(*k.shape), nan16(*v.shape)
    check(raw_bwd(engine, qd, kd, vd, od, gd, ld, delta, dq2, dk2, dv2, heads, Nk), "gn_attention_bwd")
    assert bits_equal(dq, dq2) and bits_equal(dk, dk2) and bits_equal(dv, dv2), "a second call is bit-identical"
    return dict(dq=dq.cpu(), dk=dk[:, :Nk].cpu(), dv=dv[:, :Nk].cpu(), delta=delta.cpu(), dk_full=dk.cpu(), dv_full=dv.cpu())


# ---- (a) the backward alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.bwd_cases(), ids=R.case_id)
def test_backward_alone(engine, case):
    """delta, dQ, dK, dV per element, o / lse from the f64 forward (never from the forward kernel); rows [Nk, Nk_rows) of dK / dV zero."""
    (B, heads, Nq, Nk, Nkr), family = case
    q, k, v, d_o, o16, lse32, ref = R.bwd_fixture(case)
    got = run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk)
    R.assert_bwd(got, ref, R.case_id(case))
    if Nkr > Nk:
        assert not bool(got["dk_full"][:, Nk:].view(torch.int16).any()) and not bool(got["dv_full"][:, Nk:].view(torch.int16).any()), "padding rows: +0"
    if family == "dozero":
        for n in ("dq", "dk", "dv"):
            assert float(got[n].abs().max()) == 0.0, f"{n}: dO = 0 gives exact zeros"
        assert float(got["delta"].abs().max()) == 0.0


# ---- (b) layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [R.BWD_SHAPES[4], R.BWD_SHAPES[8]], ids=lambda s: "x".join(map(str, s)))
def test_fused_qk_buffer(engine, shape):
    """The trainer's layout: q | k column slices of one buffer, dq | dk written into one buffer at the same offsets -- the bits of the
    separate-buffer call, inside the bounds."""
    B, heads, Nq, Nk, Nkr = shape
    Cc = heads * R.D
    q, k, v, d_o, o16, lse32, ref = R.bwd_fixture((shape, "gauss"))
    plain = run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk)
    qk = dev(torch.cat([q, k], -1))
    dqk, dv = nan16(B, Nq, 2 * Cc), nan16(B, Nkr, Cc)
    T.attention_bwd(engine, qk, 0, qk, Cc, dev(v), dev(o16), dev(d_o), dev(lse32), heads, Nk, dqk, dqk, dv)
    got = dict(dq=dqk[:, :, :Cc].cpu(), dk=dqk[:, :Nk, Cc:].cpu(), dv=dv[:, :Nk].cpu())
    R.assert_bwd(got, ref, "fused q|k", names=("dq", "dk", "dv"))
    for n in ("dq", "dk", "dv"):
        assert bits_equal(got[n], plain[n]), n


def _padded(t, ld, fill, rows_before=1, rows_after=1):
    """-> (buffer [B, rows_before + rows + rows_after, ld] filled with ``fill``, its [B, rows, C] view holding t)."""
    B, rows, Cc = t.shape
    buf = torch.full((B, rows_before + rows + rows_after, ld), fill, dtype=t.dtype, device="cuda")
    view = buf[:, rows_before:rows_before + rows, :Cc]
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("shape", [R.BWD_SHAPES[5], R.BWD_SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_padded_strides(engine, shape):
    """Five different input row strides (leading dimensions padded by 8, 16, ..; NaN in every pad column and in a pad row before and after
    each batch element), output row strides that are multiples of 4 but not of 8: the bits of the contiguous call, and every pad column
    and every row outside [0, Nq) / [0, Nk_rows) of the output buffers keeps its sentinel."""
    B, heads, Nq, Nk, Nkr = shape
    Cc = heads * R.D
    q, k, v, d_o, o16, lse32, ref = R.bwd_fixture((shape, "gauss"))
    plain = run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk)
    nan = float("nan")
    (_, qv), (_, ov), (_, gv), (_, vv), (_, kv) = (_padded(dev(t), Cc + pad, nan) for t, pad in ((q, 8), (o16, 8 + 8), (d_o, 24), (v, 32), (k, 40)))
    assert len({t.stride(1) for t in (ov, gv, vv)}) == 3
    outs = [torch.full((B, rows + 2, Cc + pad), SENTINEL, dtype=torch.int16, device="cuda").view(F16) for rows, pad in ((Nq, 4), (Nkr, 12), (Nkr, 20))]
    (dqv, dkv, dvv) = (buf[:, 1:-1, :Cc] for buf in outs)
    assert all(t.stride(1) % 4 == 0 and t.stride(1) % 8 for t in (dqv, dkv, dvv))
    delta = torch.full((B, heads, Nq), nan, dtype=F32, device="cuda")
    check(raw_bwd(engine, qv, kv, vv, ov, gv, dev(lse32), delta, dqv, dkv, dvv, heads, Nk), "gn_attention_bwd")
    assert bits_equal(dqv, plain["dq"]) and bits_equal(dkv, plain["dk_full"]) and bits_equal(dvv, plain["dv_full"])
    assert bits_equal(delta, plain["delta"])
    for buf in outs:
        assert is_sentinel(buf[:, 0]) and is_sentinel(buf[:, -1]) and is_sentinel(buf[:, :, Cc:]), "a pad row or column was written"


def test_nk_rows_past_the_round_up(engine):
    """(1, 2, 64, 8, 136): rows 8 .. 127 of dk / dv are written as zeros, rows 128 .. 135 are left untouched (include/genima_hip.h)."""
    shape = (1, 2, 64, 8, 136)
    B, heads, Nq, Nk, Nkr = shape
    q, k, v, d_o, o16, lse32, ref = R.bwd_fixture((shape, "gauss"))
    dq, dk, dv = nan16(*q.shape), sent16(*k.shape), sent16(*v.shape)
    T.attention_bwd(engine, dev(q), 0, dev(k), 0, dev(v), dev(o16), dev(d_o), dev(lse32), heads, Nk, dq, dk, dv)
    R.assert_bwd(dict(dq=dq, dk=dk[:, :Nk], dv=dv[:, :Nk]), ref, "Nk_rows 136", names=("dq", "dk", "dv"))
    for t in (dk, dv):
        assert not bool(t[:, Nk:128].contiguous().view(torch.int16).any()), "rows [Nk, round_up(Nk, 128)): zeros"
        assert is_sentinel(t[:, 128:]), "rows past round_up(Nk, 128) are left untouched"


def test_permutations_are_bit_exact(engine):
    """Permuting the batch, or the heads together with their columns, permutes dq / dk / dv / delta bit for bit (8 blocks: the XCD remap is
    taken; which block computes what must not show)."""
    shape = R.BWD_SHAPES[8]
    B, heads, Nq, Nk, Nkr = shape
    q, k, v, d_o, o16, lse32, ref = R.bwd_fixture((shape, "gauss"))
    base = run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk)
    pb = torch.tensor([1, 0])
    got = run_bwd(engine, q[pb], k[pb], v[pb], d_o[pb], o16[pb], lse32[pb], heads, Nk)
    for n in ("dq", "dk", "dv", "delta"):
        assert bits_equal(got[n], base[n][pb]), f"batch permutation: {n}"
    ph = torch.tensor([2, 0, 3, 1])
    cols = (ph[:, None] * R.D + torch.arange(R.D)[None, :]).flatten()
    got = run_bwd(engine, q[..., cols], k[..., cols], v[..., cols], d_o[..., cols], o16[..., cols], lse32[:, ph].contiguous(), heads, Nk)
    for n in ("dq", "dk", "dv"):
        assert bits_equal(got[n], base[n][..., cols]), f"head permutation: {n}"
    assert bits_equal(got["delta"], base["delta"][:, ph])


# ---- (c) the forward kernels' lse, per element --------------------------------------------------------------------------------------------
@pytest.fixture
def attn_variant(engine):
    """gn_attention_set_variant for the duration of a test (0 attention.hip, 4 attention_stream.hip, 5 attention_pwg.hip; -1 the library's choice)."""
    yield engine.lib.gn_attention_set_variant
    engine.lib.gn_attention_set_variant(-1)


def forward(engine, q, k, v, heads, Nk, rowmajor=False):
    """Engine.attention with an lse output -> (o, lse) on the device; V^T padded to 64 columns with NaN (never trusted)."""
    B, Nq, Cc = q.shape
    lse = torch.full((B, heads, Nq), float("nan"), dtype=F32, device="cuda")
    if rowmajor:
        vin = dev(v)
    else:
        vin = nan16(B, Cc, (Nk + 63) // 64 * 64)
        vin[:, :, :Nk] = dev(v)[:, :Nk].transpose(1, 2)
    o = engine.attention(dev(q), dev(k)[:, :Nk], vin, heads, Nk=Nk, lse=lse, v_rowmajor=rowmajor).clone()
    return o, lse


# variant (None: row-major V, attention.hip's VROW form), (B, heads, Nq, Nk): the smallest key count each accepts (one row block), and a
# size whose last row block is masked (200 = 128 + 72 rows; 320 = 2 x 128 + 64 = 256 + 64)
LSE_CASES = [(0, (1, 2, 8, 8)), (0, (2, 3, 200, 77)), (0, (1, 2, 200, 136)), (None, (1, 2, 8, 8)), (None, (2, 3, 200, 77)),
             (4, (1, 2, 128, 128)), (4, (1, 2, 320, 320)), (5, (1, 2, 128, 128)), (5, (1, 2, 320, 320))]


@pytest.mark.parametrize("variant,shape", LSE_CASES, ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("family", ["gauss", "sharp"])
def test_forward_lse(engine, attn_variant, variant, shape, family):
    """lse (log2 units) of each forward kernel within attention_ref.lse2_bound of the f64 value, every element."""
    B, heads, Nq, Nk = shape
    q, k, v, _ = R.make_inputs((B, heads, Nq, Nk, (Nk + 7) // 8 * 8), family, seed=2)
    attn_variant(0 if variant is None else variant)
    o, lse = forward(engine, q, k, v, heads, Nk, rowmajor=variant is None)
    R.assert_lse2(lse, q, k, heads, Nk, SCALE, p_sum_f16=R.P_SUM_F16[variant or 0], what=f"lse variant {variant} {shape} {family}")


def fallback_inputs(where, N=128):
    """The constructions of test_kernels_gpu.py::test_attention_stream_kernel_fallback at 128 keys (two key tiles, the fewest the stream
    and pwg kernels take): scores that beat the reference tile's by far more than the 2^13 a lane sum may reach."""
    B, heads = 1, 3
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(B, N, heads * R.D, generator=g) for _ in range(3))
    d = torch.randn(R.D, generator=g)
    d = d / d.norm()
    if where == "far_tile":      # a key of tile 1 aligned with every query of head 0: ~ +40 nats for the rows whose reference is tile 0
        q[:, :, :R.D] += 6.0 * d
        k[:, 100, :R.D] = 50.0 * d
    elif where == "one_row":     # one query row of tile 1 with one huge key in tile 0
        k[0, 37, R.D:2 * R.D] = 12.0 * q[0, 100, R.D:2 * R.D]
    else:                        # the maximum keeps growing along the keys for all rows of head 2
        q[:, :, 2 * R.D:] = 0.3 * q[:, :, 2 * R.D:] + 8.0 * d
        k[:, :, 2 * R.D:] = 0.3 * k[:, :, 2 * R.D:] + torch.linspace(-4.0, 4.0, N)[None, :, None] * d * 3.0
    return tuple(t.to(F16) for t in (q, k, v))


@pytest.mark.parametrize("where", ["far_tile", "one_row", "every_tile"])
@pytest.mark.parametrize("variant", [4, 5])
def test_forward_lse_after_the_fallback(engine, attn_variant, variant, where):
    """The same bound after the optimistic softmax's fallback (it is the same arithmetic with the maximum tracked): the 2e-2 the suite
    allowed here was 1.4 % of every probability the backward recomputes for the row."""
    q, k, v = fallback_inputs(where)
    attn_variant(variant)
    o, lse = forward(engine, q, k, v, 3, 128)
    R.assert_lse2(lse, q, k, 3, 128, SCALE, p_sum_f16=R.P_SUM_F16[variant], what=f"lse after the fallback, variant {variant} {where}")


# ---- (d) the pair ---------------------------------------------------------------------------------------------------------------------
# 136 x 136 and 200 x 77 run attention.hip whatever the variant says (attention_stream.hip / attention_pwg.hip take key counts that are
# multiples of 64 from 128 up): they get 128 x 128
PAIR_CASES = [(0, (1, 2, 136, 136, 136)), (None, (1, 2, 136, 136, 136)), (0, (2, 3, 200, 77, 80)), (None, (2, 3, 200, 77, 80)),
              (4, (1, 2, 128, 128, 128)), (5, (1, 2, 128, 128, 128))]


@pytest.mark.parametrize("variant,shape", PAIR_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_forward_feeds_backward(engine, attn_variant, variant, shape):
    """Each forward variant's own o and lse into the backward, against attn_bwd_ref evaluated ON THAT o and lse at the bounds of (a): a
    failure here with (c) passing is the backward's, a failure of (c) is the forward's.
    And what the forward's lse error e_q (within lse2_bound b_q of the true value: the rounding of c q to f16 and the f16 row sum) does to
    the gradients, derived: every probability of row q is scaled by 2^-e_q, so dQ's row q is scaled by exactly that, and an element of
    dK / dV moves by at most (2^max_q b_q - 1) of its sum of magnitudes."""
    B, heads, Nq, Nk, Nkr = shape
    q, k, v, d_o = R.make_inputs(shape, "gauss", seed=4)
    attn_variant(0 if variant is None else variant)
    o, lse = forward(engine, q, k, v, heads, Nk, rowmajor=variant is None)
    attn_variant(-1)
    o16, lse32 = o.cpu(), lse.cpu()
    got = run_bwd(engine, q, k, v, d_o, o16, lse32, heads, Nk)
    ref = R.attn_bwd_ref(q, k, v, d_o, o16, lse32, heads, Nk, SCALE)
    R.assert_bwd(got, ref, f"pair variant {variant} {shape}")
    lse_true, b = R.lse2_bound(q, k, heads, Nk, SCALE, p_sum_f16=R.P_SUM_F16[variant or 0])
    ref_true = R.attn_bwd_ref(q, k, v, d_o, o16, lse_true, heads, Nk, SCALE)
    w_row = (torch.exp2(b) - 1)[..., None].expand(B, heads, Nq, R.D).permute(0, 2, 1, 3).reshape(B, Nq, heads * R.D)
    w_head = (torch.exp2(b.amax(-1)) - 1)[:, None, :, None].expand(B, Nk, heads, R.D).reshape(B, Nk, heads * R.D)
    R.assert_within(ref.dq, ref_true.dq, w_row * ref_true.dq.abs() * (1 + 1e-9) + 1e-300, "dq moved by the lse error")
    R.assert_within(ref.dk, ref_true.dk, w_head * ref_true.dk_ab, "dk moved by the lse error")
    R.assert_within(ref.dv, ref_true.dv, w_head * ref_true.dv_ab, "dv moved by the lse error")
    print(f"lse error max {float((lse32.to(F64) - lse_true).abs().max()):.3e} (bound max {float(b.max()):.3e}): gradients move by at most "
          f"{float(w_head.max()):.3e} of their magnitude sums")


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------
def _off(t, elems):
    """The same storage, ``elems`` elements further on (a misaligned pointer; the buffers have a spare row)."""
    return t.flatten()[elems:elems + t[:, :-1].numel()].view(t.shape[0], t.shape[1] - 1, t.shape[2])


REFUSALS = {
    "D = 32": dict(D=32),
    "Nq % 8": dict(Nq=12),
    "Nk_rows < Nk": dict(Nk=16, Nk_rows=8),
    "Nk_rows % 8": dict(Nk=8, Nk_rows=12),
    "input row stride % 8": dict(q_rs=2 * 64 + 4),
    "input batch stride % 8": dict(v_bs=17 * 2 * 64 + 4),
    "output row stride % 4": dict(dq_rs=2 * 64 + 2),
    "output batch stride % 4": dict(dv_bs=17 * 2 * 64 + 2),
    "scale = 0": dict(scale=0.0),
    "scale < 0": dict(scale=-0.125),
    "null lse": dict(lse=None),
    "null delta": dict(delta=None),
    "misaligned input": "k",
    "misaligned output": "dk",
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(engine, what):
    """Every argument check of gn_attention_bwd raises through ``check`` before anything is launched: the NaN-filled outputs (and the
    delta scratch) keep their bits."""
    B, heads, N = 1, 2, 16
    Cc = heads * R.D
    g = torch.Generator().manual_seed(11)
    q, k, v, o, d_o = (torch.randn(B, N + 1, Cc, generator=g).to(F16).cuda() for _ in range(5))
    lse = torch.zeros(B, heads, N, dtype=F32, device="cuda")
    delta = torch.full((B, heads, N), float("nan"), dtype=F32, device="cuda")
    dq, dk, dv = nan16(B, N + 1, Cc), nan16(B, N + 1, Cc), nan16(B, N + 1, Cc)
    before = [t.clone() for t in (dq, dk, dv, delta)]
    t = dict(q=q[:, :N], k=k[:, :N], v=v[:, :N], o=o[:, :N], d_o=d_o[:, :N], dq=dq[:, :N], dk=dk[:, :N], dv=dv[:, :N])
    over = REFUSALS[what]
    if isinstance(over, str):  # 4 bytes past an aligned address: neither 16- nor 8-byte aligned
        t[over] = _off({**t, "k": k, "dk": dk}[over], 2)
        over = {}
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_attention_bwd"):
        check(raw_bwd(engine, t["q"], t["k"], t["v"], t["o"], t["d_o"], lse, delta, t["dq"], t["dk"], t["dv"], heads, N, over), "gn_attention_bwd")
    engine.synchronize()
    for a, b in zip((dq, dk, dv, delta), before):
        assert bits_equal(a, b), f"{what}: an output was written"
