"""-m gpu: the output O of every attention forward kernel -- attention.hip (D = 64 with V^T and with row-major V, D = 32, the block-shape
variants 1 and 2), attention_stream.hip, attention_pwg.hip (256-row and split blocks) -- against the f64 references of tests/attention_ref.py,
PER ELEMENT, at the bound derived there from the kernels' code (fwd_o_bound: B1 around the f64 attention of the rounded q' the kernels hold,
B1 + |O1 - O(q)| around the function's value), and the same rows' lse at lse2_bound.  Cases, families and fallback constructions are
attention_ref's (shared with tests/test_attention_fwd_ref_cpu.py, where the CPU restatement of the kernels' arithmetic meets the same bound).

The kernels are called through the C ABI (gn_attention_fwd on an AttnDesc), so that strides and untouched memory are under test: q and k are
column slices of one wider projection buffer whose other elements are NaN, o is a column slice of a wider buffer pre-filled with a finite
sentinel (rows >= Nq and the columns outside heads * D must keep it), V^T's pad columns and row-major V's pad columns are NaN, lse is
pre-filled with NaN.  On the same runs: a second call is bit-identical; for attention.hip and attention_stream.hip each (batch, head) run
alone (B = 1, heads = 1, same strides) gives the bits it has inside the batch; attention_pwg.hip, where the grid decides which blocks split,
gets the batch-permutation check instead.
Largest err / bound per kernel and block kind measured on MI355X (printed with -s): docs/HISTORY.md."""
import ctypes as C

import pytest
import torch

import attention_ref as R
from act_ops_ref import bits_equal
from genima_amd._lib import AttnDesc, check

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SENTINEL = 0x7BCD  # a finite f16 bit pattern (64 416) no result of these tests takes
PAD = 8            # extra columns of every buffer: the row strides are not the row lengths


@pytest.fixture
def attn_variant(engine):
    """gn_attention_set_variant for the duration of a test (-1: the library's choice)."""
    yield engine.lib.gn_attention_set_variant
    engine.lib.gn_attention_set_variant(-1)


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def sent16(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda").view(F16)


class Problem:
    """The device buffers of one attention problem (see the module docstring) and the descriptor over them."""

    def __init__(self, q, k, v, heads: int, d: int, causal: bool, vrow: bool):
        self.B, self.Nq, self.C = q.shape
        self.Nk, self.heads, self.d, self.causal, self.vrow = k.shape[1], heads, d, causal, vrow
        B, Nq, Nk, Cc = self.B, self.Nq, self.Nk, self.C
        self.proj = nan16(B, max(Nq, Nk), 2 * Cc + PAD)
        self.q, self.k = self.proj[:, :Nq, :Cc], self.proj[:, :Nk, Cc:2 * Cc]
        self.q.copy_(q)
        self.k.copy_(k)
        if vrow:
            self.vbuf = nan16(B, Nk, Cc + PAD)
            self.vbuf[:, :, :Cc] = v.cuda()
        else:
            self.vbuf = nan16(B, Cc, (Nk + 63) // 64 * 64 + PAD)
            self.vbuf[:, :, :Nk] = v.cuda().transpose(1, 2)

    def out(self):
        """-> (o buffer [B, Nq + 3, C + 2 PAD] of sentinels, lse [B, heads, Nq] of NaN)"""
        return sent16(self.B, self.Nq + 3, self.C + 2 * PAD), torch.full((self.B, self.heads, self.Nq), float("nan"), dtype=F32, device="cuda")

    def o_of(self, obuf):
        return obuf[:, :self.Nq, PAD:PAD + self.C]

    def run(self, engine, obuf, lse, only=None):
        """gn_attention_fwd into (obuf, lse); only = (b, h): that (batch, head) alone -- B = 1, heads = 1, the same strides, every pointer
        moved to its slice."""
        b, h = only if only is not None else (0, 0)
        o = self.o_of(obuf)
        desc = AttnDesc()
        desc.q_bs, desc.k_bs, desc.vt_bs, desc.o_bs = self.q.stride(0), self.k.stride(0), self.vbuf.stride(0), o.stride(0)
        desc.q_rs, desc.k_rs, desc.vt_rs, desc.o_rs = self.q.stride(1), self.k.stride(1), self.vbuf.stride(1), o.stride(1)
        v_head = h * self.d if self.vrow else h * self.d * desc.vt_rs
        desc.q = self.q.data_ptr() + 2 * (b * desc.q_bs + h * self.d)
        desc.k = self.k.data_ptr() + 2 * (b * desc.k_bs + h * self.d)
        desc.vt = self.vbuf.data_ptr() + 2 * (b * desc.vt_bs + v_head)
        desc.o = o.data_ptr() + 2 * (b * desc.o_bs + h * self.d)
        desc.lse = lse.data_ptr() + 4 * (b * self.heads + h) * self.Nq
        desc.B, desc.heads = (self.B, self.heads) if only is None else (1, 1)
        desc.Nq, desc.Nk, desc.D, desc.causal, desc.scale, desc.v_rowmajor = self.Nq, self.Nk, self.d, int(self.causal), float(self.d) ** -0.5, int(self.vrow)
        check(engine.lib.gn_attention_fwd(engine._ctx, C.byref(desc)), "gn_attention_fwd")
        engine.synchronize()

    def assert_untouched(self, obuf, what):
        """Everything of the o buffer outside [:, :Nq, PAD : PAD + C] still holds the sentinel."""
        t = obuf.clone()
        self.o_of(t).copy_(sent16(self.B, self.Nq, self.C))
        assert bool((t.view(torch.int16) == SENTINEL).all()), f"{what}: memory outside the output slice was written"


_measured: dict = {}  # (kernel, block kind) -> largest err / bound seen


def _note(kind: str, r: float):
    _measured[kind] = max(_measured.get(kind, 0.0), r)


def run_and_check(engine, attn_variant, kn, q, k, v, heads, causal, ref_key, kind, split=False):
    """One problem on one kernel: two identical calls, untouched memory, O per element (both assertions), lse per element.
    -> (problem, o buffer, lse) for the bit-level checks of the caller."""
    variant, d, vrow = R.FWD_KERNELS[kn]
    Nk = k.shape[1]
    psf = R.P_SUM_F16.get(variant, True)  # variants 1 / 2 are attention.hip's
    prob = Problem(q, k, v, heads, d, causal, vrow)
    attn_variant(variant)
    obuf, lse = prob.out()
    prob.run(engine, obuf, lse)
    obuf2, lse2 = prob.out()
    prob.run(engine, obuf2, lse2)
    assert bits_equal(obuf, obuf2) and bits_equal(lse, lse2), f"{ref_key}: a second call is bit-identical"
    prob.assert_untouched(obuf, ref_key)
    ref = R.fwd_ref_of(f"{ref_key}-{psf}-{split}", q, k, v, heads, Nk, d ** -0.5, p_sum_f16=psf, causal=causal, split=split)
    o = prob.o_of(obuf).cpu()
    try:
        _note(kind, R.assert_fwd_o(o, ref, f"{kn} {ref_key} o"))
    finally:  # the lse of the same rows is looked at even where O fails
        R.assert_lse2(lse, q, k, heads, Nk, d ** -0.5, p_sum_f16=psf, causal=causal, what=f"{kn} {ref_key} lse")
    return prob, obuf, lse, ref


def assert_alone_is_the_batch(engine, prob, obuf, lse, what):
    """Each (batch, head) run alone writes, into its slice of fresh buffers, the bits it has inside the batch -- and nothing else."""
    for b in range(prob.B):
        for h in range(prob.heads):
            ob, ls = prob.out()
            prob.run(engine, ob, ls, only=(b, h))
            cols = slice(PAD + h * prob.d, PAD + (h + 1) * prob.d)
            assert bits_equal(ob[b, :prob.Nq, cols], obuf[b, :prob.Nq, cols]) and bits_equal(ls[b, h], lse[b, h]), f"{what}: (b, h) = ({b}, {h}) alone"
            ob[b, :prob.Nq, cols] = sent16(prob.Nq, prob.d)
            assert bool((ob.view(torch.int16) == SENTINEL).all()) and bool(torch.isnan(ls).sum() == ls.numel() - prob.Nq), f"{what}: ({b}, {h}) alone wrote elsewhere"


def pwg_kind(B, heads, Nq, Nk):
    hs = R.pwg_split_heads(B, heads, Nq, Nk)
    return hs, "256-row" if hs == 0 else "split" if hs == heads else "mixed"


@pytest.mark.parametrize("case", R.fwd_cases(), ids=R.fwd_case_id)
def test_forward_per_element(engine, attn_variant, case):
    """Every case of attention_ref.fwd_cases(): see the module docstring."""
    kn, (B, heads, Nq, Nk), causal, family = case
    variant, d, vrow = R.FWD_KERNELS[kn]
    q, k, v = R.fwd_inputs(case)
    kind, split = kn, False
    if variant in (4, 5):
        assert not causal and Nk % 64 == 0 and Nk >= 128, "not a stream / pwg problem: gn_attention_fwd would run attention.hip instead"
    if variant == 5:  # gn_launch_attention_pwg's split rule, restated: the result is filed under the block kind that ran
        hs, name = pwg_kind(B, heads, Nq, Nk)
        want = [0] * len(R.FWD_PWG_FULL) + [s[1] for s in R.FWD_PWG_SPLIT] + [1, 0]
        assert hs == want[(R.FWD_PWG_FULL + R.FWD_PWG_SPLIT + R.FWD_PWG_MIXED).index((B, heads, Nq, Nk))]
        kind, split = f"pwg {name}", hs > 0
    ref_key = f"D{d}-" + R.fwd_case_id(case).split("-", 1)[1]
    prob, obuf, lse, ref = run_and_check(engine, attn_variant, kn, q, k, v, heads, causal, ref_key, kind, split)
    if variant == 5 and 0 < hs < heads:  # the two block kinds of a mixed grid apart
        err = R._heads((prob.o_of(obuf).cpu().to(F64) - ref.o1).abs() / ref.b1, heads)
        print(f"mixed grid: largest err/bound {float(err[:, :heads - hs].max()):.3f} in the 256-row blocks, {float(err[:, heads - hs:].max()):.3f} in the split blocks")
    if variant in (0, 4) and B * heads > 1:
        assert_alone_is_the_batch(engine, prob, obuf, lse, R.fwd_case_id(case))
    if variant == 5 and B > 1:  # which rows run in split blocks depends on the head, never on the batch position
        perm = torch.arange(B - 1, -1, -1)
        pp = Problem(q[perm], k[perm], v[perm], heads, d, causal, vrow)
        ob, ls = pp.out()
        pp.run(engine, ob, ls)
        assert bits_equal(ob, obuf[perm.cuda()]) and bits_equal(ls, lse[perm.cuda()]), "permuting the batch permutes the output bit for bit"


@pytest.mark.parametrize("fb", R.FWD_FALLBACKS, ids=lambda f: "-".join(str(x) for x in f))
def test_forward_fallback_per_element(engine, attn_variant, fb):
    """The redo of attention_stream.hip and attention_pwg.hip (split and 256-row blocks): rows that beat their diagonal-tile reference by
    more than 14 log2 units (asserted from the f64 scores: a probability above 2^14 > PLIM sets the block's flag) -- one key of the second
    key half against every query (far_tile), one key of the first half against one row (one_row), a maximum that grows along the keys
    (every_tile).  Same assertions as the plain cases."""
    kn, kind, where, Nq, Nk = fb
    q, k, v, (bs, h, rows) = R.fallback_inputs(where, Nq, Nk)
    ex = R.fallback_excess(q, k, 3, 0.125)[bs][:, h][:, rows]
    print(f"{where}: the intended rows exceed their reference by {float(ex.min()):.1f} .. {float(ex.max()):.1f} log2 units")
    assert float(ex.min()) > 14
    if kn == "pwg":
        assert pwg_kind(2, 3, Nq, Nk)[1] == {"split": "split", "256": "256-row"}[kind]
    prob, obuf, lse, _ = run_and_check(engine, attn_variant, kn, q, k, v, 3, False, f"fallback-{where}-{Nq}x{Nk}", f"{kn} {kind} redo", split=kind == "split")
    if kn == "stream":
        assert_alone_is_the_batch(engine, prob, obuf, lse, f"fallback {where}")


def test_measured_summary():
    """Prints the largest err / bound per kernel and block kind of this session's runs (docs/HISTORY.md records them; they are never fed back
    into a bound)."""
    for kind, r in sorted(_measured.items()):
        print(f"largest err/bound {kind}: {r:.3f}")
        assert r <= 1.0
