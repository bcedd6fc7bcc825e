"""The forward's O reference and bound of tests/attention_ref.py (fwd_o_bound), checked on the CPU: the f32 / f16 restatement of the kernels'
arithmetic (emulate_fwd_f32) is inside the bound on every element of every case tests/test_attention_fwd_gpu.py runs, for every reference
walk and both row-sum conventions; planted errors are outside it -- or inside, where the bound cannot see them, and said so -- and for each
plant it is recorded whether the whole-tensor bar the suite had before (test_kernels_gpu.attention_whole_tensor_bar) lets it through."""
import pytest
import torch

import attention_ref as R
from test_kernels_gpu import attention_whole_tensor_bar

F16, F32, F64 = torch.float16, torch.float32, torch.float64


def walks_of(Nk: int, causal: bool):
    """(walk, tile, split) the restatement is run with: attention.hip's walk and the max-tracking loop everywhere; where the stream and pwg
    kernels are eligible (whole unmasked tiles, >= 128 keys) the fixed diagonal reference in 64- and 32-key steps, and with an even tile
    count the two key halves merged."""
    w = [("first", 64, False), ("track", 32, False)]
    if Nk % 64 == 0 and Nk >= 128 and not causal:
        w += [("diag", 64, False), ("diag", 32, False)]
        if (Nk // 64) % 2 == 0:
            w.append(("diag", 32, True))
    return w


def ratio(o, ref) -> float:
    return float(((o.to(F64) - ref.o1).abs() / ref.b1).max())


def old_bar_passes(o, q, k, v, heads, causal=False, factor=1.35) -> bool:
    try:
        attention_whole_tensor_bar(o, q, k, v, heads, causal, factor=factor)
        return True
    except AssertionError:
        return False


# ---- the reference itself --------------------------------------------------------------------------------------------------------------
def test_centre_and_function_value():
    """o of fwd_o_bound is attn_fwd_ref's; o1 is the same attention evaluated on q' (exponent units: weights 2^(q'.k)); for q = 0 they
    coincide; the centred sum is what its formula says."""
    case = ("att64", (2, 3, 200, 77), False, "qzero")
    q, k, v = R.fwd_inputs(case)
    ref = R.fwd_o_bound(q, k, v, 3, 77, 0.125, p_sum_f16=True)
    assert float((ref.o - R.attn_fwd_ref(q, k, v, 3, 77, 0.125)[0]).abs().max()) < 1e-14
    q1 = R.q_prime(q, 0.125)
    o1 = R.attn_fwd_ref(q1, k, v, 3, 77, R.LN2)[0]  # softmax(ln 2 q'.k) = weights 2^(q'.k)
    assert float((ref.o1 - o1).abs().max()) < 1e-14
    assert float(ref.shift[:, 100].max()) < 1e-15 and float(ref.shift.max()) > 1e-5  # the zero query row has nothing to round
    P = torch.softmax(R._heads(q1, 3)[1, 2] @ R._heads(k, 3)[1, 2].t() * R.LN2, -1)
    vv, o1h = R._heads(v, 3)[1, 2], R._heads(ref.o1, 3)[1, 2]
    cn = (P[:, :, None] * (vv[None] - o1h[:, None]).abs()).sum(1)
    got = R._centred_sum(P, vv, o1h)
    assert bool((got >= cn).all()) and float((got / cn).max()) < 1 + 1e-4


def test_causal_rows_count_their_live_keys():
    """Under causal the bound of row i is the bound of the same row of the i + 1 key problem."""
    q, k, v = R.fwd_inputs(("att64", (1, 2, 77, 77), True, "gauss"))
    ref = R.fwd_o_bound(q, k, v, 2, 77, 0.125, p_sum_f16=True, causal=True)
    for i in (0, 40, 76):
        cut = R.fwd_o_bound(q[:, i:i + 1], k, v, 2, i + 1, 0.125, p_sum_f16=True)
        assert float((ref.o1[:, i] - cut.o1[:, 0]).abs().max()) < 1e-14
        assert float((ref.b1[:, i] / cut.b1[:, 0] - 1).abs().max()) < 1e-6  # (the centred sum is evaluated in f32)


# ---- the restatement against the bound ---------------------------------------------------------------------------------------------------
def problems():
    """The GPU module's cases without the kernel: (D, shape, causal, family), each once."""
    seen, out = set(), []
    for case in R.fwd_cases():
        kn, shape, causal, family = case
        key = (R.FWD_KERNELS[kn][1], shape, causal, family)
        if key not in seen:
            seen.add(key)
            out.append(case)
    return out


_worst: dict = {}


@pytest.mark.parametrize("case", problems(), ids=lambda c: R.fwd_case_id(c).split("-", 1)[1] + f"-D{R.FWD_KERNELS[c[0]][1]}")
def test_restatement_is_within_the_bound(case):
    """emulate_fwd_f32 is inside B1 on every element: l = sum p16 against the bound with the centred term, l = sum p32 against U alone
    (with the split block's two additions), every walk."""
    kn, (B, heads, Nq, Nk), causal, family = case
    d = R.FWD_KERNELS[kn][1]
    q, k, v = R.fwd_inputs(case)
    for psf in (True, False):
        ref = R.fwd_o_bound(q, k, v, heads, Nk, d ** -0.5, p_sum_f16=psf, causal=causal, split=not psf)
        for walk, tile, split in walks_of(Nk, causal):
            o = R.emulate_fwd_f32(q, k, v, heads, Nk, d ** -0.5, causal=causal, walk=walk, p_sum_f16=psf, tile=tile, split=split)
            r = R.assert_within(o, ref.o1, ref.b1, f"{R.fwd_case_id(case)} {walk}/{tile}{'/split' if split else ''} sum {'f16' if psf else 'f32'}")
            R.assert_within(o, ref.o, ref.b1 + ref.shift, "... vs O(q)")
            _worst[family] = max(_worst.get(family, 0.0), r)


def test_restatement_worst_per_family():
    """The largest err / bound per family (printed): measured 0.78 gauss (the first rows of a causal problem: few keys, the tightest window),
    0.52 sharp, 0.52 spike, 0.70 qzero / vpos, 0 vconst / voffset (the weights sum to one: o = f16(v) exactly)."""
    for f, r in sorted(_worst.items()):
        print(f"{f}: largest err/bound of the restatement {r:.3f}")
        assert r < 1.0


def test_bound_sizes():
    """What B1 allows, in f16 ulps of the element (median): a few ulps at 72 keys growing to ~20 at 1024 on zero-mean V (the P -> f16 term
    grows like o_ab / |O| ~ sqrt(n)); under 2 ulps on |v| and on a V constant along the keys, where the centred term takes over."""
    med = {}
    for family in ("gauss", "vpos", "voffset"):
        q, k, v = R.fwd_inputs(("att64", (1, 2, 136, 72), False, family))
        ref = R.fwd_o_bound(q, k, v, 2, 72, 0.125, p_sum_f16=True)
        med[family] = float((ref.b1 / R.ulp16(ref.o1)).median())
        print(f"{family}: median b1 {med[family]:.2f} f16 ulps, |O1 - O(q)| / b1 median {float((ref.shift / ref.b1).median()):.3f} max {float((ref.shift / ref.b1).max()):.2f}")
    assert 4 < med["gauss"] < 10 and med["vpos"] < 2.6 and med["voffset"] < 2.6


def test_shift_is_not_slack():
    """On sharp rows the evaluated |O1 - O(q)| exceeds the whole remaining bound (measured 2.65 x at 136 x 72 with q x 4): added as slack it
    would more than double the window exactly where it is tightest."""
    q, k, v = R.fwd_inputs(("att64", (1, 2, 136, 72), False, "sharp"))
    ref = R.fwd_o_bound(q, k, v, 2, 72, 0.125, p_sum_f16=True)
    assert float((ref.shift / ref.b1).max()) > 1.5 and float((ref.shift / ref.b1).median()) < 0.3


# ---- planted errors --------------------------------------------------------------------------------------------------------------------
# plant -> (kernel, shape, causal, family, emulate keywords, the whole-tensor bar's factor there, whether that bar passes it).  The smallest
# case of the GPU lists that shows each.  On the q x 4 family the clean restatement itself sits at 2.1 x the f16-storage figure (the
# rounding of q'), so the bar is taken with the factor 2.5 the suite gives re-referencing rows; test_clean_restatement_passes_the_old_bar
# asserts that every clean run passes the bar its plant is judged by.
DIAG_SPLIT = dict(walk="diag", tile=32, split=True, p_sum_f16=False)
PLANTS = {
    "flush_subnormal_p": ("att64", (1, 2, 128, 64), False, "sharp", {}, 2.5, True),        # 9.1 x outside; rel-L2 5.5e-4, 2.47 x: passes
    "drop_key_last_row": ("att64", (1, 2, 136, 136), False, "sharp", {}, 2.5, False),      # 11.7 x outside; one element 7.6e-3 > 7.3e-3: fails, barely
    "drop_last_key": ("att64", (1, 2, 136, 72), False, "gauss", {}, 1.35, False),
    "causal_off_by_one": ("att64", (1, 1, 8, 136), True, "gauss", {}, 1.35, False),
    "scale_for_scale_log2": ("att64", (1, 1, 8, 8), False, "gauss", {}, 1.35, False),
    "no_alpha_on_o": ("att64", (1, 2, 136, 72), False, "gauss", {}, 1.35, False),
    "split_refs_differ": ("pwg", (1, 1, 256, 512), False, "gauss", DIAG_SPLIT, 1.35, False),
    "early_o_round": ("att64", (1, 2, 136, 72), False, "voffset", {}, 1.35, False),        # 1.6 x outside; the bar fails it by its ratio clause
    #                                                                                        (the f16-storage restatement is exact on a constant V)
}


def _plant_run(name, plant):
    kn, (B, heads, Nq, Nk), causal, family, kw, factor, _ = PLANTS[name]
    q, k, v = R.fwd_inputs((kn, (B, heads, Nq, Nk), causal, family))
    psf = kw.get("p_sum_f16", True)
    ref = R.fwd_o_bound(q, k, v, heads, Nk, 0.125, p_sum_f16=psf, causal=causal, split=kw.get("split", False))
    o = R.emulate_fwd_f32(q, k, v, heads, Nk, 0.125, causal=causal, plant=plant, **kw)
    return o, ref, old_bar_passes(o, q, k, v, heads, causal, factor)


@pytest.mark.parametrize("name", list(PLANTS))
def test_planted_errors_violate_the_bound(name):
    """Each error planted into the restatement leaves B1 at the recorded case, and the whole-tensor bar's verdict on it is the recorded one.
    The errors: f16-subnormal probabilities flushed to zero (a conversion in the wrong denormal mode); key Nk / 2 never reaching the last
    live query row; the last key of a ragged tile dead; the causal mask off by one (key >= row dead); scale in place of scale log2 e; O not
    rescaled by alpha on one re-reference while l is; the two key halves of a split block merged with different references; O rounded to f16
    before the division by l (seen on a V constant along the keys only, and only through the centred term: 1.6 x)."""
    o, ref, old = _plant_run(name, name)
    r = (o.to(F64) - ref.o1).abs() / ref.b1
    print(f"{name}: largest err/bound {float(r.max()):.2f}, {int((r > 1).sum())} elements outside; the whole-tensor bar {'passes' if old else 'fails'} it")
    assert float(r.max()) > 1.0, f"{name}: not seen by the bound"
    assert old == PLANTS[name][-1], f"{name}: the whole-tensor bar {'passes' if old else 'fails'} it"


@pytest.mark.parametrize("name", list(PLANTS))
def test_clean_restatement_passes_the_old_bar(name):
    """... while the restatement without the plant is inside the bound AND passes the bar the plant is judged by."""
    o, ref, old = _plant_run(name, "")
    assert float(((o.to(F64) - ref.o1).abs() / ref.b1).max()) < 1.0 and old


def test_one_row_drop_on_gaussian_rows():
    """On long Gaussian rows the drop is small but still seen: one key dropped from one query row of 136 x 1024 Gaussian data is 5 x outside, and there the whole-tensor bar
    fails it too (the elementwise part)."""
    q, k, v = R.fwd_inputs(("att64", (1, 1, 136, 1024), False, "gauss"))
    ref = R.fwd_o_bound(q, k, v, 1, 1024, 0.125, p_sum_f16=True)
    o = R.emulate_fwd_f32(q, k, v, 1, 1024, 0.125, plant="drop_key_last_row")
    r = ratio(o, ref)
    old = old_bar_passes(o, q, k, v, 1)
    print(f"one key of 1024 dropped from one row: {r:.2f} x the bound; the whole-tensor bar {'passes' if old else 'fails'} it")
    assert r > 2.0 and not old


def crafted_row_sum_case():
    """8 queries x 128 keys, one head: every score 0 except key 100 (outside the rows' diagonal tile), whose exponent x = q'_0 k_0 is searched
    over the f16 grid so that 2^x sits just below 4098 -- f16 rounds it to 4096, a relative 2^-11 -- and v = 1.9990234375 everywhere, the
    top of its binade.  With l = sum p16 the weights sum to one and o = v exactly; with l = sum p32, o = v (1 - 4.7e-4) stores one f16 below v."""
    qs = torch.arange(0x4400, 0x4800, dtype=torch.int16).view(F16)          # q in [4, 8)
    ks = torch.arange(0x4800, 0x4C00, dtype=torch.int16).view(F16)          # k in [8, 16)
    q1 = R.q_prime(qs, 0.125).to(F32)
    p = torch.exp2(q1[:, None] * ks.to(F32)[None, :])
    p = torch.where((p > 4096) & (p < 4098), p, torch.zeros_like(p))
    i = int(p.argmax())
    assert float(p.flatten()[i]) > 4097.5, "no exponent found"
    q, k = torch.zeros(1, 8, 64, dtype=F16), torch.zeros(1, 128, 64, dtype=F16)
    q[..., 0], k[0, 100, 0] = qs[i // ks.numel()], ks[i % ks.numel()]
    return q, k, torch.full((1, 128, 64), 1.9990234375, dtype=F16)


def test_row_sum_convention_matters_for_the_centred_term():
    """sum p32 used as l with the centred term claimed: outside on the crafted case (1 f16 ulp against 1/2 ulp + the f32 part), while
    l = sum p16 gives o = v exactly -- and the same sum p32 result is inside U alone, the bound attention_pwg.hip gets.  (On the random
    families of the GPU lists this plant stays inside, at 0.7 .. 0.96: the centred term is claimed for what the code does, not for what a
    test could tell apart.)"""
    q, k, v = crafted_row_sum_case()
    centred = R.fwd_o_bound(q, k, v, 1, 128, 0.125, p_sum_f16=True)
    plain = R.fwd_o_bound(q, k, v, 1, 128, 0.125, p_sum_f16=False)
    o16 = R.emulate_fwd_f32(q, k, v, 1, 128, 0.125, walk="diag", p_sum_f16=True)
    o32 = R.emulate_fwd_f32(q, k, v, 1, 128, 0.125, walk="diag", p_sum_f16=False)
    old = old_bar_passes(o32, q, k, v, 1)
    print(f"l = sum p16: {ratio(o16, centred):.2f}; l = sum p32: {ratio(o32, centred):.2f} of the centred bound, {ratio(o32, plain):.2f} of U alone; "
          f"the whole-tensor bar {'passes' if old else 'fails'} it")
    assert torch.equal(o16, v[:, :8]) and ratio(o16, centred) < 1e-9
    assert ratio(o32, centred) > 1.0 and ratio(o32, plain) < 1.0
    assert not old  # (by its ratio clause alone: the f16-storage restatement is exact on a constant V, so any error at all is "worse than f16 storage")


@pytest.mark.parametrize("plant,kn,shape", [("trunc_p", "att64", (1, 2, 136, 72)), ("trunc_p", "stream", (1, 2, 136, 192)),
                                            ("early_o_round", "att64", (1, 2, 136, 72)), ("early_o_round", "stream", (1, 2, 136, 192))])
def test_what_the_bound_cannot_see(plant, kn, shape):
    """B1 is a worst-case bound: it charges every probability a full 2^-11 in the worst direction, so P rounded TOWARD ZERO (at most 2^-10,
    but with one sign: the numerator and l move together and most of it cancels in the quotient) and O rounded to f16 before the division
    (another half ulp of the element, against a window of several ulps on zero-mean V) stay inside it -- measured 0.29 .. 0.42 on these
    Gaussian cases, up to 0.98 on sharp rows.  The second is seen on a V constant along the keys (PLANTS["early_o_round"])."""
    B, heads, Nq, Nk = shape
    q, k, v = R.fwd_inputs((kn, shape, False, "gauss"))
    ref = R.fwd_o_bound(q, k, v, heads, Nk, 0.125, p_sum_f16=True)
    walk = "diag" if kn == "stream" else "first"
    clean, bad = (R.emulate_fwd_f32(q, k, v, heads, Nk, 0.125, walk=walk, plant=p) for p in ("", plant))
    print(f"{plant} {kn}: {ratio(bad, ref):.2f} of the bound (clean {ratio(clean, ref):.2f}), {int((bad != clean).sum())} elements differ")
    assert not torch.equal(bad, clean) and ratio(bad, ref) < 1.0


# ---- the split rule, the fallback constructions ------------------------------------------------------------------------------------------
def test_split_rule_on_the_pwg_cases():
    """pwg_split_heads on the GPU lists: the 256-row cases split nothing, the all-split cases every head, (1, 257, 256, 512) its last head,
    (3, 86, 256, 512) nothing (a remainder of two blocks is no whole head of three)."""
    assert all(R.pwg_split_heads(*s) == 0 for s in R.FWD_PWG_FULL)
    assert all(R.pwg_split_heads(*s) == s[1] for s in R.FWD_PWG_SPLIT)
    assert [R.pwg_split_heads(*s) for s in R.FWD_PWG_MIXED] == [1, 0]


@pytest.mark.parametrize("fb", R.FWD_FALLBACKS, ids=lambda f: "-".join(str(x) for x in f))
def test_fallback_constructions_exceed_the_guess(fb):
    """The intended rows beat their diagonal-tile reference by more than 14 log2 units (a probability above 2^14 > PLIM: the redo is taken by
    construction), far_tile's key lies in the second key half and one_row's in the first; the restatement (which then takes the
    max-tracking loop, as the kernels do) is inside the bound."""
    kn, kind, where, Nq, Nk = fb
    q, k, v, (bs, h, rows) = R.fallback_inputs(where, Nq, Nk)
    ex = R.fallback_excess(q, k, 3, 0.125)
    print(f"{where} {Nq}x{Nk}: excess of the intended rows {float(ex[bs][:, h][:, rows].min()):.1f} .. {float(ex[bs][:, h][:, rows].max()):.1f} log2 units")
    assert float(ex[bs][:, h][:, rows].min()) > 14
    assert kind != "split" or R.pwg_split_heads(2, 3, Nq, Nk) == 3
    assert kind != "256" or R.pwg_split_heads(2, 3, Nq, Nk) == 0
    psf = R.P_SUM_F16[R.FWD_KERNELS[kn][0]]
    ref = R.fwd_o_bound(q, k, v, 3, Nk, 0.125, p_sum_f16=psf, split=kind == "split")
    o = R.emulate_fwd_f32(q, k, v, 3, Nk, 0.125, walk="diag", tile=32, p_sum_f16=psf, split=kind == "split")
    R.assert_within(o, ref.o1, ref.b1, f"fallback {where} {Nq}x{Nk}")
