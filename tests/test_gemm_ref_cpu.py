"""CPU tests of tests/gemm_ref.py, the reference and the per-element bound the gn_gemm GPU tests (tests/test_gemm_f64_gpu.py) assert with:
  1. the f32 restatement of the kernels' arithmetic (gemm_common.h) is inside the bound on every case and family -- the bound's form holds;
  2. every plant (a plausible slip in epilogue_tile_math / epilogue_vals4 / a K-tail mask / a store path) is OUTSIDE the bound on every sharp case it
     applies to, while util.assert_close -- the bar these kernels were held to before -- lets most of them through;
  3. K_ACT is 4 x the measured f32 error of the activations;
  4. the im2col reference agrees with torch's conv2d in f64, so the reference does not depend on the packing code.
No GPU.  (The tile table is read from the built library, which loads without a device.)"""
import pytest
import torch

import gemm_ref as R
from gemm_ref import F16, F32, F64

U32 = R.U32


def _ratio(r32, ref):
    """largest |restatement's stored value - ref| / bound"""
    return float(((r32.y16.to(F64) - ref.y).abs() / ref.bound.clamp_min(1e-300)).max())


def _outside(got: torch.Tensor, ref) -> tuple:
    """-> (elements outside the bound, flat index of the worst, its err / bound)"""
    err = (got.to(F64) - ref.y).abs()
    worst = int((err / ref.bound.clamp_min(1e-300)).argmax())
    return int((err > ref.bound).sum()), worst, float(err.flatten()[worst] / ref.bound.flatten()[worst])


def test_tile_shapes_are_the_librarys():
    from genima_amd._lib import gemm_tiles  # (the one test of this module that needs the built library -- no device; the others are pure torch)

    assert sorted(set((c.bm, c.bn) for c in gemm_tiles().values())) == sorted(R.TILE_SHAPES)


# ---- 1. references stay finite; the restatement is inside the bound ----------------------------------------------------------------------------------
def test_restatement_is_inside_the_bound_dense():
    """Every dense case x family: the f64 reference is finite and below 65504, the bound is finite, and the f32 restatement's f16 result is inside it."""
    top = 0.0
    for case in R.dense_cases():
        worst = 0.0
        for fam in R.FAMILIES:
            for act, mode in R.dense_combos(case, fam):
                ref = R.dense_ref(case, fam, act, mode)
                assert torch.isfinite(ref.y).all() and float(ref.y.abs().max()) < 65504 and torch.isfinite(ref.bound).all(), (case, fam, act, mode)
                q = _ratio(R.dense_f32(case, fam, act, mode), ref)
                assert q < 1.0, (case, fam, R.ACT_NAME[act], mode, q)
                worst = max(worst, q)
        print(f"dense {case}: restatement's largest err/bound {worst:.3f}")
        top = max(top, worst)
    assert top > 0.5  # (a correctly rounded result sits up to half an ulp off: a bound that is never approached would be vacuous)


def test_restatement_is_inside_the_bound_splitk_geglu_f32out():
    for (case, sk) in R.SPLITK_CASES:
        x, w, b, r = R.dense_inputs(case)
        n = sk if sk else R.AUTO_SPLITK_MAX
        for kw in (dict(bias=b, act=R.ACT_SILU), dict(res=r)):
            ref = R.gemm_ref(F64, x, w, splitk=n, **kw)
            assert torch.isfinite(ref.y).all() and float(ref.y.abs().max()) < 65504
            q = _ratio(R.gemm_ref(F32, x, w, **kw), ref)
            print(f"split-K {case} x{sk} {sorted(kw)}: {q:.3f}")
            assert q < 1.0
    for case in R.GEGLU_CASES:
        x, wp, bp, ref = R.geglu_fixture(case)
        q = _ratio(R.gemm_ref(F32, x, wp, bp, act=R.ACT_GEGLU), ref)
        print(f"GEGLU {case}: {q:.3f}")
        assert q < 1.0 and ref.y.shape == (case[0], case[1])
    x, w, _, _ = R.dense_inputs((200, 136, 128))
    one, r32 = R.gemm_ref(F64, x, w, out_f32=True), R.gemm_ref(F32, x, w, out_f32=True)
    assert _ratio(r32, one) < 1.0
    two = R.accumulate_twice_ref(x, w, 0.25)
    y2 = (torch.full_like(r32.y, 0.25) + r32.y) + r32.y
    q = float(((y2.to(F64) - two.y).abs() / two.bound).max())
    print(f"f32 output, two accumulating calls: {q:.3f}")
    assert q < 1.0


@pytest.mark.parametrize("case", R.CONV_CASES, ids=R.conv_id)
def test_conv_reference_is_torch_conv2d_and_restatement_inside_bound(case):
    """The im2col matrix times the packed weight IS torch.nn.functional.conv2d in f64 (1e-12 relative): stride, four-sided pad, virtual concat, fused
    nearest-2x upsample.  And the f32 restatement of the whole conv call is inside the bound."""
    c, ref = R.conv_fixture(case)
    plain = R.conv_ref(F64, c.x, c.x2, c.w, c.bias, c.k, c.stride, c.pad, c.ups)
    want = R.conv2d_f64(c.x, c.x2, c.w, c.bias, c.k, c.stride, c.pad, c.ups)
    assert plain.y.shape == want.shape == (c.B, c.Ho, c.Wo, c.Cout)
    assert float((plain.y - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.isfinite(ref.y).all() and float(ref.y.abs().max()) < 65504
    q = _ratio(R.conv_case_ref(F32, c), ref)
    print(f"conv {R.conv_id(case)}: restatement's largest err/bound {q:.3f}")
    assert q < 1.0


@pytest.mark.parametrize("kind", R.LN_KINDS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_restatement_is_inside_the_bound_layernorm_fold(case, kind):
    """One-pass f32 statistics on rows with |mean| = 0, 6 and 20 spreads: the variance's error is relative to sum x^2 / K + mean^2, and the bound carries it."""
    ref = R.ln_fixture(case, kind)[-1]
    assert torch.isfinite(ref.y).all() and torch.isfinite(ref.bound).all() and float(ref.y.abs().max()) < 65504
    r32 = R.ln_f32(case, kind)
    ratio = (r32.y16.to(F64) - ref.y).abs() / ref.bound
    q = float(ratio.max())
    per_mean = [float(ratio[i::len(R.LN_MEANS)].max()) for i in range(len(R.LN_MEANS))]
    print(f"LayerNorm fold {R.ln_shape(case, kind)} {kind}: {q:.3f}; by |mean| / sigma {R.LN_MEANS}: {[round(v, 3) for v in per_mean]}")
    assert q < 1.0
    # the reference is LayerNorm -> Linear on the same numbers (torch, f64): the folded formula is algebra, not an approximation (c1 is GIVEN as the f32
    # sum of the rounded weight row: its own rounding, K 2^-24 sum|w'| times |mean| rstd <= 20, is the difference allowed here)
    if kind == "gelu":
        x, w, b, gamma, beta, _ = R.ln_inputs(R.ln_shape(case, kind))
        wg, c1, c2 = R.fold_layernorm(w, gamma, beta, b)
        ln = torch.nn.functional.layer_norm(x.to(F64), (x.shape[1],), None, None, R.eps32(1e-5))
        z = ln @ wg.to(F64).t() + c2.to(F64)
        assert float((ref.z - z).abs().max()) <= 20 * x.shape[1] * U32 * float(wg.to(F64).abs().sum(1).max())


# ---- 2. the plants -------------------------------------------------------------------------------------------------------------------------------------
# plant -> (activation, mode) it is planted under on the dense sharp cases
DENSE_PLANTS = {
    "tanh_gelu": (R.ACT_GELU, "bias"),
    "acc_f16_before_bias": (R.ACT_NONE, "bias"),
    "acc_f16_per_ktile": (R.ACT_NONE, "bias"),
    "act_f16_then_residual": (R.ACT_SILU, "bias_res"),
    "drop_last_k_last_row": (R.ACT_NONE, "bias"),
    "res_after_for_res_first": (R.ACT_SILU, "bias_res_first"),
    "scale_before_act": (R.ACT_SILU, "scale"),
}
# the old bar has to let these through on at least one sharp case: that is why the new bar exists
OLD_BAR_BLIND_TO = ("tanh_gelu", "acc_f16_before_bias", "acc_f16_per_ktile", "act_f16_then_residual")


@pytest.mark.parametrize("plant", list(DENSE_PLANTS))
def test_dense_plants_are_outside_the_new_bar(plant):
    """Every dense plant, on every sharp case (gemm_ref.sharp_cases: K <= 200): at least one element outside the bound, named here.  The four
    rounding / approximation plants (tanh_gelu, acc_f16_before_bias, acc_f16_per_ktile, act_f16_then_residual) pass util.assert_close's two conditions
    (old_bar_passes) -- measured: on every sharp case.  drop_last_k_last_row FAILS the old bar on every case of this list and is a plant of the new bar
    only: the dropped term is x[M-1, K-1] w[n, K-1], up to 3 K^-1/2 |x| over a row of N columns, and the old bar's 2e-3 max|ref| + 1e-3 ~ 0.01 lets it
    through only where the draw made |x[M-1, K-1]| < 0.04 (3 % of Gaussian draws; none of these).  res_after_for_res_first and scale_before_act are
    errors of O(1) and fail either bar."""
    act, mode = DENSE_PLANTS[plant]
    blind = 0
    for case in R.sharp_cases():
        ref = R.dense_ref(case, "gauss", act, mode)
        got = R.dense_f32(case, "gauss", act, mode, plant=plant).y16
        n, worst, q = _outside(got, ref)
        old = R.old_bar_passes(got, ref.y)
        blind += old
        M, N, _ = case
        print(f"{plant} @ {case} {R.ACT_NAME[act]} {mode}: {n} of {M * N} elements out, worst (row {worst // N}, col {worst % N}) at {q:.1f} x the bound; "
              f"old bar {'PASSES' if old else 'fails'}")
        assert n >= 1, (plant, case)
    if plant in OLD_BAR_BLIND_TO:
        assert blind >= 1, plant
    else:
        assert blind == 0, plant


def test_geglu_plants():
    """geglu_halves_swapped is outside the new bar (and, an O(1) error, outside the old one too); the tanh GELU in the gate -- the GEGLU-side plant the old
    bar lets through -- is outside the new bar on both cases."""
    for case in R.GEGLU_CASES:
        x, wp, bp, ref = R.geglu_fixture(case)
        for plant, old_blind in (("geglu_halves_swapped", False), ("tanh_gelu", True)):
            got = R.gemm_ref(F32, x, wp, bp, act=R.ACT_GEGLU, plant=plant).y16
            n, worst, q = _outside(got, ref)
            old = R.old_bar_passes(got, ref.y)
            print(f"{plant} @ GEGLU {case}: {n} elements out, worst (row {worst // case[1]}, col {worst % case[1]}) at {q:.1f} x the bound; old bar {'PASSES' if old else 'fails'}")
            assert n >= 1 and old == old_blind


def test_conv_plant_tap_off_by_one_at_the_border():
    """conv_tap_off_by_one_at_border on every conv case whose right-hand padding column is read at all (stride 1, or the asymmetric pad): outside the new
    bar at an output pixel of the last column.  It fails the old bar as well (the border pixels are off by O(1)): a plant of the new bar only."""
    applied = 0
    for case in R.CONV_CASES:
        c, ref = R.conv_fixture(case)
        pad = (c.k // 2,) * 4 if c.pad is None else c.pad
        same = torch.equal(R.im2col(c.x, c.x2, c.k, c.stride, pad, c.ups, "conv_tap_off_by_one_at_border")[0], R.im2col(c.x, c.x2, c.k, c.stride, pad, c.ups)[0])
        if same:
            continue
        applied += 1
        got = R.conv_case_ref(F32, c, plant="conv_tap_off_by_one_at_border").y16
        n, worst, q = _outside(got, ref)
        ox = worst // c.Cout % c.Wo
        print(f"conv_tap_off_by_one_at_border @ {R.conv_id(case)}: {n} elements out, worst at output column {ox} of {c.Wo}, {q:.1f} x the bound; "
              f"old bar {'PASSES' if R.old_bar_passes(got, ref.y) else 'fails'}")
        assert n >= 1 and ox == c.Wo - 1
    assert applied >= 5


def test_conv_plant_bias_and_shift_summed_in_f16():
    """conv_bias_plus_shift_f16 -- the bias and the per-sample time shift combined in f16 before they meet the accumulator, a slip only the conv call sites
    can make (Engine.linear has no shift) -- on every conv case with a shift the old bar PASSES it (half an f16 ulp of bias + shift); it is outside the new bar
    where K is short enough for the bar to be sharp (K = 288 here: asserted); at K = 576 and 648 the accumulation term is as large as the slip and the few elements
    that still fall outside are printed, not asserted."""
    cases = [case for case in R.CONV_CASES if case[R.CONV_FIELDS.index("shift")]]
    assert len(cases) >= 3
    for case in cases:
        c, ref = R.conv_fixture(case)
        got = R.conv_case_ref(F32, c, plant="conv_bias_plus_shift_f16").y16
        n, worst, q = _outside(got, ref)
        old = R.old_bar_passes(got, ref.y)
        print(f"conv_bias_plus_shift_f16 @ {R.conv_id(case)}: {n} elements out, worst at flat index {worst}, {q:.1f} x the bound; old bar {'PASSES' if old else 'fails'}")
        assert old and (n >= 1 or c.k * c.k * (c.C1 + c.C2) > 300)
    assert any(c[6] * c[6] * (c[3] + c[4]) <= 300 for c in cases)


LOW_MEANS = (0.0, 1.0)


@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layernorm_fold_plants(case):
    """ln_var_two_terms_f16 and (where K is no multiple of 64) ln_mean_of_padded_k are outside the new bar.  On rows of |mean| <= 1 spread -- the rows the
    workload has -- the f16 variance terms are wrong by 1e-4 relative and the old bar PASSES them; with the 6 and 20 spread rows it fails too."""
    M, N, K = case
    ref = R.ln_fixture(case, "res")[-1]
    got = R.ln_f32(case, "res", plant="ln_var_two_terms_f16").y16
    n, worst, q = _outside(got, ref)
    print(f"ln_var_two_terms_f16 @ {case}: {n} elements out, worst (row {worst // N}, col {worst % N}) at {q:.1f} x the bound; old bar "
          f"{'PASSES' if R.old_bar_passes(got, ref.y) else 'fails'}")
    assert n >= 1
    ref_low = R.ln_fixture(case, "res", LOW_MEANS)[-1]
    got = R.ln_f32(case, "res", plant="ln_var_two_terms_f16", means=LOW_MEANS).y16
    n, worst, q = _outside(got, ref_low)
    print(f"ln_var_two_terms_f16 @ {case}, |mean| <= 1 spread: {n} elements out, worst (row {worst // N}, col {worst % N}) at {q:.1f} x the bound")
    assert n >= 1 and R.old_bar_passes(got, ref_low.y)
    assert float(((R.ln_f32(case, "res", means=LOW_MEANS).y16.to(F64) - ref_low.y).abs() / ref_low.bound).max()) < 1.0
    if K % 64:
        got = R.ln_f32(case, "res", plant="ln_mean_of_padded_k").y16
        n, worst, q = _outside(got, ref)
        print(f"ln_mean_of_padded_k @ {case}: {n} elements out, worst (row {worst // N}, col {worst % N}) at {q:.1f} x the bound")
        assert n >= 1


# ---- 3. K_ACT ------------------------------------------------------------------------------------------------------------------------------------------
def test_k_act_is_four_times_the_measured_f32_error():
    """K_ACT = 4 x the largest |f32 activation - f64| / (2^-24 T_act) over every case.  The figure depends a little on the CPU's exp: it may sit up to 25 %
    above or a factor 2 below the recorded one, not further -- K_ACT cannot be inflated quietly."""
    got = R.measure_k_act()
    print({n: round(v, 4) for n, v in got.items()})
    for n, rec in R.K_ACT_MEASURED.items():
        assert 0.5 * rec <= got[n] <= 1.25 * rec, (n, got[n], rec)
        assert R.K_ACT[n] == 4 * rec


# ---- 4. the bound is sharp where it is meant to be -----------------------------------------------------------------------------------------------------
def test_the_bound_is_the_f16_half_ulp_at_short_k():
    """On the Gaussian sharp cases without activation the median bound / (1/2 ulp16) stays below 2: E_z = 2 (K + 1) 2^-24 sum|x||w| with sum|x||w| ~ 0.64 sqrt K
    is 2.0e-4 at K = 192 against a half-ulp of 2.4e-4 for |y| in [0.5, 1) -- the accumulation term is below the store's own rounding, which is what makes
    the f16-rounding plants visible (at K = 11520 it is 400 times that: the split-K cases are looser, as the module's docstring says)."""
    for case in R.sharp_cases():
        ref = R.dense_ref(case, "gauss", R.ACT_NONE, "bias")
        med = float((ref.bound / (0.5 * R.ulp16(ref.y))).median())
        print(f"{case}: median bound / half-ulp {med:.3f}")
        assert med < 2.0
    assert R.ulp16(torch.tensor([3.0e-5], dtype=F64)).item() == 2.0 ** -24  # the subnormal spacing: the `tiny` family's results are held to it
    y = R.dense_ref(R.SHARED_TRIPLES[1], "tiny", R.ACT_NONE, "nobias").y.abs()
    assert float((y < 2.0 ** -14).float().mean()) > 0.3 and float(y.max()) < 2.0 ** -10
