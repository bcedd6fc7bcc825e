"""No GPU: the references and bounds of tests/norm_fwd_ref.py, which tests/test_norm_fwd_gpu.py holds the forward kernels to.
  * the f64 closed forms agree with torch in float64 (F.layer_norm, F.group_norm (+ F.silu) on the concatenated input, torch.softmax) to 1e-12;
  * the f32 restatement of the kernels' arithmetic stays inside the bounds on every element of every case and family of the GPU module;
  * the constants of the bounds are the measured ones (K = 4 x the restatement's worst error);
  * the bounds are not vacuous: their median against |ref| on the Gaussian cases is capped at twice the recorded figure (about the f16 store);
  * tightness: one planted error at a time, stored as f16 as a kernel would, leaves the bounds on a named small case -- printed with the count
    of elements out and with whether tests/util.py::assert_close (the bar these outputs were judged by before) would have let it through.

Measured here (pytest -s):
  K_MEASURED re-measured: ln_y 2.62, gn_z 1.986, silu 1.956, softmax_y 0.9425
  median bound / |ref| (Gaussian cases): ln 3.49e-04, gn 3.57e-04, stats_in 3.52e-04, softmax 3.53e-04 (capped at twice that)
  plants (elements out of bound / of; whether the old bar lets it through):
    variance_over_n_minus_1 (5, 1024) gauss    3600 / 5120      PASSES the old bar (rstd off by 4.9e-4)
    eps_outside_sqrt (5, 520) lowvar           2600 / 2600      fails it
    dead_lanes_in_variance (5, 520) offset     2600 / 2600      fails it
    last_chunk_params (3, 1032) gauss          24 / 3096        fails it
    last_row_unnormalised (8195, 64) gauss     64 / 524480      fails it
    silu_before_affine (2, 144, 64, 0, 32)     18381 / 18432    fails it
    stats_of_x1_only (2, 64, 640, 320, 32)     3816 / 122880    fails it
    chunk_first_group (2, 64, 96, 0, 8) r3     1998 / 12288     fails it
    ninth_replica_dropped (2, 64, 640, 320, 32) r9  122878 / 122880  fails it
    masked_columns_given_mass (5, 72) valid 69 284 / 360        fails it
    row_sum_before_mask (5, 72) valid 69       272 / 360        fails it
  The plants are gross by design (a wrong formula, not a wrong rounding); what the old bar cannot see is anything below 1e-3 of the tensor, as
  the first one shows."""
import pytest
import torch
import torch.nn.functional as F

import norm_fwd_ref as R

F16, F32, F64 = torch.float16, torch.float32, torch.float64
ACTS = (R.ACT_NONE, R.ACT_SILU)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- 1. the references against torch in f64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("case", [(3, 8), (5, 520), (3, 1032), (5, 4096), (2049, 320)], ids=R.ln_id)
def test_layernorm_reference_is_torch(case, fam):
    x, gamma, beta, ref, _ = R.ln_fixture(case, fam)
    want = F.layer_norm(x.to(F64), (case[1],), gamma.to(F64), beta.to(F64), R.eps32(R.EPS))
    assert _rel(ref.y, want) <= 1e-12


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fam", ["gauss", "offset", "tailmark"])  # (lowvar: mean x^2 - mean^2 in f64 is good to 2^-53 / (var + eps) ~ 1e-11 only)
@pytest.mark.parametrize("case", [R.GN_CASES[0], R.GN_CASES[3], R.GN_CASES[6], R.FWD_THREE[1], R.GN_THREE_MORE[1]], ids=R.gn_id)
def test_groupnorm_reference_is_torch(case, fam, act):
    B, HW, C1, C2, G = case
    x1, x2, gamma, beta, sv = R.gn_fixture(case, fam)
    y = R._apply(F64, R._cat(x1, x2), sv.scsh[..., 0], sv.scsh[..., 1], act)[0]
    want = F.group_norm(R._cat(x1, x2).to(F64).permute(0, 2, 1), G, gamma.to(F64), beta.to(F64), R.eps32(R.EPS)).permute(0, 2, 1)
    assert _rel(y, F.silu(want) if act else want) <= 1e-12


@pytest.mark.parametrize("case", [R.SI_CASES[5], R.SI_CASES[10], R.SI_CASES[-1]], ids=R.si_id)
def test_stats_in_reference_is_torch_up_to_the_bridge_quantum(case):
    """The reference takes the handed integer totals as exact, so it differs from group_norm of x by the bridge's quantisation: half a quantum
    2^-13 of the sum of squares over n >= 640 elements against var + eps ~ 1 (Gaussian) is 2e-7 of rstd."""
    x, x1, x2, gamma, beta, blk = R.si_fixture(case, "gauss")
    ref = R._gn_stats_in(F64, x, gamma, beta, blk, case[4], R.ACT_NONE)
    want = F.group_norm(x.to(F64).permute(0, 2, 1), case[4], gamma.to(F64), beta.to(F64), R.eps32(R.EPS)).permute(0, 2, 1)
    assert _rel(ref.y, want) <= 1e-6


@pytest.mark.parametrize("case", [(5, 8), (5, 72), (33, 520), (5, 4096)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_softmax_reference_is_torch(case):
    x = R.softmax_inputs(case)
    for valid in R.softmax_valids(case[1]):
        for scale in R.SOFTMAX_SCALES:
            y, T = R.softmax_ref(x, scale, valid)
            want = torch.softmax(x.to(F64)[:, :valid] * scale, -1)
            assert _rel(y[:, :valid], want) <= 1e-12 and float(y[:, valid:].abs().sum()) == 0.0 and bool((T[:, valid:] == 0).all())


def test_the_silu_slope_maximum_is_one():
    """silu_slope_max against a dense scan of |silu'| over random intervals, those around +-z* included."""
    g = torch.Generator().manual_seed(1)
    lo = torch.cat([8 * torch.randn(2000, generator=g, dtype=F64), torch.tensor([-2.41, 2.39, -30.0, -2.5, 2.3])])
    hi = lo + torch.cat([torch.rand(2000, generator=g, dtype=F64) ** 4 * 6, torch.tensor([0.02, 0.02, 60.0, 5.0, 0.05])])
    scan = R._silu_slope(lo[:, None] + (hi - lo)[:, None] * torch.linspace(0, 1, 4001, dtype=F64)).abs().max(-1).values
    got = R.silu_slope_max(lo, hi)
    assert bool((got >= scan - 1e-12).all()) and bool((got <= scan + 1e-5).all())  # (1e-12: the scan's own abscissae are rounded)


# ---- 2. the restatement inside the bounds; 6. the stored reference inside them ----------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LN_CASES, ids=R.ln_id)
def test_layernorm_restatement_inside_bounds(case):
    assert R.ln_fwd_route(*case) in R.LN_ROUTES
    worst = 0.0
    for fam in R.FAMILIES:
        x, gamma, beta, ref, bound = R.ln_fixture(case, fam)
        worst = max(worst, R.assert_within(R.ln_fwd_f32(x, gamma, beta).y, ref.y, bound, f"ln {case} {fam}", quiet=True))
        R.assert_within(ref.y.to(F16), ref.y, bound, f"ln {case} {fam}: the stored reference", quiet=True)
    print(f"ln {case} {R.ln_fwd_route(*case)}: restatement max err/bound {worst:.3f}")


@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_id)
def test_groupnorm_restatement_inside_bounds(case):
    route = R.gn_fwd_route(*case)
    assert route == R.GN_ROUTE[case]
    worst = 0.0
    for fam in R.FAMILIES:
        x1, x2, gamma, beta, sv = R.gn_fixture(case, fam)
        for act in ACTS:
            ref, bound = R.gn_fwd_bound(x1, x2, gamma, beta, sv, act)
            r32 = R.gn_fwd_f32(x1, x2, gamma, beta, case[4], act, route)
            worst = max(worst, R.assert_within(r32.y, ref, bound, f"gn {case} {fam} act {act} ({route})", quiet=True))
            R.assert_within(ref.to(F16), ref, bound, "the stored reference", quiet=True)
    print(f"gn {case} ({route}): restatement max err/bound {worst:.3f}")


@pytest.mark.parametrize("case", R.STATS_ONLY_CASES, ids=R.gn_id)
def test_statistics_only_restatement_inside_bounds(case):
    """The statistics-only call runs the three-launch statistics whatever the shape: its restatement at the bounds of norm_bwd_ref."""
    for fam in R.FAMILIES:
        x1, x2, gamma, beta, sv = R.gn_fixture(case, fam)
        s32, b = R.gn_saved_f32(x1, x2, gamma, beta, case[4], route="three"), R.gn_saved_bounds(sv, gamma, beta)
        R.assert_within(s32.stats, sv.stats, b["stats"], f"stats-only stats {case} {fam}")
        R.assert_within(s32.scsh, sv.scsh, b["scsh"], f"stats-only scsh {case} {fam}")


@pytest.mark.parametrize("case", R.SI_CASES, ids=R.si_id)
def test_stats_in_restatement_inside_bounds(case):
    worst = 0.0
    for fam in R.FAMILIES:
        x, x1, x2, gamma, beta, blk = R.si_fixture(case, fam)
        assert int(blk[..., 2:].ne(R.STATS_SENTINEL).sum()) == 0 and blk.shape[0] == case[5]
        for act in ACTS:
            ref, bound = R.stats_in_bound(x, gamma, beta, R._gn_stats_in(F64, x, gamma, beta, blk, case[4], act), act)
            y32 = R._gn_stats_in(F32, x, gamma, beta, blk, case[4], act).y.to(F16)
            worst = max(worst, R.assert_within(y32, ref, bound, f"stats_in {case} {fam} act {act}", quiet=True))
            R.assert_within(ref.to(F16), ref, bound, "the stored reference", quiet=True)
    print(f"stats_in {case}: restatement max err/bound {worst:.3f}")


@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_softmax_restatement_inside_bounds(case):
    x = R.softmax_inputs(case)
    for valid in R.softmax_valids(case[1]):
        for scale in R.SOFTMAX_SCALES:
            (y64, T), (y32, _) = R._softmax(F64, x, scale, valid), R._softmax(F32, x, scale, valid)
            R.assert_within(y32.to(F16), y64, R.softmax_bound(y64, T), f"softmax {case} valid {valid} scale {scale}", quiet=True)
            R.assert_within(y64.to(F16), y64, R.softmax_bound(y64, T), "the stored reference", quiet=True)
            assert abs(float(y64.to(F16).to(F64).sum(-1).max()) - 1) <= case[1] * 2.0 ** -11


# ---- 3. the constants ---------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_measured_ones():
    """K_MEASURED is the restatement's worst error over every case and family, re-measured here: at most 25 % above the recorded figure (another
    CPU's exp) and at most a factor 2 below it -- a looser constant than the arithmetic needs would be a tolerance chosen by hand."""
    got = R.measure_constants()
    print({n: round(v, 4) for n, v in got.items()})
    for n, rec in R.K_MEASURED.items():
        assert 0.5 * rec <= got[n] <= 1.25 * rec, (n, got[n], rec)
        assert R.K[n] == R.MARGIN * rec


# ---- 4. the bounds are not vacuous ----------------------------------------------------------------------------------------------------------------
def _median_ratio(pairs) -> float:
    r = torch.cat([(b / y.abs().clamp_min(1e-300)).flatten()[::7] for y, b in pairs])
    return float(r.median())


def test_the_bounds_are_not_vacuous():
    """Median bound / |ref| on the Gaussian cases: about the f16 store's 2^-12 .. 2^-11 of the value, against 1e-3 of the whole tensor's norm
    plus 2e-3 max|ref| + 1e-3 per element before."""
    got = {"ln": _median_ratio([(f[3].y, f[4]) for f in (R.ln_fixture(c, "gauss") for c in R.LN_CASES)])}
    gn = []
    for c in R.GN_CASES:
        x1, x2, gamma, beta, sv = R.gn_fixture(c, "gauss")
        gn += [R.gn_fwd_bound(x1, x2, gamma, beta, sv, act) for act in ACTS]
    got["gn"] = _median_ratio(gn)
    si = []
    for c in R.SI_CASES:
        x, x1, x2, gamma, beta, blk = R.si_fixture(c, "gauss")
        si += [R.stats_in_bound(x, gamma, beta, R._gn_stats_in(F64, x, gamma, beta, blk, c[4], act), act) for act in ACTS]
    got["stats_in"] = _median_ratio(si)
    sm = []
    for c in R.SOFTMAX_CASES:
        y, T = R.softmax_ref(R.softmax_inputs(c), 0.125, c[1])
        sm.append((y, R.softmax_bound(y, T)))
    got["softmax"] = _median_ratio(sm)
    print("median bound / |ref|:", {n: f"{v:.3e}" for n, v in got.items()})
    for n, v in got.items():
        assert v <= 2 * R.TIGHTNESS[n], (n, v)
        assert v >= 2.0 ** -13, "below a quarter f16 ulp no store can comply"


# ---- 5. planted errors ------------------------------------------------------------------------------------------------------------------------------
def _planted(name, bad64, ref, bound, expect_old=None):
    bad = bad64.to(F16)
    out = int(((bad.to(F64) - ref).abs() > bound).sum())
    old = R.old_bar_passes(bad, ref)
    print(f"plant {name}: {out} / {ref.numel()} elements out of bound; the old bar {'PASSES it' if old else 'fails it'}")
    assert R.breaks(bad, ref, bound) and out > 0, name
    assert not R.breaks(ref.to(F16), ref, bound), "the unplanted reference, stored as f16, is inside"
    return old


@pytest.mark.parametrize("plant,case,fam", [("variance_over_n_minus_1", (5, 1024), "gauss"), ("eps_outside_sqrt", (5, 520), "lowvar"),
                                            ("dead_lanes_in_variance", (5, 520), "offset"), ("last_chunk_params", (3, 1032), "gauss"),
                                            ("last_row_unnormalised", (8195, 64), "gauss")])
def test_layernorm_plants_leave_the_bounds(plant, case, fam):
    assert plant != "last_row_unnormalised" or R.ln_fwd_route(*case)[1] > 1
    x, gamma, beta, ref, bound = R.ln_fixture(case, fam)
    old = _planted(f"{plant} {case} {fam}", R.ln_fwd_ref(x, gamma, beta, plant=plant).y, ref.y, bound)
    if plant == "variance_over_n_minus_1":
        assert old, "rstd off by 1 / (2 C) = 4.9e-4: inside the old bar"


@pytest.mark.parametrize("plant,case", [("silu_before_affine", (2, 144, 64, 0, 32)), ("stats_of_x1_only", (2, 64, 640, 320, 32))])
def test_groupnorm_plants_leave_the_bounds(plant, case):
    x1, x2, gamma, beta, sv = R.gn_fixture(case, "gauss")
    ref, bound = R.gn_fwd_bound(x1, x2, gamma, beta, sv, R.ACT_SILU)
    _planted(f"{plant} {case}", R._gn_fwd(F64, x1, x2, gamma, beta, case[4], R.ACT_SILU, "fused", plant=plant).y, ref, bound)


@pytest.mark.parametrize("plant,case", [("chunk_first_group", (2, 64, 96, 0, 8)), ("ninth_replica_dropped", (2, 64, 640, 320, 32))])
def test_stats_in_plants_leave_the_bounds(plant, case):
    case = next(c for c in R.SI_CASES if c[:5] == case and (plant != "ninth_replica_dropped" or c[5] == 9))
    x, x1, x2, gamma, beta, blk = R.si_fixture(case, "gauss")
    ref, bound = R.stats_in_bound(x, gamma, beta, R._gn_stats_in(F64, x, gamma, beta, blk, case[4], R.ACT_SILU), R.ACT_SILU)
    _planted(f"{plant} {case}", R._gn_stats_in(F64, x, gamma, beta, blk, case[4], R.ACT_SILU, plant=plant).y, ref, bound)


@pytest.mark.parametrize("plant", ["masked_columns_given_mass", "row_sum_before_mask"])
def test_softmax_plants_leave_the_bounds(plant):
    x = R.softmax_inputs((5, 72))
    y, T = R.softmax_ref(x, 1.0, 69)
    _planted(f"{plant} (5, 72) valid 69", R.softmax_ref(x, 1.0, 69, plant=plant)[0], y, R.softmax_bound(y, T))
