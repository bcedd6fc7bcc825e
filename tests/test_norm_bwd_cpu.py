"""No GPU: the references and bounds of tests/norm_bwd_ref.py, which tests/test_norm_bwd_gpu.py holds the kernels to.
  * the f64 closed forms agree with torch autograd in float64 (F.layer_norm; F.group_norm (+ F.silu) on the concatenated input; the activations,
    GEGLU and softmax) to 2^-40 of the magnitude sums T of the bounds, and the forward-saved stats / scsh reference with its definition;
  * the f32 restatement of the kernels' arithmetic stays inside the bounds on every case and family -- at the GPU tests' own shapes: the
    largest ones (M = 16321, HW = 6400) restate in well under a second, so no smaller stand-in is used anywhere;
  * the constants of the bounds are the measured ones (K = 4 x the restatement's worst error, per output);
  * tightness: the restatement with one planted error breaks the bound on the family built for that error."""
import pytest
import torch
import torch.nn.functional as F

import norm_bwd_ref as R

F16, F32, F64 = torch.float16, torch.float32, torch.float64
AUTOGRAD_REL = 2.0 ** -40  # of T, the magnitude sums: 2^13 roundings of 2^-53 -- more than any f64 chain here accumulates (<= 6400 terms)


# ---- the references against autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["gauss", "offset", "lowvar", "rowmark"])
@pytest.mark.parametrize("case", [(3, 8), (300, 320), (7, 1032), (4081, 320)], ids=R.ln_id)
def test_layernorm_reference_is_autograd(case, fam):
    x, gamma, dy, ref = R.ln_fixture(case, fam)
    C = case[1]
    xa, ga, ba = x.to(F64).requires_grad_(True), gamma.to(F64).requires_grad_(True), torch.zeros(C, dtype=F64, requires_grad=True)
    F.layer_norm(xa, (C,), ga, ba, R.eps32(R.EPS)).backward(dy.to(F64))
    for n, g in (("dx", xa.grad), ("dgamma", ga.grad), ("dbeta", ba.grad)):
        R.assert_within(getattr(ref, n), g, AUTOGRAD_REL * getattr(ref, n + "_T") + 1e-300, f"layernorm {case} {fam} {n} vs autograd")


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
@pytest.mark.parametrize("fam", ["gauss", "offset", "lowvar", "chanmark"])
@pytest.mark.parametrize("case", [R.GN_CASES[0], R.GN_CASES[3], R.GN_CASES[7], R.GN_CASES[12]], ids=R.gn_id)
def test_groupnorm_reference_is_autograd(case, fam, act):
    """gn_bwd_ref on the UNROUNDED f64 stats / scsh is the autograd gradient of group_norm (+ silu) over the concatenated input."""
    B, HW, C1, C2, G = case
    x1, x2, gamma, beta, dy, st, sc, sv, _ = R.gn_fixture(case, fam, act)
    ref = R.gn_bwd_ref(x1, x2, gamma, dy, sv.stats, sv.scsh, G, act)
    nchw = lambda t: t.to(F64).permute(0, 2, 1).reshape(B, -1, HW, 1)
    xa = nchw(torch.cat([x1, x2], -1) if x2 is not None else x1).requires_grad_(True)
    ga, ba = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    y = F.group_norm(xa, G, ga, ba, R.eps32(R.EPS))
    (F.silu(y) if act else y).backward(nchw(dy))
    dx = xa.grad.reshape(B, C1 + C2, HW).permute(0, 2, 1)
    for n, g in (("dx", dx), ("dgamma", ga.grad), ("dbeta", ba.grad)):
        R.assert_within(getattr(ref, n), g, AUTOGRAD_REL * getattr(ref, n + "_T") + 1e-300, f"groupnorm {case} {fam} act {act} {n} vs autograd")


@pytest.mark.parametrize("fam", R.FWD_FAMILIES)
@pytest.mark.parametrize("case", [R.GN_CASES[3], R.GN_CASES[6], R.FWD_THREE[1]], ids=R.gn_id)
def test_saved_reference_is_the_definition(case, fam):
    """stats[b][g] = (mean, rstd) of the group's HW x cpg slab (biased variance), scsh[b][c] = (rstd gamma, beta - mean rstd gamma)."""
    B, HW, C1, C2, G = case
    x1, x2, gamma, beta, sv = R.fwd_fixture(case, fam)
    x = (torch.cat([x1, x2], -1) if x2 is not None else x1).to(F64)
    cpg = (C1 + C2) // G
    for b in range(B):
        for g in range(G):
            var, mean = torch.var_mean(x[b, :, g * cpg:(g + 1) * cpg], unbiased=False)
            rstd = 1 / torch.sqrt(var + R.eps32(R.EPS))
            T = float(sv.var_T[b, g])  # the two-pass variance of torch against mean x^2 - mean^2: both within 2^-40 of mean x^2
            assert abs(float(sv.mean[b, g] - mean)) <= AUTOGRAD_REL * float(sv.mean_T[b, g])
            assert abs(float(sv.rstd[b, g] - rstd)) <= 0.5 * float(rstd) ** 3 * AUTOGRAD_REL * T * 2
            a = sv.rstd[b, g] * gamma[g * cpg:(g + 1) * cpg].to(F64)
            assert torch.equal(sv.scsh[b, g * cpg:(g + 1) * cpg, 0], a)
            assert torch.equal(sv.scsh[b, g * cpg:(g + 1) * cpg, 1], beta[g * cpg:(g + 1) * cpg].to(F64) - sv.mean[b, g] * a)
    assert torch.equal(sv.stats[..., 0], sv.mean) and torch.equal(sv.stats[..., 1], sv.rstd)


def test_pointwise_references_are_autograd():
    dy, z = R.act_inputs()
    fwd = {R.ACT_NONE: lambda t: t, R.ACT_SILU: F.silu, R.ACT_GELU: F.gelu, R.ACT_QUICK_GELU: lambda t: t * torch.sigmoid(1.702 * t), R.ACT_RELU: torch.relu}
    for act, fn in fwd.items():
        za = z.to(F64).requires_grad_(True)
        fn(za).backward(dy.to(F64))
        val, T = R.act_bwd_terms(F64, dy, z, act)
        k = float(torch.tensor(1.702, dtype=F32)) / 1.702 - 1  # the kernel's 1.702f against the double: relative |k z| of the sigmoid's slope
        slack = abs(k) * dy.to(F64).abs() * (1 + z.to(F64).abs()) ** 2 if act == R.ACT_QUICK_GELU else 0
        R.assert_within(val, za.grad, AUTOGRAD_REL * (T + dy.to(F64).abs()) + slack, f"act {act} vs autograd")
    for blk in (0, 32):
        d, hg = R.geglu_inputs()
        ha = hg.to(F64).requires_grad_(True)
        h, g = R.geglu_split(ha, blk)
        (h * F.gelu(g)).backward(d.to(F64))
        val, T = R.geglu_bwd_terms(F64, d, hg, blk)
        R.assert_within(val, ha.grad, AUTOGRAD_REL * T + 1e-300, f"geglu blk {blk} vs autograd")
    g = torch.Generator().manual_seed(3)
    s, dp = torch.randn(5, 520, generator=g, dtype=F64).requires_grad_(True), torch.randn(5, 520, generator=g, dtype=F64)
    p = torch.softmax(0.125 * s, -1)
    p.backward(dp)
    val, T = R.softmax_bwd_terms(F64, p.detach(), dp, 0.125)
    R.assert_within(val, s.grad, AUTOGRAD_REL * T + 1e-300, "softmax vs autograd")


# ---- the restatement inside the bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", R.LN_C)
def test_layernorm_restatement_inside_bounds(Cc):
    """Every LN_CASES entry of this width (at C = 320 that includes M = 4081, 8161, 16321), every family."""
    worst = {}
    for case in [c for c in R.LN_CASES if c[1] == Cc]:
        for fam in R.FAMILIES:
            x, gamma, dy, ref = R.ln_fixture(case, fam)
            r32, b = R.ln_restated(case, fam), R.ln_bounds(ref)
            for n in ("dx", "dgamma", "dbeta"):
                worst[n] = max(worst.get(n, 0.0), R.assert_within(getattr(r32, n), getattr(ref, n), b[n], f"ln {case} {fam} {n}", quiet=True))
            if fam == "dyzero":
                assert all(float(getattr(r32, n).abs().max()) == 0.0 for n in ("dx", "dgamma", "dbeta"))
    print(f"ln C = {Cc}: restatement max err/bound {worst}")


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_id)
def test_groupnorm_restatement_inside_bounds(case, act):
    worst = {}
    for fam in R.FAMILIES:
        ref = R.gn_fixture(case, fam, act)[-1]
        r32, b = R.gn_restated(case, fam, act), R.gn_bounds(ref)
        for n in ("dx", "dgamma", "dbeta"):
            worst[n] = max(worst.get(n, 0.0), R.assert_within(getattr(r32, n), getattr(ref, n), b[n], f"gn {case} {fam} {n}", quiet=True))
        if fam == "dyzero":
            assert all(float(getattr(r32, n).abs().max()) == 0.0 for n in ("dx", "dgamma", "dbeta"))
    print(f"gn {case} act {act}: restatement max err/bound {worst}")


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.gn_id)
def test_saved_restatement_inside_bounds(case):
    route = R.gn_fwd_route(*case)
    assert (route == "three") == (case in R.FWD_THREE)
    for fam in R.FWD_FAMILIES:
        x1, x2, gamma, beta, sv = R.fwd_fixture(case, fam)
        s32, b = R.gn_saved_f32(x1, x2, gamma, beta, case[4], route=route), R.gn_saved_bounds(sv, gamma, beta)
        R.assert_within(s32.stats, sv.stats, b["stats"], f"saved stats {case} {fam} ({route})")
        R.assert_within(s32.scsh, sv.scsh, b["scsh"], f"saved scsh {case} {fam} ({route})")


def test_pointwise_restatement_inside_bounds():
    dy, z = R.act_inputs()
    for act in range(5):
        (v64, T), (v32, _) = R.act_bwd_terms(F64, dy, z, act), R.act_bwd_terms(F32, dy, z, act)
        R.assert_within(v32.to(F16), v64, R.pointwise_bound(v64, T, "act"), f"act {act}")
    for blk in (0, 32):
        d, hg = R.geglu_inputs()
        (v64, T), (v32, _) = R.geglu_bwd_terms(F64, d, hg, blk), R.geglu_bwd_terms(F32, d, hg, blk)
        R.assert_within(v32.to(F16), v64, R.pointwise_bound(v64, T, "geglu"), f"geglu blk {blk}")
    for case in R.SOFTMAX_CASES:
        p, dp = R.softmax_inputs(case)
        (v64, T), (v32, _) = R.softmax_bwd_terms(F64, p, dp, 0.125), R.softmax_bwd_terms(F32, p, dp, 0.125)
        R.assert_within(v32.to(F16), v64, R.pointwise_bound(v64, T, "softmax"), f"softmax {case}")


def test_constants_are_the_measured_ones():
    """K_MEASURED is the restatement's worst error over every case and family, re-measured here: not above the recorded figure (2 % for another
    CPU's exp / erf), and not more than a tenth below it -- a looser constant than the arithmetic needs would be a tolerance chosen by hand."""
    got = R.measure_constants()
    print({n: round(v, 4) for n, v in got.items()})
    for n, rec in R.K_MEASURED.items():
        assert 0.9 * rec <= got[n] <= 1.02 * rec, (n, got[n], rec)
        assert R.K[n] == R.MARGIN * rec


# ---- tightness: planted errors ------------------------------------------------------------------------------------------------------------------
GN_PLANT_CASES = [R.GN_CASES[1], R.GN_CASES[3], R.GN_CASES[7], R.GN_CASES[10]]


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
@pytest.mark.parametrize("case", GN_PLANT_CASES, ids=R.gn_id)
def test_a_dropped_slab_row_breaks_the_bounds(case, act):
    """rowmark: the last row of slab 0 left out of S1 / S2 takes a whole term out of dbeta, dgamma and the group means behind dx."""
    x1, x2, gamma, beta, dy, st, sc, sv, ref = R.gn_fixture(case, "rowmark", act)
    bad, b = R.gn_bwd_f32(x1, x2, gamma, dy, st, sc, case[4], act, plant="slab_last_row"), R.gn_bounds(ref)
    assert R.breaks(bad.dbeta, ref.dbeta, b["dbeta"]) and R.breaks(bad.dgamma, ref.dgamma, b["dgamma"]) and R.breaks(bad.dx, ref.dx, b["dx"])


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
@pytest.mark.parametrize("case", GN_PLANT_CASES, ids=R.gn_id)
def test_a_group_sum_one_channel_short_breaks_the_bounds(case, act):
    """chanmark: all of dy sits in each group's last channel, so T[0] / T[1] without it are zero."""
    x1, x2, gamma, beta, dy, st, sc, sv, ref = R.gn_fixture(case, "chanmark", act)
    bad, b = R.gn_bwd_f32(x1, x2, gamma, dy, st, sc, case[4], act, plant="group_last_channel"), R.gn_bounds(ref)
    assert R.breaks(bad.dx, ref.dx, b["dx"])
    assert not R.breaks(bad.dgamma, ref.dgamma, b["dgamma"]), "(dgamma does not go through T)"


@pytest.mark.parametrize("fam", ["gauss", "chanmark"])
def test_a_scaled_dgamma_channel_breaks_the_bounds(fam):
    """One channel of dgamma times 1 + 2^-9 (inside the suite's old 2e-3 bar) -- a group's last channel (LayerNorm: channel C - 1), the one
    chanmark keeps.  (Not offset: there S2 - mu S1 cancels sixteen-fold in the kernel's own f32 and the bound says so.)"""
    for case in GN_PLANT_CASES:
        x1, x2, gamma, beta, dy, st, sc, sv, ref = R.gn_fixture(case, fam, R.ACT_SILU)
        Cc, cpg = case[2] + case[3], (case[2] + case[3]) // case[4]
        assert float(ref.dgamma[Cc // 2 + cpg - 1]) != 0.0, "the planted channel carries a gradient"
        bad = R.gn_bwd_f32(x1, x2, gamma, dy, st, sc, case[4], R.ACT_SILU, plant="dgamma_scaled")
        assert R.breaks(bad.dgamma, ref.dgamma, R.gn_bounds(ref)["dgamma"]), (case, fam)
    for case in [(300, 320), (7, 1032), (4081, 320)]:
        x, gamma, dy, ref = R.ln_fixture(case, fam)
        assert float(ref.dgamma[case[1] - 1]) != 0.0, "the planted channel carries a gradient"
        bad = R.ln_bwd_f32(x, gamma, dy, plant="dgamma_scaled")
        assert R.breaks(bad.dgamma, ref.dgamma, R.ln_bounds(ref)["dgamma"]), (case, fam)


@pytest.mark.parametrize("case", [(7, 8), (300, 320), (7, 640), (3, 2048)], ids=R.ln_id)
def test_m1_over_c_plus_8_breaks_the_bounds(case):
    x, gamma, dy, ref = R.ln_fixture(case, "gauss")
    bad = R.ln_bwd_f32(x, gamma, dy, plant="m1_over_c_plus_8")
    assert R.breaks(bad.dx, ref.dx, R.ln_bounds(ref)["dx"])


@pytest.mark.parametrize("case", [(7, 8), (300, 320), (7, 640), (3, 2048)], ids=R.ln_id)
def test_dx_through_f16_twice_breaks_the_bounds(case):
    """gv - m1 - xh m2 rounded to f16 before the product with rstd is rounded again: up to a whole f16 ulp, twice what the store may cost."""
    x, gamma, dy, ref = R.ln_fixture(case, "gauss")
    bad = R.ln_bwd_f32(x, gamma, dy, plant="dx_twice_f16")
    assert R.breaks(bad.dx, ref.dx, R.ln_bounds(ref)["dx"])
