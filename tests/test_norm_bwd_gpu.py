"""-m gpu: gn_layernorm_bwd, gn_groupnorm_bwd (csrc/backward.hip), the stats / scsh the GroupNorm forward saves for it (csrc/norm.hip) and
act_bwd / geglu_bwd / softmax_bwd against the f64 references of tests/norm_bwd_ref.py, PER ELEMENT, at the bounds derived there:
  (a) the LayerNorm backward alone over LN_CASES x FAMILIES: NaN-filled dx, dgamma | dbeta accumulated onto prior contents, the dgamma = None
      route, add= (also aliasing dx) as bits, a second call bit-identical;
  (b) the GroupNorm backward alone over GN_CASES x {NONE, SILU} x FAMILIES, handed the f64 forward's stats / scsh (rounded to f32) through a
      GNSaved built here: NaN-filled outputs AND workspace, need_dx2 = False, add / add2 as bits, dgamma / dbeta over B onto prior contents, rerun;
  (c) what the forward saves, per element, on both of its routes (the route that ran is read off the workspace: only the three-launch path
      writes its partials there), then forward -> backward chained against the reference evaluated on THAT forward's saved values;
  (d) act_bwd (acts 0 - 4, |z| to 30, +-0), geglu_bwd (blk 0 / 32), softmax_bwd (8 .. 4096 columns, ld > cols with NaN pads that stay);
  (e) every argument refusal of gn_layernorm_bwd, gn_groupnorm_bwd and gn_softmax_bwd: an error, and nothing written.

Route -> case:
  layernorm_bwd_kernel<1, 4> / <2, 2> / <3, 1> / <4, 1>      C = 8, 320, 512 / 520, 640, 1024 / 1032, 1280, 1536 / 1544, 2048 (chunk edges on both sides)
  rows per block 8 / 16 / 32 / 64, one-row tail               M = 1 .. 300 / 4081 / 8161 / 16321 at C = 320
  last trip short of R rows, M < 4                            M = 1, 3, 7 (R = 4 at C <= 512, R = 2 at C <= 1024)
  part == nullptr; dx_add aliasing dx                         (a), gauss family of every case
  gnb_finalize idle threads: cpg = 10, 20, 30, 60, 80         (2,64,320,0,32) (3,64,640,0,32) (2,64,640,320,32) (2,64,1280,640,32) (2,64,1280,1280,32)
  L = 1 (cpg = 256); L = 32 (cpg = 8)                         (1,64,256,0,1); (2,64,64,0,8)
  gnb_partial TY = 6 with 16 idle threads                     (2,64,320,0,32)
  two cb passes (C = 2560)                                    (2,64,1280,1280,32)
  four-rows-in-flight loop and remainder, TY = 6 / TY = 32    (1,4096,320,0,32) / (1,6400,64,0,32)
  HW < 16; short last slab; p.chunks < chunks; 64 slabs       (1,9,64,0,32); (2,100,320,0,32); (1,1000,64,0,32); (1,1024,320,0,32)
  group straddling x | x2                                     (2,64,640,320,32)
  need_dx2 = False; B > 2; dgamma onto non-zero               (b) gauss family of the concat cases; (3,64,640,0,32); every case
  forward gn_fused_kernel / three-launch                      every GN case / (1,4096,512,0,32) (slab 128 KB) and (2,64,72,0,8) (odd cpg)

Largest err / bound measured on MI355X (printed with -s, summed up after the module's last test):
  (a) dx 0.9997, dgamma 0.926, dbeta 0.983      (b) dx 0.998, dgamma 0.526, dbeta 0.411      (d) act 0.998, geglu 0.998, softmax 1.0000 (rounded; below 1)
  (c) saved stats / scsh: fused 0.231 / 0.184, three-launch 0.224 / 0.224; the pair: dx 0.993 / 0.995, dgamma 0.038 / 0.033, dbeta 0.053 / 0.040
The f16 outputs sit just under 1 because half an f16 ulp IS reached (a tie of the store) and the f32 term beside it is ~1e-3 of the bound on
unit Gaussians (the CPU restatement of the same arithmetic reaches dx 0.9996 / 0.998 there); the f32 term alone, as the f32 outputs show, is
used to 0.03 .. 0.5 (the restatement: 0.25 by construction).  (a) dgamma / dbeta at 0.93 / 0.98 are M = 1 cases ((1, 1544), (1, 2048)), where
nearly all of the bound is the rounding of prior + sum.  No route came out above 1.
The module (181 tests) takes 18 s."""
import ctypes as C

import pytest
import torch

import norm_bwd_ref as R
from act_ops_ref import bits_equal
from genima_amd import train_ops as T
from genima_amd._lib import GenimaHipError, GroupNormDesc, check

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SENTINEL16, SENTINEL32 = 0x7BCD, 0x7F7FABCD  # finite bit patterns no result of these tests takes
WORST: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the largest err / bound per output (with -s), the figures of the docstring.  Every one of them was asserted <= 1 where
    it was measured (assert_within)."""
    yield
    for n in sorted(WORST):
        print(f"\n{n}: {WORST[n]:.6f}", end="")


def dev(t):
    return None if t is None else t.cuda()


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def ptr(t):
    return None if t is None else t.data_ptr()


def note(group: str, ratios: dict):
    for n, r in ratios.items():
        WORST[f"{group} {n}"] = max(WORST.get(f"{group} {n}", 0.0), r)


def prior_for(Cc: int, seed: int):
    """Non-zero prior contents of a dgamma | dbeta pair: one contiguous f32 [2, C] buffer (the flat gradient buffer's layout)."""
    return torch.randn(2, Cc, generator=torch.Generator().manual_seed(seed)) * 3


def nan_workspace(engine, nbytes: int):
    ws = engine._workspace(int(nbytes))
    ws.fill_(float("nan"))
    return ws


# ---- (a) LayerNorm backward alone ------------------------------------------------------------------------------------------------------------
def raw_ln(engine, x, gamma, dy, dx, dgamma, dbeta, M, Cc, add=None, workspace=True):
    ws = nan_workspace(engine, engine.lib.gn_layernorm_bwd_workspace_bytes(M, Cc)) if workspace else None
    return engine.lib.gn_layernorm_bwd(engine._ctx, ptr(x), ptr(gamma), ptr(dy), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), M, Cc, R.EPS, ptr(add))


@pytest.mark.parametrize("case", R.LN_CASES, ids=R.ln_id)
def test_layernorm_backward_alone(engine, case):
    M, Cc = case
    ratios = {}
    for fam in R.FAMILIES:
        x, gamma, dy, ref = R.ln_fixture(case, fam)
        xd, gd, dd = dev(x), dev(gamma), dev(dy)
        prior = prior_for(Cc, M + Cc)
        dgb, dx = dev(prior), nan16(M, Cc)
        check(raw_ln(engine, xd, gd, dd, dx, dgb[0], dgb[1], M, Cc), "gn_layernorm_bwd")
        b = R.ln_bounds(ref, prior)
        for n, got, want in (("dx", dx, ref.dx), ("dgamma", dgb[0], ref.dgamma + prior[0]), ("dbeta", dgb[1], ref.dbeta + prior[1])):
            ratios[n] = max(ratios.get(n, 0.0), R.assert_within(got, want, b[n], f"ln {case} {fam} {n}"))
        if fam == "dyzero":
            assert float(dx.abs().max()) == 0.0 and bits_equal(dgb, prior), "dy = 0: exact zeros, prior contents untouched in value"
        dgb2, dx2 = dev(prior), nan16(M, Cc)
        check(raw_ln(engine, xd, gd, dd, dx2, dgb2[0], dgb2[1], M, Cc), "gn_layernorm_bwd")
        assert bits_equal(dx, dx2) and bits_equal(dgb, dgb2), "a second call is bit-identical"
        if fam != "gauss":
            continue
        dx3 = nan16(M, Cc)  # dgamma == NULL: part == nullptr, no workspace
        check(raw_ln(engine, xd, gd, dd, dx3, None, None, M, Cc, workspace=False), "gn_layernorm_bwd")
        assert bits_equal(dx, dx3), "dx does not depend on whether dgamma is asked for"
        held = dev(torch.randn(M, Cc, generator=torch.Generator().manual_seed(5)).to(F16))
        want = (dx.float() + held.float()).half()
        assert bits_equal(T.layernorm_bwd(engine, xd, gd, dd, add=held), want), "add=: f16(f32(dx) + f32(held))"
        buf = held.clone()  # add aliasing the output, through the raw entry point
        check(raw_ln(engine, xd, gd, dd, buf, None, None, M, Cc, add=buf, workspace=False), "gn_layernorm_bwd")
        assert bits_equal(buf, want), "add aliasing dx"
    note("(a) ln", ratios)


# ---- (b) GroupNorm backward alone ------------------------------------------------------------------------------------------------------------
def saved_from(case, act, x1, x2, gamma, beta, stats, scsh):
    """A GNSaved as train_ops.groupnorm_fwd_train leaves it, from tensors of the test's own (never the forward kernel's)."""
    B, HW, C1, C2, G = case
    s = T.GNSaved()
    s.x, s.x2, s.gamma, s.beta, s.stats, s.scsh = x1, x2, gamma, beta, stats, scsh
    d = GroupNormDesc()
    d.x, d.x2, d.gamma, d.beta = ptr(x1), ptr(x2), ptr(gamma), ptr(beta)
    d.B, d.HW, d.C1, d.C2, d.groups, d.act, d.eps = B, HW, C1, C2, G, act, R.EPS
    s.desc = d
    return s


def raw_gn(engine, s, dy, dx, dx2, dgamma, dbeta, add=None, add2=None):
    d = s.desc
    ws = nan_workspace(engine, engine.lib.gn_groupnorm_bwd_workspace_bytes(d.B, d.HW, d.C1 + d.C2))
    return engine.lib.gn_groupnorm_bwd(engine._ctx, C.byref(d), ptr(dy), ptr(dx), ptr(dx2), ptr(s.scsh), ptr(s.stats), ptr(dgamma), ptr(dbeta),
                                       ptr(ws), ptr(add), ptr(add2))


def run_gn(engine, s, dy, prior):
    """NaN-filled dx / dx2 and workspace, dgamma | dbeta starting from ``prior`` -> (dx1 | dx2 [B, HW, C], dgb [2, C]) on the device."""
    dx = nan16(*s.x.shape)
    dx2 = nan16(*s.x2.shape) if s.x2 is not None else None
    dgb = dev(prior)
    check(raw_gn(engine, s, dy, dx, dx2, dgb[0], dgb[1]), "gn_groupnorm_bwd")
    return (torch.cat([dx, dx2], -1) if dx2 is not None else dx), dgb


def check_gn(got_dx, dgb, ref, prior, what) -> dict:
    b = R.gn_bounds(ref, prior)
    return {n: R.assert_within(got, want, b[n], f"{what} {n}")
            for n, got, want in (("dx", got_dx, ref.dx), ("dgamma", dgb[0], ref.dgamma + prior[0]), ("dbeta", dgb[1], ref.dbeta + prior[1]))}


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_id)
def test_groupnorm_backward_alone(engine, case, act):
    B, HW, C1, C2, G = case
    Cc = C1 + C2
    ratios = {}
    for fam in R.FAMILIES:
        x1, x2, gamma, beta, dy, st, sc, sv, ref = R.gn_fixture(case, fam, act)
        s = saved_from(case, act, dev(x1), dev(x2), dev(gamma), dev(beta), dev(st), dev(sc))
        dd, prior = dev(dy), prior_for(Cc, HW + Cc)
        dx, dgb = run_gn(engine, s, dd, prior)
        for n, r in check_gn(dx, dgb, ref, prior, f"gn {case} act {act} {fam}").items():
            ratios[n] = max(ratios.get(n, 0.0), r)
        if fam == "dyzero":
            assert float(dx.abs().max()) == 0.0 and bits_equal(dgb, prior), "dy = 0: exact zeros"
        dx_b, dgb_b = run_gn(engine, s, dd, prior)
        assert bits_equal(dx, dx_b) and bits_equal(dgb, dgb_b), "a rerun is bit-identical"
        if fam != "gauss":
            continue
        # need_dx2 = False (the `if (!dst) return` path), no parameter gradients: dx1 the same bits
        only1, none2 = T.groupnorm_bwd(engine, s, dd, need_dx2=False)
        assert none2 is None and bits_equal(only1, dx[..., :C1]), "dx1 does not depend on dx2 being asked for"
        if C2:
            none1, only2 = T.groupnorm_bwd(engine, s, dd, need_dx=False)
            assert none1 is None and bits_equal(only2, dx[..., C1:])
        g = torch.Generator().manual_seed(6)
        held1 = dev(torch.randn(B, HW, C1, generator=g).to(F16))
        held2 = dev(torch.randn(B, HW, C2, generator=g).to(F16)) if C2 else None
        a1, a2 = T.groupnorm_bwd(engine, s, dd, add=held1, add2=held2)
        assert bits_equal(a1, (dx[..., :C1].float() + held1.float()).half()), "add: f16(f32(dx1) + f32(held))"
        if C2:
            assert bits_equal(a2, (dx[..., C1:].float() + held2.float()).half()), "add2"
        b1, b2 = held1.clone(), (held2.clone() if C2 else None)  # add / add2 aliasing the outputs
        check(raw_gn(engine, s, dd, b1, b2, None, None, add=b1, add2=b2), "gn_groupnorm_bwd")
        assert bits_equal(b1, a1) and (not C2 or bits_equal(b2, a2)), "add aliasing dx"
    note("(b) gn", ratios)


# ---- (c) what the forward saves; the pair ---------------------------------------------------------------------------------------------------------
def forward_train(engine, case, act, x1, x2, gamma, beta):
    """train_ops.groupnorm_fwd_train with the shared workspace NaN-filled beforehand -> (y, saved, the route that ran).  gn_fused_kernel never
    touches the workspace; the three-launch path writes its per-slab partials at its start."""
    B, HW, C1, C2, G = case
    ws = nan_workspace(engine, 1 << 22)
    y, s = T.groupnorm_fwd_train(engine, dev(x1), dev(gamma), dev(beta), G, R.EPS, act, x2=dev(x2))
    assert engine._workspace(1 << 22).data_ptr() == ws.data_ptr()
    slabs = R.gn_pick_chunks(B, HW)
    route = "fused" if bool(torch.isnan(ws[:B * slabs * G * 2]).all()) else "three"
    return y, s, route


@pytest.mark.parametrize("fam", R.FWD_FAMILIES)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.gn_id)
def test_forward_saved_values(engine, case, fam):
    """stats = (mean, rstd) and scsh = (rstd gamma, beta - mean rstd gamma) per element against f64, on the route gn_launch_groupnorm's rule
    gives the case: slab HW cpg 2 against GNF_MAX_LDS, B groups >= 64 or a small tensor, an even cpg."""
    x1, x2, gamma, beta, sv = R.fwd_fixture(case, fam)
    y, s, route = forward_train(engine, case, R.ACT_SILU, x1, x2, gamma, beta)
    print(f"forward {case} {fam}: route {route}")
    assert route == R.gn_fwd_route(*case) == ("three" if case in R.FWD_THREE else "fused")
    b = R.gn_saved_bounds(sv, gamma, beta)
    note(f"(c) saved, {route}", {"stats": R.assert_within(s.stats, sv.stats, b["stats"], f"saved stats {case} {fam} ({route})"),
                                 "scsh": R.assert_within(s.scsh, sv.scsh, b["scsh"], f"saved scsh {case} {fam} ({route})")})


PAIR_CASES = [R.GN_CASES[3], R.GN_CASES[7], R.FWD_THREE[0], R.FWD_THREE[1]]


@pytest.mark.parametrize("fam", ["gauss", "offset"])
@pytest.mark.parametrize("case", PAIR_CASES, ids=R.gn_id)
def test_forward_feeds_backward(engine, case, fam):
    """Each forward route's own stats / scsh into the backward, against gn_bwd_ref evaluated ON THOSE at the bounds of (b): a failure here
    with (c) passing is the backward's, a failure of (c) is the forward's."""
    B, HW, C1, C2, G = case
    x1, x2, gamma, beta, dy = R.gn_inputs(case, fam, seed=4)
    y, s, route = forward_train(engine, case, R.ACT_SILU, x1, x2, gamma, beta)
    assert route == R.gn_fwd_route(*case)
    prior = prior_for(C1 + C2, 9)
    dgb = dev(prior)
    dx1, dx2 = T.groupnorm_bwd(engine, s, dev(dy), dgamma=dgb[0], dbeta=dgb[1])
    ref = R.gn_bwd_ref(x1, x2, gamma, dy, s.stats.cpu(), s.scsh.cpu(), G, R.ACT_SILU)
    note(f"(c) pair, {route}", check_gn(torch.cat([dx1, dx2], -1) if C2 else dx1, dgb, ref, prior, f"pair {case} {fam} ({route})"))


# ---- (d) pointwise ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", range(5))
def test_act_bwd(engine, act):
    dy, z = R.act_inputs()
    ref, Tm = R.act_bwd_terms(F64, dy, z, act)
    got = T.act_bwd(engine, dev(dy), dev(z), act)
    if act in (R.ACT_NONE, R.ACT_RELU):  # dy or (signed) zero, exactly
        assert bits_equal(got, ref.to(F16))
    else:
        note("(d)", {"act_bwd": R.assert_within(got, ref, R.pointwise_bound(ref, Tm, "act"), f"act_bwd {act}")})


@pytest.mark.parametrize("blk", [0, 32])
def test_geglu_bwd(engine, blk):
    dy, hg = R.geglu_inputs()
    ref, Tm = R.geglu_bwd_terms(F64, dy, hg, blk)
    got = T.geglu_bwd(engine, dev(dy), dev(hg), blk)
    note("(d)", {"geglu_bwd": R.assert_within(got, ref, R.pointwise_bound(ref, Tm, "geglu"), f"geglu_bwd blk {blk}")})


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_softmax_bwd(engine, case, pad):
    rows, cols = case
    p, dp = R.softmax_inputs(case)
    ref, Tm = R.softmax_bwd_terms(F64, p, dp, 0.125)
    pb, db = nan16(rows, cols + pad), nan16(rows, cols + pad)
    pb[:, :cols], db[:, :cols] = dev(p), dev(dp)
    T.softmax_bwd(engine, pb[:, :cols], db[:, :cols], 0.125)
    note("(d)", {"softmax_bwd": R.assert_within(db[:, :cols], ref, R.pointwise_bound(ref, Tm, "softmax"), f"softmax_bwd {case} ld {cols + pad}")})
    assert bool(torch.isnan(db[:, cols:]).all()), "the pad columns keep their NaN"


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------------
def sent16(*shape):
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device="cuda").view(F16)


def sent32(*shape):
    return torch.full(shape, SENTINEL32, dtype=torch.int32, device="cuda").view(F32)


LN_REFUSALS = ["C = 2056", "C % 8", "M = 0", "null x", "dgamma without dbeta", "dbeta without dgamma", "dgamma | dbeta not contiguous", "no workspace"]


@pytest.mark.parametrize("what", LN_REFUSALS)
def test_layernorm_bwd_refusals(engine, what):
    """Every GN_REQUIRE of gn_layernorm_bwd returns an error before anything is launched: dx and dgamma | dbeta keep their sentinel.  (The
    buffers are sized for the largest shape named, whatever is refused.)"""
    M, Cc = 16, 320
    big = 2056
    x, dy = (torch.zeros(M, big, dtype=F16, device="cuda") for _ in range(2))
    gamma = torch.ones(big, dtype=F16, device="cuda")
    dx, dgb = sent16(M, big), sent32(3, big)
    a = dict(x=x, gamma=gamma, dy=dy, dx=dx, dgamma=dgb[0], dbeta=dgb[0, Cc:], M=M, Cc=Cc, workspace=True)  # dbeta == dgamma + C
    if what == "C = 2056":
        a.update(Cc=big, dbeta=dgb[1])
    elif what == "C % 8":
        a.update(Cc=316, dbeta=dgb[0, 316:])
    elif what == "M = 0":
        a.update(M=0)
    elif what == "null x":
        a.update(x=None)
    elif what == "dgamma without dbeta":
        a.update(dbeta=None)
    elif what == "dbeta without dgamma":
        a.update(dgamma=None)
    elif what == "dgamma | dbeta not contiguous":
        a.update(dbeta=dgb[1])
    elif what == "no workspace":
        a.update(workspace=False)
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_layernorm_bwd"):
        check(raw_ln(engine, **a), "gn_layernorm_bwd")
    engine.synchronize()
    assert bool((dx.view(torch.int16) == SENTINEL16).all()) and bool((dgb.view(torch.int32) == SENTINEL32).all()), f"{what}: an output was written"


GN_REFUSALS = ["null dy", "null stats", "neither dx nor dx2", "C1 % 8", "C > 4096", "groups = 0", "C % groups", "cpg > 256", "dgamma without dbeta",
               "dbeta without dgamma", "C2 without x2", "HW = 0"]


@pytest.mark.parametrize("what", GN_REFUSALS)
def test_groupnorm_bwd_refusals(engine, what):
    """Every GN_REQUIRE of gn_groupnorm_bwd, the channels-per-group checks included, comes before the first launch: outputs and the
    workspace's partials keep their sentinel / NaN."""
    B, HW, C1, C2, G = 1, 16, 512, 0, 32
    big = 4104
    x1, dy = (torch.zeros(B, HW, big, dtype=F16, device="cuda") for _ in range(2))
    gamma, beta = torch.ones(big, dtype=F16, device="cuda"), torch.zeros(big, dtype=F16, device="cuda")
    stats, scsh = torch.ones(B, big, 2, dtype=F32, device="cuda"), torch.ones(B, big, 2, dtype=F32, device="cuda")
    dx, dx2, dgb = sent16(B, HW, big), sent16(B, HW, big), sent32(2, big)
    over = {"C1 % 8": dict(C1=508, C2=4), "C > 4096": dict(C1=big, G=513), "groups = 0": dict(G=0), "C % groups": dict(G=24), "cpg > 256": dict(G=1),
            "C2 without x2": dict(C2=64), "HW = 0": dict(HW=0)}.get(what, {})
    c = dict(B=B, HW=HW, C1=C1, C2=C2, G=G)
    c.update(over)
    s = saved_from((c["B"], c["HW"], c["C1"], c["C2"], c["G"]), R.ACT_SILU, x1, x1 if what == "C1 % 8" else None, gamma, beta,
                   None if what == "null stats" else stats, scsh)
    a = dict(dy=None if what == "null dy" else dy, dx=dx, dx2=None, dgamma=dgb[0], dbeta=dgb[1])
    if what == "neither dx nor dx2":
        a.update(dx=None)
    elif what == "dgamma without dbeta":
        a.update(dbeta=None)
    elif what == "dbeta without dgamma":
        a.update(dgamma=None)
    ws = nan_workspace(engine, engine.lib.gn_groupnorm_bwd_workspace_bytes(B, HW, big))
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_groupnorm_bwd"):
        check(engine.lib.gn_groupnorm_bwd(engine._ctx, C.byref(s.desc), ptr(a["dy"]), ptr(a["dx"]), ptr(a["dx2"]), ptr(s.scsh), ptr(s.stats),
                                          ptr(a["dgamma"]), ptr(a["dbeta"]), ptr(ws), None, None), "gn_groupnorm_bwd")
    engine.synchronize()
    assert bool((dx.view(torch.int16) == SENTINEL16).all()) and bool((dgb.view(torch.int32) == SENTINEL32).all()), f"{what}: an output was written"
    assert bool(torch.isnan(ws).all()), f"{what}: a kernel ran (the workspace was written)"


@pytest.mark.parametrize("what", ["cols = 4104", "cols % 8", "ld % 8", "rows = 0", "cols = 0", "null p"])
def test_softmax_bwd_refusals(engine, what):
    rows, cols, ld = 4, 256, 256
    p, dp = torch.zeros(8, 4104, dtype=F16, device="cuda"), sent16(8, 4104)
    a = {"cols = 4104": (rows, 4104, 4104), "cols % 8": (rows, 252, 256), "ld % 8": (rows, 256, 260), "rows = 0": (0, cols, ld), "cols = 0": (rows, 0, ld)}.get(what, (rows, cols, ld))
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_softmax_bwd"):
        check(engine.lib.gn_softmax_bwd(engine._ctx, None if what == "null p" else ptr(p), ptr(dp), a[0], a[1], a[2], 0.125), "gn_softmax_bwd")
    engine.synchronize()
    assert bool((dp.view(torch.int16) == SENTINEL16).all()), f"{what}: dp was written"
