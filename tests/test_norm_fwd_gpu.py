"""-m gpu: gn_layernorm_fwd, gn_groupnorm_fwd on each of its routes (csrc/norm.hip) and gn_softmax_rows / gn_softmax_rows_masked
(csrc/elementwise.hip) against the f64 references of tests/norm_fwd_ref.py, PER ELEMENT, at the bounds derived there:
  (a) gn_layernorm_fwd over LN_CASES x FAMILIES: NaN-filled y with a NaN guard region behind it, a second call bit-identical, the recorded form
      (gn_program_add_layernorm, replayed) the same bits for one case per (CH, ROWS);
  (b) gn_groupnorm_fwd over GN_CASES x {NONE, SILU} x FAMILIES: NaN-filled y AND workspace; the route that ran is read off the workspace (only the
      three-launch path writes its partials there) and must be the one gn_fwd_route gives; inference (nothing saved) and training (save_stats +
      save_scsh) give the same y bits on the same route; rerun; the recorded form (gn_program_add_groupnorm);
  (c) stats_in: y against the reference evaluated from the handed integer totals, the block bit-unchanged, the replicas permuted -> the same bits;
  (d) statistics only (y == NULL): stats / scsh at the three-launch bounds, sentinel-filled neighbours untouched, and an ordinary three-launch
      call of the same input writes the same scsh bits and a y that is act(x a + s) of exactly those;
  (e) gn_softmax_rows / gn_softmax_rows_masked: every element, exact zeros at columns >= valid, NaN pad columns untouched, the row sum of the
      stored values within cols 2^-11 of 1;
  (f) every argument refusal of the three entry points: an error, and nothing written.  valid <= 0 and valid > cols are refused by
      gn_softmax_rows_masked (its caller, training.py's cross-attention backward, always has valid >= 1): pinned here, no NaN rows.

Route -> case:
  layernorm_kernel<1, 1> / <1, 2> / <1, 4>            C = 8, 320, 512 at M = 1, 3, 5 and (2047, 320) / (2048, 320) .. (8191, 320) / (8192, 320), (8193, 320), (8195, 64)
  layernorm_kernel<2, 1> / <2, 2>                     C = 520, 1024 at M = 1, 3, 5 and (4095, 520) / (4096, 520), (4097, 520)
  layernorm_kernel<4, 1> / <8, 1>                     C = 1032, 2048 / C = 2056, 4096 at M = 1, 3, 5
  dispatch thresholds, both sides                     M = 2047 | 2048, 8191 | 8192 at C = 320; M = 4095 | 4096 at C = 520
  last wave with dead rows (live of ROWS)             (2049, 320) 1 of 2; (8193, 320) 1 of 4; (8195, 64) 3 of 4; (4097, 520) 1 of 2
  C = 512 k + 8: lanes >= CC of the last chunk        C = 520, 1032, 2056
  gn_fused_kernel                                     norm_bwd_ref.GN_CASES (cpg 2 .. 256, concat with a straddling group, HW 9 .. 6400)
  three-launch: slab > 96 KB; odd cpg                 (1,4096,512,0,32); (2,64,72,0,8)
  three-launch: CC = 320 > 256 (cx += TX loops)       (1,1024,2560,0,32)
  three-launch: group 20 straddling x | x2            (1,4096,328,184,32)
  three-launch: ragged apply slab                     (1,4100,512,0,32)
  stats_in: cpg 2, 4, 10, 12, 20, 30, 80, 256         SI_CASES, each cpg at HW 9, 64, 1000 with 1, 3 and 9 replicas between them (cpg 12, 10, 20, 30:
                                                      a chunk's 8 channels in two groups; cpg 2, 4: in four / two); concat (2,64,640,320,32) r9
  statistics only                                     (2,64,320,0,32) (fused-eligible); (2,64,72,0,8)
  masked softmax, valid = 1                           every softmax case (cols 8 .. 4096, rows 1, 5, 33)

Largest err / bound measured on MI355X (printed with -s, summed up after the module's last test):
  (a) y: <1, 1> 0.9978, <1, 2> 0.9977, <1, 4> 0.9979, <2, 1> 0.9976, <2, 2> 0.9977, <4, 1> 0.9971, <8, 1> 0.9975
  (b) y: fused 0.9971, three-launch 0.9972        (c) stats_in y 0.9988        (e) softmax y 0.99992
  (d) statistics only: stats 0.224, scsh 0.224 (the CPU restatement of the same sums: 0.224, lowvar (2, 64, 72, 0, 8)); apply from that scsh 0.9987
The f16 outputs sit just under 1 because half an f16 ulp IS reached (a tie of the store) and the f32 term beside it is 1e-2 .. 1e-3 of the bound
on unit Gaussians -- the CPU restatement of the same arithmetic reaches 0.997 there as well; the f32 term alone, as the f32 outputs of (d) show,
is used to 0.22 (the restatement: 0.25 by construction).  On the offset and lowvar families the GroupNorm bound is mostly |x| b_a + b_sh, what
the f32 statistics of such inputs may cost (norm_bwd_ref.gn_saved_bounds), and y uses 0.03 .. 0.13 and < 0.001 of it: those two families pin
the statistics' share, gauss and tailmark the apply step's.  No route came out above 1, and no kernel was changed for one.
The module (153 tests) takes 19 s.
"""
import ctypes as C
import time

import pytest
import torch

import norm_fwd_ref as R
from act_ops_ref import bits_equal
from genima_amd._lib import GenimaHipError, GroupNormDesc, check
from genima_amd.engine import Engine

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
SENTINEL16, SENTINEL32 = 0x7BCD, 0x7F7FABCD  # finite bit patterns no result of these tests takes
GUARD = 4096
ACTS = (R.ACT_NONE, R.ACT_SILU)
WORST: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the largest err / bound per output and route (with -s), the figures of the docstring.  Every one of them was asserted
    <= 1 where it was measured (assert_within)."""
    t0 = time.time()
    yield
    for n in sorted(WORST):
        print(f"\n{n}: {WORST[n]:.6f}", end="")
    print(f"\nmodule wall time {time.time() - t0:.1f} s")


def dev(t):
    return None if t is None else t.cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def guarded(*shape):
    """-> (the whole NaN-filled buffer, its leading view of ``shape``): GUARD elements behind the view must stay NaN."""
    n = 1
    for s in shape:
        n *= s
    buf = nan16(n + GUARD)
    return buf, buf[:n].view(shape)


def guard_intact(buf) -> bool:
    return bool(torch.isnan(buf[-GUARD:]).all())


def sent16(*shape):
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device="cuda").view(F16)


def sent32(*shape):
    return torch.full(shape, SENTINEL32, dtype=torch.int32, device="cuda").view(F32)


def note(name: str, ratio: float):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


# ---- (a) LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def raw_ln(engine, x, gamma, beta, y, M, Cc):
    return engine.lib.gn_layernorm_fwd(engine._ctx, x, gamma, beta, y, M, Cc, R.EPS)


def run_ln(engine, xd, gd, bd, M, Cc):
    buf, y = guarded(M, Cc)
    check(raw_ln(engine, ptr(xd), ptr(gd), ptr(bd), ptr(y), M, Cc), "gn_layernorm_fwd")
    engine.synchronize()
    assert guard_intact(buf), "written past y"
    return y


@pytest.mark.parametrize("case", R.LN_CASES, ids=R.ln_id)
def test_layernorm_forward(engine, case):
    M, Cc = case
    route = R.ln_fwd_route(M, Cc)
    for fam in R.FAMILIES:
        x, gamma, beta, ref, bound = R.ln_fixture(case, fam)
        xd, gd, bd = dev(x), dev(gamma), dev(beta)
        y = run_ln(engine, xd, gd, bd, M, Cc)
        note(f"(a) ln y <{route[0]}, {route[1]}>", R.assert_within(y, ref.y, bound, f"ln {case} {fam} <{route[0]}, {route[1]}>"))
        assert bits_equal(y, run_ln(engine, xd, gd, bd, M, Cc)), "a second call is bit-identical"


def test_layernorm_recorded_form(engine):
    """gn_program_add_layernorm, replayed: the same bits as the eager call, one case per layernorm_kernel instantiation."""
    ER = Engine("cuda:0", record=True, autotune=False)
    pairs = []
    for route in R.LN_ROUTES:
        case = next(c for c in R.LN_CASES if R.ln_fwd_route(*c) == route and c[0] > 1)
        x, gamma, beta, _, _ = R.ln_fixture(case, "gauss")
        xd, gd, bd = dev(x), dev(gamma), dev(beta)
        out = nan16(*case)
        ER.layernorm(xd, gd, bd, R.EPS, out=out)
        pairs.append((case, run_ln(engine, xd, gd, bd, *case), out))
    ER.run()
    ER.synchronize()
    for case, eager, out in pairs:
        assert bits_equal(eager, out), f"recorded layernorm {case}"


# ---- (b) GroupNorm on the fused and the three-launch route ------------------------------------------------------------------------------------------
def gn_desc(case, act, x1, x2, gamma, beta, y, ws, save_stats=None, save_scsh=None, stats_in=None, reps=0):
    B, HW, C1, C2, G = case[:5]
    d = GroupNormDesc()
    d.x, d.x2, d.gamma, d.beta, d.y, d.workspace = ptr(x1), ptr(x2), ptr(gamma), ptr(beta), ptr(y), ptr(ws)
    d.B, d.HW, d.C1, d.C2, d.groups, d.act, d.eps = B, HW, C1, C2, G, act, R.EPS
    d.save_stats, d.save_scsh, d.stats_in, d.stats_replicas = ptr(save_stats), ptr(save_scsh), ptr(stats_in), reps
    return d


def nan_workspace(engine, case):
    """The engine's shared workspace, NaN-filled over what gn_groupnorm_workspace_bytes asks for this case -> (the buffer, that many floats)."""
    B, HW, C1, C2, G = case[:5]
    d = GroupNormDesc()
    d.B, d.HW, d.C1, d.C2, d.groups = B, HW, C1, C2, G
    n = int(engine.lib.gn_groupnorm_workspace_bytes(C.byref(d))) // 4
    ws = engine._workspace(4 * n)
    ws[:n].fill_(float("nan"))
    return ws, n


def route_of(ws, case) -> str:
    """gn_fused_kernel never touches the workspace; the three-launch path writes its per-slab partials at its start."""
    B, HW, _, _, G = case[:5]
    return "fused" if bool(torch.isnan(ws[:B * R.gn_pick_chunks(B, HW) * G * 2]).all()) else "three"


def run_gn(engine, case, act, t, train=False, stats_in=None):
    """t = device (x1, x2, gamma, beta).  NaN-filled y (guarded) and workspace -> (y, stats, scsh, route)."""
    B, HW, C1, C2, G = case[:5]
    buf, y = guarded(B, HW, C1 + C2)
    ws, n = nan_workspace(engine, case)
    stats = sent32(B, G, 2) if train else None
    scsh = sent32(B, C1 + C2, 2) if train else None
    d = gn_desc(case, act, *t, y, ws, stats, scsh, stats_in, 0 if stats_in is None else int(stats_in.shape[0]))
    check(engine.lib.gn_groupnorm_fwd(engine._ctx, C.byref(d)), "gn_groupnorm_fwd")
    engine.synchronize()
    assert guard_intact(buf), "written past y"
    route = route_of(ws, case)
    if stats_in is not None:
        assert bool(torch.isnan(ws[:n]).all()), "stats_in: one apply launch, the workspace is not used"
    return y, stats, scsh, route


@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_id)
def test_groupnorm_forward(engine, case):
    want_route = R.gn_fwd_route(*case)
    assert want_route == R.GN_ROUTE[case]
    for fam in R.FAMILIES:
        x1, x2, gamma, beta, sv = R.gn_fixture(case, fam)
        t = (dev(x1), dev(x2), dev(gamma), dev(beta))
        for act in ACTS:
            ref, bound = R.gn_fwd_bound(x1, x2, gamma, beta, sv, act)
            y, _, _, route = run_gn(engine, case, act, t)
            print(f"groupnorm {case} {fam} act {act}: route {route}")
            assert route == want_route
            note(f"(b) gn y {route}", R.assert_within(y, ref, bound, f"gn {case} {fam} act {act} ({route})"))
            y_t, stats, scsh, route_t = run_gn(engine, case, act, t, train=True)
            assert route_t == route and bits_equal(y_t, y), "training mode (save_stats + save_scsh): the same route, the same y bits"
            assert not bool((stats.view(torch.int32) == SENTINEL32).any()) and not bool((scsh.view(torch.int32) == SENTINEL32).any())
            assert bits_equal(run_gn(engine, case, act, t)[0], y), "a rerun is bit-identical"


def test_groupnorm_recorded_form(engine):
    """gn_program_add_groupnorm, replayed: the same bits as the eager call -- a fused case, a concatenated one, two three-launch ones."""
    ER = Engine("cuda:0", record=True, autotune=False)
    pairs = []
    for case in (R.GN_CASES[1], R.GN_CASES[3], R.FWD_THREE[1], R.GN_THREE_MORE[1]):
        B, HW, C1, C2, G = case
        x1, x2, gamma, beta, _ = R.gn_fixture(case, "gauss")
        t = (dev(x1), dev(x2), dev(gamma), dev(beta))
        out = nan16(B, HW, C1 + C2)
        ER.groupnorm(t[0], t[2], t[3], G, R.EPS, act=R.ACT_SILU, x2=t[1], out=out)
        pairs.append((case, run_gn(engine, case, R.ACT_SILU, t)[0], out))
    ER.run()
    ER.synchronize()
    for case, eager, out in pairs:
        assert bits_equal(eager, out), f"recorded groupnorm {case}"


# ---- (c) GroupNorm from bridge statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SI_CASES, ids=R.si_id)
def test_groupnorm_from_bridge_statistics(engine, case):
    reps = case[5]
    for fam in R.FAMILIES:
        x, x1, x2, gamma, beta, blk = R.si_fixture(case, fam)
        t = (dev(x1), dev(x2), dev(gamma), dev(beta))
        bd = blk.cuda()
        perm = torch.randperm(reps, generator=torch.Generator().manual_seed(reps))
        bp = blk[perm].contiguous().cuda()
        for act in ACTS:
            ref, bound = R.stats_in_bound(x, gamma, beta, R._gn_stats_in(F64, x, gamma, beta, blk, case[4], act), act)
            y, _, _, _ = run_gn(engine, case, act, t, stats_in=bd)
            note("(c) stats_in y", R.assert_within(y, ref, bound, f"stats_in {case} {fam} act {act}"))
            assert torch.equal(bd.cpu(), blk), "the statistics block is bit-unchanged"
            assert bits_equal(run_gn(engine, case, act, t, stats_in=bp)[0], y), "which replica holds which part does not change a bit"


# ---- (d) statistics only --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.STATS_ONLY_CASES, ids=R.gn_id)
def test_statistics_only(engine, case):
    B, HW, C1, C2, G = case
    Cc = C1 + C2
    n_st, n_sc, pad = B * G * 2, B * Cc * 2, 64
    for fam in R.FAMILIES:
        x1, x2, gamma, beta, sv = R.gn_fixture(case, fam)
        t = (dev(x1), dev(x2), dev(gamma), dev(beta))
        area = sent32(pad + n_st + pad + n_sc + pad)  # guard | stats | guard | scsh | guard
        stats, scsh = area[pad:pad + n_st].view(B, G, 2), area[2 * pad + n_st:2 * pad + n_st + n_sc].view(B, Cc, 2)
        ws, n = nan_workspace(engine, case)
        d = gn_desc(case, R.ACT_SILU, *t, None, ws, stats, scsh)
        check(engine.lib.gn_groupnorm_fwd(engine._ctx, C.byref(d)), "gn_groupnorm_fwd")
        engine.synchronize()
        assert route_of(ws, case) == "three", "the statistics-only call takes the three-launch statistics whatever the shape"
        b = R.gn_saved_bounds(sv, gamma, beta)
        note("(d) stats-only stats", R.assert_within(stats, sv.stats, b["stats"], f"stats-only stats {case} {fam}"))
        note("(d) stats-only scsh", R.assert_within(scsh, sv.scsh, b["scsh"], f"stats-only scsh {case} {fam}"))
        ai = area.view(torch.int32)
        for lo, hi in ((0, pad), (pad + n_st, 2 * pad + n_st), (2 * pad + n_st + n_sc, 3 * pad + n_st + n_sc)):
            assert bool((ai[lo:hi] == SENTINEL32).all()), "written outside stats / scsh"
        if R.gn_fwd_route(*case) != "three":
            continue
        for act in ACTS:  # an ordinary three-launch call of the same input: the same scsh, and gn_apply_kernel's y is act(x a + s) of exactly those
            y, stats_t, scsh_t, route = run_gn(engine, case, act, t, train=True)
            assert route == "three" and bits_equal(scsh_t, scsh.contiguous()) and bits_equal(stats_t, stats.contiguous())
            a32, s32 = scsh_t[..., 0].cpu(), scsh_t[..., 1].cpu()
            zero = torch.zeros(B, Cc, dtype=F64)
            ref, bound = R.apply_bound(R._cat(x1, x2), a32, s32, zero, zero, act)
            note("(d) apply from that scsh", R.assert_within(y, ref, bound, f"apply from the stats-only scsh {case} {fam} act {act}"))


# ---- (e) softmax ----------------------------------------------------------------------------------------------------------------------------------
def run_softmax(engine, x, ld, scale, valid, masked):
    rows, cols = x.shape
    buf = nan16(rows, ld)
    buf[:, :cols] = dev(x)
    if masked:
        check(engine.lib.gn_softmax_rows_masked(engine._ctx, ptr(buf), rows, cols, ld, scale, valid), "gn_softmax_rows_masked")
    else:
        check(engine.lib.gn_softmax_rows(engine._ctx, ptr(buf), rows, cols, ld, scale), "gn_softmax_rows")
    engine.synchronize()
    assert bool(torch.isnan(buf[:, cols:]).all()), "the pad columns keep their NaN"
    return buf[:, :cols]


@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_softmax_rows(engine, case):
    rows, cols = case
    x = R.softmax_inputs(case)
    for valid in R.softmax_valids(cols):
        for scale in R.SOFTMAX_SCALES:
            ref, Tm = R.softmax_ref(x, scale, valid)
            bound = R.softmax_bound(ref, Tm)
            outs = []
            for ld in (cols, cols + 8):
                for masked in ((False, True) if valid == cols else (True,)):
                    y = run_softmax(engine, x, ld, scale, valid, masked)
                    what = f"softmax {case} valid {valid} scale {scale} ld {ld} {'masked' if masked else 'plain'}"
                    note("(e) softmax y", R.assert_within(y, ref, bound, what))
                    assert bool((y[:, valid:] == 0).all()), f"{what}: columns >= valid are exact zeros"
                    total = y.cpu().to(F64).sum(-1)
                    assert float((total - 1).abs().max()) <= cols * 2.0 ** -11, f"{what}: row sums {total.min()} .. {total.max()}"
                    outs.append(y.contiguous())
            assert all(bits_equal(o, outs[0]) for o in outs), "ld and the entry point do not change a bit"


# ---- (f) refusals ---------------------------------------------------------------------------------------------------------------------------------
LN_REFUSALS = ["C % 8", "C = 4104", "C = 0", "M = 0", "null x", "null y", "x misaligned", "y misaligned", "gamma misaligned", "beta misaligned"]


@pytest.mark.parametrize("what", LN_REFUSALS)
def test_layernorm_fwd_refusals(engine, what):
    """Every GN_REQUIRE of gn_layernorm_fwd returns an error before anything is launched: y keeps its sentinel.  (The buffers are sized for the
    largest shape named, whatever is refused.)"""
    M, Cc, big = 8, 320, 4104
    x, y = torch.zeros(M + 1, big, dtype=F16, device="cuda"), sent16(M + 1, big)
    gamma, beta = torch.ones(big + 8, dtype=F16, device="cuda"), torch.zeros(big + 8, dtype=F16, device="cuda")
    a = dict(x=x.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(), M=M, Cc=Cc)
    a.update({"C % 8": dict(Cc=316), "C = 4104": dict(Cc=big), "C = 0": dict(Cc=0), "M = 0": dict(M=0), "null x": dict(x=None), "null y": dict(y=None),
              "x misaligned": dict(x=x.data_ptr() + 2), "y misaligned": dict(y=y.data_ptr() + 2), "gamma misaligned": dict(gamma=gamma.data_ptr() + 2),
              "beta misaligned": dict(beta=beta.data_ptr() + 2)}[what])
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_layernorm_fwd"):
        check(raw_ln(engine, **a), "gn_layernorm_fwd")
    engine.synchronize()
    assert bool((y.view(torch.int16) == SENTINEL16).all()), f"{what}: y was written"


GN_REFUSALS = ["C1 % 8", "C2 % 8", "HW = 0", "B = 0", "C1 = 0", "C % groups", "groups = 0", "groups = 512", "x2 without C2", "C2 without x2", "act = GELU",
               "act = -1", "y NULL without save_scsh", "stats_in with save_stats", "stats_in with save_scsh", "stats_in with y NULL",
               "stats_in with gamma misaligned", "stats_in misaligned", "x misaligned", "y misaligned", "workspace misaligned", "null workspace",
               "null gamma", "null x"]


@pytest.mark.parametrize("what", GN_REFUSALS)
def test_groupnorm_fwd_refusals(engine, what):
    """Every GN_REQUIRE of gn_groupnorm_fwd comes before the first launch: y, the save buffers and the workspace keep their sentinel / NaN."""
    case = [1, 16, 512, 0, 32]
    x1, x2 = torch.zeros(1, 16, 520, dtype=F16, device="cuda"), torch.zeros(1, 16, 520, dtype=F16, device="cuda")
    gamma, beta = torch.ones(1040, dtype=F16, device="cuda"), torch.zeros(1040, dtype=F16, device="cuda")
    y, stats, scsh = sent16(1, 16, 1040 + 8), sent32(1, 512, 2), sent32(1, 1040, 2)
    blk = torch.zeros(1, 1, 512, R.STATS_LINE, dtype=torch.int64, device="cuda")
    ws, n = nan_workspace(engine, (1, 16, 1040, 0, 1))
    p = dict(x=x1.data_ptr(), x2=None, gamma=gamma.data_ptr(), beta=beta.data_ptr(), y=y.data_ptr(), ws=ws.data_ptr(), act=R.ACT_SILU, save_stats=None,
             save_scsh=None, stats_in=None)
    if what == "C1 % 8":
        case[2] = 508
    elif what == "C2 % 8":
        case[3], p["x2"] = 4, x2.data_ptr()
    elif what == "HW = 0":
        case[1] = 0
    elif what == "B = 0":
        case[0] = 0
    elif what == "C1 = 0":
        case[2], case[3], p["x2"] = 0, 512, x2.data_ptr()
    elif what == "C % groups":
        case[4] = 24
    elif what == "groups = 0":
        case[4] = 0
    elif what == "groups = 512":
        case[4] = 512
    elif what == "x2 without C2":
        p["x2"] = x2.data_ptr()
    elif what == "C2 without x2":
        case[3] = 512
    elif what == "act = GELU":
        p["act"] = 2
    elif what == "act = -1":
        p["act"] = -1
    elif what == "y NULL without save_scsh":
        p["y"] = None
    elif what == "stats_in with save_stats":
        p.update(stats_in=blk.data_ptr(), save_stats=stats.data_ptr())
    elif what == "stats_in with save_scsh":
        p.update(stats_in=blk.data_ptr(), save_scsh=scsh.data_ptr())
    elif what == "stats_in with y NULL":
        p.update(stats_in=blk.data_ptr(), save_scsh=scsh.data_ptr(), y=None)
    elif what == "stats_in with gamma misaligned":
        p.update(stats_in=blk.data_ptr(), gamma=gamma.data_ptr() + 2)
    elif what == "stats_in misaligned":
        p.update(stats_in=blk.data_ptr() + 4)
    elif what == "x misaligned":
        p["x"] = x1.data_ptr() + 2
    elif what == "y misaligned":
        p["y"] = y.data_ptr() + 2
    elif what == "workspace misaligned":
        p["ws"] = ws.data_ptr() + 4
    elif what == "null workspace":
        p["ws"] = None
    elif what == "null gamma":
        p["gamma"] = None
    elif what == "null x":
        p["x"] = None
    d = GroupNormDesc()
    d.x, d.x2, d.gamma, d.beta, d.y, d.workspace = p["x"], p["x2"], p["gamma"], p["beta"], p["y"], p["ws"]
    d.B, d.HW, d.C1, d.C2, d.groups = case
    d.act, d.eps = p["act"], R.EPS
    d.save_stats, d.save_scsh, d.stats_in, d.stats_replicas = p["save_stats"], p["save_scsh"], p["stats_in"], 1 if p["stats_in"] else 0
    engine.synchronize()
    with pytest.raises(GenimaHipError, match="gn_groupnorm_fwd"):
        check(engine.lib.gn_groupnorm_fwd(engine._ctx, C.byref(d)), "gn_groupnorm_fwd")
    engine.synchronize()
    assert bool((y.view(torch.int16) == SENTINEL16).all()), f"{what}: y was written"
    assert bool((stats.view(torch.int32) == SENTINEL32).all()) and bool((scsh.view(torch.int32) == SENTINEL32).all()), f"{what}: a save buffer was written"
    assert bool(torch.isnan(ws[:n]).all()), f"{what}: a kernel ran (the workspace was written)"


SOFTMAX_REFUSALS = ["cols % 8", "cols = 4104", "cols = 0", "rows = 0", "ld % 8", "ld < cols", "null x", "x misaligned"]
MASKED_REFUSALS = ["valid = 0", "valid = -1", "valid = cols + 1"]


@pytest.mark.parametrize("what,masked", [(w, False) for w in SOFTMAX_REFUSALS] + [(w, True) for w in SOFTMAX_REFUSALS + MASKED_REFUSALS])
def test_softmax_rows_refusals(engine, what, masked):
    """Both softmax entry points refuse before the launch and leave the scores alone.  valid = 0 in particular: every score of the row masked would
    be exp(-inf - -inf) = NaN in every column, so gn_softmax_rows_masked refuses it (as valid < 0 and valid > cols) -- its one caller, the
    cross-attention backward of training.py, passes the prompt's key count, which is at least 1."""
    rows, cols, ld, valid = 4, 256, 256, 200
    x = sent16(8, 4104 + 8)
    a = {"cols % 8": (rows, 252, 256), "cols = 4104": (rows, 4104, 4104), "cols = 0": (rows, 0, ld), "rows = 0": (0, cols, ld), "ld % 8": (rows, cols, 260),
         "ld < cols": (rows, cols, 248)}.get(what, (rows, cols, ld))
    valid = {"valid = 0": 0, "valid = -1": -1, "valid = cols + 1": cols + 1}.get(what, valid)
    xp = {"null x": None, "x misaligned": x.data_ptr() + 2}.get(what, x.data_ptr())
    name = "gn_softmax_rows_masked" if masked else "gn_softmax_rows"
    engine.synchronize()
    with pytest.raises(GenimaHipError, match=name):
        if masked:
            check(engine.lib.gn_softmax_rows_masked(engine._ctx, xp, a[0], a[1], a[2], 0.125, min(valid, a[1]) if what not in MASKED_REFUSALS else valid), name)
        else:
            check(engine.lib.gn_softmax_rows(engine._ctx, xp, a[0], a[1], a[2], 0.125), name)
    engine.synchronize()
    assert bool((x.view(torch.int16) == SENTINEL16).all()), f"{what}: the scores were written"
