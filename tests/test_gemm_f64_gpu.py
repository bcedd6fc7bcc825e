"""-m gpu: gn_gemm against the f64 reference of tests/gemm_ref.py, PER ELEMENT, on every block-tile configuration: every element of every output within
    1/2 ulp16(ref) + S E_z + K_act 2^-24 T_act (+ out_scale / residual roundings)
-- the bound gemm_ref.py derives from csrc/gemm_common.h and tests/test_gemm_ref_cpu.py shows to hold for plain f32 evaluation and to reject a tanh GELU, an
f16 accumulator, a double-rounded residual, a dropped K element, a swapped GEGLU half, a wrong border tap and f16 variance terms, most of which
util.assert_close (tests/test_gemm_tiles_gpu.py's bar) lets through.  Dense and conv, every activation x epilogue mode, row / column / K edges on one
tile of each kernel family with four input families, f32 / accumulating / batch-transposed / two-destination outputs, GEGLU, split-K through
splitk_reduce_kernel, the LayerNorm fold, and the persistent tile 25.  The largest err / bound per kernel family and epilogue is printed at the end
(test_zz_report): reported, not asserted."""
import ctypes as C

import pytest
import torch

import gemm_ref as R
from gemm_ref import F64, assert_within
from genima_amd._lib import GEMM_DMA, GEMM_PP, GEMM_PPP, GEMM_REG, GEMM_RING, OUT_ROWMAJOR, GemmDesc, gemm_tiles

pytestmark = pytest.mark.gpu

CFG = gemm_tiles()
TILES = [t for t, c in CFG.items() if c.family != GEMM_PPP]
PPP_TILES = [t for t, c in CFG.items() if c.family == GEMM_PPP]
assert sorted(TILES + PPP_TILES) == list(range(1, len(CFG) + 1)) and len(TILES) == 24 and PPP_TILES == [25], (TILES, PPP_TILES)  # must not shrink unnoticed
FAMILY_NAME = {GEMM_REG: "register-staged", GEMM_DMA: "LDS-DMA", GEMM_PP: "ping-pong", GEMM_RING: "3-stage ring", GEMM_PPP: "persistent ping-pong"}
FAMILY_TILE = {GEMM_REG: 2, GEMM_DMA: 9, GEMM_PP: 15, GEMM_RING: 16}  # the tile of each family the edge lists and the full conv list run on
assert all(CFG[t].family == f and (CFG[t].bm, CFG[t].bn) in R.EDGE_TILE_SHAPES for f, t in FAMILY_TILE.items())
GEGLU_TILES = [t for t in TILES if CFG[t].geglu]
DMA_TILES = [t for t in TILES if CFG[t].family in (GEMM_DMA, GEMM_RING)]  # the kernels that carry the LayerNorm fold
assert len(GEGLU_TILES) == 10 and len(DMA_TILES) == 17, (GEGLU_TILES, DMA_TILES)

RATIOS: dict = {}


def _note(family, label: str, ratio: float):
    """family: the kernel family that RAN (_runs), or a string"""
    key = (FAMILY_NAME.get(family, family), label)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _runs(tile: int, K: int, C1: int = 0, C2: int = 0, conv: bool = False) -> int:
    """The kernel family that runs when ``tile`` is named for a problem -- plan_gemm's substitutions (csrc/gemm.hip) restated, so that a result is filed under
    the kernel that produced it and a test can insist on the one it is about: the ping-pong kernel takes whole K tiles and, in a conv, 64-channel multiples
    of both inputs (pp_eligible; else the LDS-DMA 256 x 256 tile runs); a K tile of the LDS-DMA loaders (two-stage, ring) must not straddle a virtual concat
    (dma_eligible; else the tile's register-staged sibling runs).  A 1 x 1 conv view of a dense problem has C1 = K."""
    fam = CFG[tile].family
    if fam == GEMM_PP and (K % 64 or (conv and (C1 % 64 or C2 % 64))):
        fam = GEMM_DMA
    if fam != GEMM_REG and conv and C2 and (C1 % 64 or (C1 + C2) % 64):
        fam = GEMM_REG
    return fam


def _workspace_bytes(eng, M: int, N: int, K: int, x, w, out, bias=None, residual=None, act: int = 0, splitk: int = 0, tile: int = 0) -> int:
    """gn_gemm_workspace_bytes of the dense row-major launch Engine.linear builds: the planner's own answer to "is K split, and how many ways"."""
    d = GemmDesc()
    d.a, d.w, d.out = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias, d.residual = (bias.data_ptr() if bias is not None else None), (residual.data_ptr() if residual is not None else None)
    d.M, d.N, d.K, d.lda, d.ldw, d.ldo, d.ldr = M, N, K, K, K, N, (N if residual is not None else 0)
    d.out_mode, d.act, d.splitk, d.out_scale, d.tile = OUT_ROWMAJOR, act, splitk, 1.0, tile
    return int(eng.lib.gn_gemm_workspace_bytes(C.byref(d)))


@pytest.fixture()
def eng(engine):
    old, old_auto = getattr(engine, "no_table", False), engine.autotune
    engine.no_table, engine.autotune = True, False  # the override decides, not the tune table / the autotuner
    yield engine
    engine.no_table, engine.autotune = old, old_auto
    engine.lib.gn_set_gemm_tile_override(-1)


def _override(eng, tile: int):
    eng.lib.gn_set_gemm_tile_override(tile - 1)


def _cu(t):
    return None if t is None else t.cuda()


def _triples(tile: int):
    c = CFG[tile]
    return [R.tile_triple(c.bm, c.bn, k_tail=c.family != GEMM_PP)] + R.SHARED_TRIPLES


def _run_dense(eng, x, w, b, r, act: int, mode: str):
    """Engine.linear; the residual before the activation and out_scale through the 1 x 1 conv2d view of the same problem (as the seeded sweep does)."""
    ub, ur, first, scale = R.MODES[mode]
    b, r = (b if ub else None), (r if ur else None)
    if first or scale != 1.0:
        (M, K), N = x.shape, w.shape[0]
        return eng.conv2d(x.view(1, 1, M, K), w, b, ksize=1, residual=None if r is None else r.view(1, 1, M, N), act=act, residual_before_act=first,
                          out_scale=scale).view(M, N)
    return eng.linear(x, w, b, act=act, residual=r)


def _check_dense(eng, tile: int, case, family: str, combos):
    x, w, b, r = (_cu(t) for t in R.dense_inputs(case, family))
    ran = _runs(tile, case[2], C1=case[2], conv=True)  # (the 1 x 1 conv view of two of the modes asks no more of K than the dense call)
    failed = []
    for act, mode in combos:
        ref = R.dense_ref(case, family, act, mode)
        y = _run_dense(eng, x, w, b, r, act, mode)
        try:
            _note(ran, f"dense {R.ACT_NAME[act]} / {mode}" + ("" if family == "gauss" else f" [{family}]"),
                  assert_within(y, ref.y, ref.bound, f"tile {tile} {case} {family} {R.ACT_NAME[act]} {mode}"))
        except AssertionError as e:  # look at every combination before raising
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ---- dense: every tile x activation x epilogue mode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
def test_dense_every_activation_and_mode_every_tile(eng, tile):
    """The tile's own ragged problem (BM + 33, BN + 12, K = 136) and the two shared ones: act in {none, silu, gelu, quick_gelu, relu} x {no bias, bias,
    bias + residual after, bias + residual before (1 x 1 conv view), out_scale 0.5}."""
    _override(eng, tile)
    for case in _triples(tile):
        assert _runs(tile, case[2]) == CFG[tile].family, (tile, case)  # the tile named is the tile that runs
        _check_dense(eng, tile, case, "gauss", [(a, m) for a in R.ACTS for m in R.MODES])


# ---- edges: M, N, K lists x the four input families on one tile of each kernel family ----------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("kfam", list(FAMILY_TILE), ids=lambda f: FAMILY_NAME[f])
def test_edge_shapes_and_input_families(eng, kfam, family):
    """M in {1, 31, 33, BM - 1, BM, BM + 1}, N in {4, 8, 76, BN - 4, BN, BN + 8}, K in {8, 56, 64, 72, 136, 192}; gauss, cancel (sum|x||w| >> |result|), tiny
    (results in the f16 subnormal range) and, for the smooth activations, wide (pre-activations from -110 to 110).  The ping-pong kernel takes whole K
    tiles only, so ITS M and N lists run at K = 64 and K = 128 and every one of them runs on it; of the K list it takes 64 and 192, the other four run the
    LDS-DMA 256 x 256 tile, as they do in the product, and are filed under that kernel."""
    tile = FAMILY_TILE[kfam]
    _override(eng, tile)
    cases = R.edge_cases(CFG[tile].bm, CFG[tile].bn, whole_k=kfam == GEMM_PP)
    on_it = [c for c in cases if _runs(tile, c[2]) == kfam]
    assert len(on_it) == (len(cases) - 4 if kfam == GEMM_PP else len(cases)), (kfam, on_it)
    assert {c[0] for c in on_it} >= {1, 31, 33, CFG[tile].bm - 1, CFG[tile].bm, CFG[tile].bm + 1}
    assert {c[1] for c in on_it} >= {4, 8, 76, CFG[tile].bn - 4, CFG[tile].bn, CFG[tile].bn + 8}
    for case in cases:
        _check_dense(eng, tile, case, family, R.dense_combos(case, family))


# ---- the other outputs ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


@pytest.mark.parametrize("tile", TILES)
def test_f32_accumulate_transposed_and_two_destinations_every_tile(eng, tile):
    from genima_amd import train_ops as T

    _override(eng, tile)
    M, N, K = 200, 136, 128
    assert _runs(tile, K) == CFG[tile].family
    a, w, b, _ = R.dense_inputs((M, N, K))
    one, two = R.gemm_ref(F64, a, w, out_f32=True), R.accumulate_twice_ref(a, w, 0.25)
    ad, wd, bd = a.cuda(), w.cuda(), b.cuda()
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32)   # f32 output without accumulate: whatever was there is overwritten
    T.gemm(eng, ad, wd, out, M, N, K, K, K, N, f32_out=True)
    _note(CFG[tile].family, "f32 output", assert_within(out, one.y, one.bound, f"tile {tile} f32 output"))
    out = torch.full((M, N), 0.25, device="cuda", dtype=torch.float32)           # two accumulating calls onto a non-zero start
    T.gemm(eng, ad, wd, out, M, N, K, K, K, N, f32_out=True, accumulate=True)
    T.gemm(eng, ad, wd, out, M, N, K, K, K, N, f32_out=True, accumulate=True)
    _note(CFG[tile].family, "f32 output, accumulate x 2", assert_within(out, two.y, two.bound, f"tile {tile} f32 accumulate"))
    # batch-transposed output y[b, n, m_local], row stride pad: the pad columns keep what they held
    Bn, rows, pad = 2, 100, 104
    ref = R.gemm_ref(F64, a, w, b)
    tr = lambda t: t.view(Bn, rows, -1).permute(0, 2, 1)  # noqa: E731
    y = torch.full((Bn, N, pad), SENTINEL, device="cuda", dtype=torch.float16)
    eng.linear(ad.view(Bn, rows, K), wd, bd, transposed_out=True, rows_per_batch=rows, pad_cols=pad, out=y)
    _note(CFG[tile].family, "batch-transposed", assert_within(y[:, :, :rows], tr(ref.y), tr(ref.bound), f"tile {tile} transposed"))
    assert bool((y[:, :, rows:] == SENTINEL).all()), f"tile {tile}: transposed output wrote its pad columns"
    # two destinations: columns [0, 2 Cq) row-major, [2 Cq, 3 Cq) batch-transposed
    Cq = 96
    _, w3, b3, _ = R.dense_inputs((M, 3 * Cq, K))
    ref = R.gemm_ref(F64, a, w3, b3)
    vt = torch.full((Bn, Cq, pad), SENTINEL, device="cuda", dtype=torch.float16)
    qk, vt2 = eng.linear(ad.view(Bn, rows, K), w3.cuda(), b3.cuda(), split_n=2 * Cq, rows_per_batch=rows, pad_cols=pad, out2=vt)
    assert vt2.data_ptr() == vt.data_ptr()
    _note(CFG[tile].family, "split_n q|k", assert_within(qk.reshape(M, 2 * Cq), ref.y[:, :2 * Cq], ref.bound[:, :2 * Cq], f"tile {tile} q|k part"))
    _note(CFG[tile].family, "split_n V^T", assert_within(vt[:, :, :rows], tr(ref.y[:, 2 * Cq:]), tr(ref.bound[:, 2 * Cq:]), f"tile {tile} V^T part"))
    assert bool((vt[:, :, rows:] == SENTINEL).all()), f"tile {tile}: V^T wrote its pad columns"


@pytest.mark.parametrize("tile", GEGLU_TILES)
def test_geglu_every_geglu_tile(eng, tile):
    """(acc_h + b_h) gelu_fast(acc_g + b_g) on packed hidden | gate blocks: N = 320 (a ragged last block of the tile, 8-byte stores) and N = 384 (N % 128 == 0:
    the 16-byte store path)."""
    _override(eng, tile)
    for case in R.GEGLU_CASES:
        x, wp, bp, ref = R.geglu_fixture(case)
        y = eng.linear(x.cuda(), wp.cuda(), bp.cuda(), act=R.ACT_GEGLU)
        _note(CFG[tile].family, "GEGLU", assert_within(y, ref.y, ref.bound, f"tile {tile} GEGLU {case}"))


# ---- split-K -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,sk", R.SPLITK_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_splitk_reduce(eng, case, sk):
    """Partial f32 slabs summed in z order by splitk_reduce_kernel, then epilogue_store4: explicit 2 and 5 slabs, and the planner's own small-M split (at most
    16 slabs for an f16 output, plan_gemm).  The slab count is the planner's (its workspace is slabs x M x N floats): K IS split, the asked number of
    ways, and that count enters the bound.  K is long: the accumulation term leads the bound here."""
    M, N, K = case
    x, w, b, r = R.dense_inputs(case)
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda()
    for label, kw, rkw in (("bias + SiLU", dict(bias=bd, act=R.ACT_SILU), dict(bias=b, act=R.ACT_SILU)), ("residual", dict(residual=rd), dict(res=r))):
        out = torch.empty(M, N, device="cuda", dtype=torch.float16)
        slabs, rest = divmod(_workspace_bytes(eng, M, N, K, xd, wd, out, splitk=sk, **kw), M * N * 4)
        assert rest == 0 and (slabs == sk if sk else 1 < slabs <= R.AUTO_SPLITK_MAX), (case, sk, slabs)
        ref = R.gemm_ref(F64, x, w, splitk=slabs, **rkw)
        y = eng.linear(xd, wd, kw.get("bias"), act=kw.get("act", R.ACT_NONE), residual=kw.get("residual"), splitk=sk, out=out)
        _note("split-K reduce", label, assert_within(y, ref.y, ref.bound, f"split-K {case} x{sk} -> {slabs} slabs, {label}"))


# ---- conv ----------------------------------------------------------------------------------------------------------------------------------------------
def _check_conv(eng, tile: int, case):
    c, ref = R.conv_fixture(case)
    y = eng.conv2d(c.x.cuda(), c.w.cuda(), c.bias.cuda(), ksize=c.k, stride=c.stride, pad=c.pad, x2=_cu(c.x2), shift=_cu(c.shift_t), residual=_cu(c.res_t),
                   act=c.act, upsample2x=c.ups, out_scale=c.out_scale, residual_before_act=c.res_first)
    _note(_runs(tile, c.k * c.k * (c.C1 + c.C2), c.C1, c.C2, conv=True), "conv " + R.conv_id(case), assert_within(y, ref.y, ref.bound, f"tile {tile} conv {R.conv_id(case)}"))


@pytest.mark.parametrize("tile", TILES)
def test_conv_every_tile(eng, tile):
    """3 x 3 / stride 1 / virtual concat, and 3 x 3 / stride 2 / ragged Cout + SiLU + residual."""
    _override(eng, tile)
    for case in R.CONV_EVERY_TILE:
        _check_conv(eng, tile, case)


@pytest.mark.parametrize("kfam", list(FAMILY_TILE), ids=lambda f: FAMILY_NAME[f])
def test_conv_case_list(eng, kfam):
    """The whole conv list (1 x 1 and 3 x 3, stride 2, the asymmetric pad, concat inside a K tile, taps straddling a K tile, fused upsample, shift / residual /
    residual before the activation / out_scale) on one tile of each kernel family.  The ping-pong kernel takes the four cases whose inputs are 64-channel
    multiples, the LDS-DMA loaders every case but the four whose concat falls inside a K tile; the others run the kernel the planner substitutes and are
    filed under it (_runs)."""
    _override(eng, FAMILY_TILE[kfam])
    on_it = [c for c in R.CONV_CASES if _runs(FAMILY_TILE[kfam], c[6] * c[6] * (c[3] + c[4]), c[3], c[4], conv=True) == kfam]
    assert len(on_it) == {GEMM_REG: 11, GEMM_DMA: 7, GEMM_PP: 4, GEMM_RING: 7}[kfam], (kfam, len(on_it))
    failed = []
    for case in R.CONV_CASES:
        try:
            _check_conv(eng, FAMILY_TILE[kfam], case)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ---- LayerNorm fold ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", DMA_TILES)
def test_layernorm_fold_every_tile(eng, tile):
    """gn_gemm_desc.ln_c1 on rows with |mean| = 0, 6 and 20 spreads: plain + residual, GELU, GEGLU, the q | k + V^T two-destination form -- against the folded
    formula in f64 from the kernel's own inputs, the one-pass f32 statistics' error carried explicitly (gemm_ref.ln_fold_ref)."""
    _override(eng, tile)
    failed = []
    for case in R.LN_CASES:
        for kind in R.LN_KINDS:
            x, wg, c1, c2, res, ref = R.ln_fixture(case, kind)
            M, N, K = R.ln_shape(case, kind)
            what = f"tile {tile} ln-fold {(M, N, K)} {kind}"
            try:
                if kind == "qkv":
                    Bn, Cq = 2, N // 3
                    rows = M // Bn
                    pad = (rows + 7) // 8 * 8 + 8
                    vt = torch.full((Bn, Cq, pad), SENTINEL, device="cuda", dtype=torch.float16)
                    qk, _ = eng.linear(x.cuda().view(Bn, rows, K), wg.cuda(), c2.cuda(), ln_c1=c1.cuda(), split_n=2 * Cq, rows_per_batch=rows, pad_cols=pad, out2=vt)
                    tr = lambda t: t.view(Bn, rows, Cq).permute(0, 2, 1)  # noqa: E731
                    q1 = assert_within(qk.reshape(M, 2 * Cq), ref.y[:, :2 * Cq], ref.bound[:, :2 * Cq], what + " q|k")
                    q2 = assert_within(vt[:, :, :rows], tr(ref.y[:, 2 * Cq:]), tr(ref.bound[:, 2 * Cq:]), what + " V^T")
                    assert bool((vt[:, :, rows:] == SENTINEL).all()), what + ": V^T wrote its pad columns"
                    _note(CFG[tile].family, "LayerNorm fold qkv", max(q1, q2))
                else:
                    act = {"res": R.ACT_NONE, "gelu": R.ACT_GELU, "geglu": R.ACT_GEGLU}[kind]
                    y = eng.linear(x.cuda(), wg.cuda(), c2.cuda(), ln_c1=c1.cuda(), act=act, residual=_cu(res))
                    _note(CFG[tile].family, "LayerNorm fold " + kind, assert_within(y, ref.y, ref.bound, what))
            except AssertionError as e:
                failed.append(str(e))
    assert not failed, "\n".join(failed)


# ---- tile 25: the persistent ping-pong kernel ------------------------------------------------------------------------------------------------------------
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows_of_bands(bands, extra_stride: int, M: int) -> torch.Tensor:
    """every row of the 256-row bands named + every extra_stride-th row of the rest"""
    keep = torch.zeros(M, dtype=torch.bool)
    for b in bands:
        keep[256 * b:256 * (b + 1)] = True
    keep[::extra_stride] = True
    return keep.nonzero().flatten()


PPP_MAX_PARTS = 8   # gn_ppp_plan (csrc/gemm_ppp.hip): a tile of the last partial round is split into at most 8 parts along K
PPP_SLAB_BYTES = 256 * 256 * 4


def _ppp_takes(M: int, N: int, K: int) -> bool:
    """ppp_eligible (csrc/gemm.hip) for a dense row-major f16 launch with 16-byte aligned operands: whole 256 x 256 tiles, at least four whole K tiles, at
    least one tile per CU.  Anything else runs tile 15 or 7 under tile 25's name."""
    return M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 256 and (M // 256) * (N // 256) >= _ncu()


@pytest.mark.parametrize("M,N,K,act,res,first_bands,want_parts", [
    (16384, 1024, 256, R.ACT_NONE, False, [0, 63], 1),      # one full round at the minimum K: 64 x 4 = 256 tiles, no tail
    (28160, 2048, 256, R.ACT_SILU, True, [0, 32, 64], 1),   # 110 x 8 = 880 tiles: 3 rounds + 112 tail tiles; at K = 4 tiles the planner leaves them whole
    (20480, 1024, 1280, R.ACT_SILU, True, [0], 4),           # 80 x 4 = 320 tiles: 64 tail tiles, 4 parts each (3 hand-offs a tile)
    (18432, 1024, 1024, R.ACT_NONE, True, [0], 8)])          # 72 x 4 = 288 tiles: 32 tail tiles, 8 parts each -- the most the planner deals
def test_tile25_dense(eng, M, N, K, act, res, first_bands, want_parts):
    """The f64 reference is evaluated on a SUBSET of rows: every row of the bands named -- the first band of each full round (a round is 256 tiles = 256 / (N / 256)
    bands; all the band's column tiles, so whole tiles) -- and EVERY band of the last, partial round (all its tiles, split along K or not), plus every 61st
    row of the rest.  The parts a tail tile is split into are the planner's own (its workspace is one 256 x 256 f32 slab per hand-off): the two problems
    meant to hand partial sums over DO, and the owner's additions enter the bound like a split K's."""
    if _ncu() != 256:
        pytest.skip("tile counts are written for 256 CUs")
    from util import randn_h

    assert _ppp_takes(M, N, K)
    tiles_n = N // 256
    bands = M // 256
    full = (bands * tiles_n // 256) * 256 // tiles_n       # bands of the full rounds
    tail = (bands - full) * tiles_n                        # tiles of the last partial round
    rows = _rows_of_bands(first_bands + list(range(full, bands)), 61, M)
    x, w, b = randn_h(M, K, seed=1, device="cpu"), randn_h(N, K, seed=2, scale=K ** -0.5, device="cpu"), randn_h(N, seed=3, device="cpu")
    r = randn_h(M, N, seed=4, device="cpu") if res else None
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), _cu(r)
    out = torch.empty(M, N, device="cuda", dtype=torch.float16)
    t0 = int(eng.lib.gn_ppp_timeouts())
    _override(eng, 25)
    ws = _workspace_bytes(eng, M, N, K, xd, wd, out, bias=bd, residual=rd, act=act)
    parts = ws // (tail * PPP_SLAB_BYTES) + 1 if tail else 1
    assert ws == (tail * (parts - 1) * PPP_SLAB_BYTES if tail else 0) and parts == want_parts <= PPP_MAX_PARTS, (ws, tail, parts)
    ref = R.gemm_ref(F64, x[rows], w, b, res=None if r is None else r[rows], act=act, splitk=parts)
    y = eng.linear(xd, wd, bd, act=act, residual=rd, out=out)
    eng.synchronize()
    _note(GEMM_PPP, f"dense {R.ACT_NAME[act]}" + (" + residual" if res else "") + (f", tail in {parts} parts" if parts > 1 else ""),
          assert_within(y.cpu()[rows], ref.y, ref.bound, f"tile 25 {(M, N, K)}, tail tiles in {parts} parts"))
    assert int(eng.lib.gn_ppp_timeouts()) == t0, "a bounded hand-off wait gave up"


def test_tile25_feed_forward_variant(eng):
    """LayerNorm fold + GEGLU as one persistent launch at the smallest problem of one full round: 16 x 16 = 256 tiles, K = 256.  Reference on the rows of the
    first and the last band (whole tiles of every column) + every 16th row."""
    if _ncu() != 256:
        pytest.skip("tile counts are written for 256 CUs")
    M, N, K = 4096, 4096, 256
    assert _ppp_takes(M, N, K)
    x, w, b, gamma, beta, _ = R.ln_inputs((M, N, K), nh=1)
    wg, c1, c2 = R.fold_layernorm(R.pack_geglu_rows(w), gamma, beta, R.pack_geglu_rows(b))
    rows = _rows_of_bands([0, M // 256 - 1], 16, M)
    ref = R.ln_fold_ref(F64, x[rows], wg, c1, c2, 1e-5, None, R.ACT_GEGLU)
    t0 = int(eng.lib.gn_ppp_timeouts())
    _override(eng, 25)
    y = eng.linear(x.cuda(), wg.cuda(), c2.cuda(), ln_c1=c1.cuda(), act=R.ACT_GEGLU)
    eng.synchronize()
    _note(GEMM_PPP, "LayerNorm fold geglu", assert_within(y.cpu()[rows], ref.y, ref.bound, "tile 25 feed-forward variant"))
    assert int(eng.lib.gn_ppp_timeouts()) == t0


def test_zz_report():
    """Not an assertion: the largest err / bound seen per kernel family and epilogue, for the record of how much room the derived bound leaves."""
    for (fam, label), v in sorted(RATIOS.items()):
        print(f"REPORT {fam:22s} {label:60s} {v:.3f}")
