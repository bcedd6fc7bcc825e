"""-m gpu: EVERY block-tile configuration of gn_gemm but the persistent ping-pong one (register-staged, LDS-DMA, ping-pong, 3-stage ring,
exact-fit; test_gemm_ppp_gpu.py has the persistent one) through EVERY epilogue mode -- bias, per-batch time shift, residual before / after the activation, activation, output
scale, narrow (N % 8 != 0) rows, f32 output with accumulation, batch-transposed output -- against an fp32 torch restatement on the
same f16-rounded inputs.  The engine's autotuner only ever runs the per-shape winner, so without this test a tile whose epilogue
variant is wrong shows up as a NaN three subsystems later (the fused epilogue is shared: csrc/gemm_common.h).
Reference ops: diffusers' ResnetBlock2D / Attention / FeedForward Linear + conv call sites."""
import pytest
import torch
import torch.nn.functional as F

from genima_amd._lib import GEMM_DMA, GEMM_PPP, GEMM_RING, gemm_tiles
import gemm_ref
from util import assert_close, randn_h

pytestmark = pytest.mark.gpu

TILES = [t for t, c in gemm_tiles().items() if c.family != GEMM_PPP]
assert len(TILES) == 24, TILES  # the parametrisation must not shrink unnoticed


@pytest.fixture()
def tile_override(engine):
    yield lambda t: engine.lib.gn_set_gemm_tile_override(t - 1)
    engine.lib.gn_set_gemm_tile_override(-1)


@pytest.fixture()
def eng(engine):
    old, old_auto = getattr(engine, "no_table", False), engine.autotune
    engine.no_table, engine.autotune = True, False  # the override decides, not the tune table / the autotuner
    yield engine
    engine.no_table, engine.autotune = old, old_auto


ACTS = {0: lambda v: v, 1: F.silu, 2: F.gelu, 4: F.relu}


@pytest.mark.parametrize("tile", TILES)
def test_linear_epilogues_every_tile(eng, tile_override, tile):
    tile_override(tile)
    # ragged M (row tail inside a 32-row band), N = 5 x 64 + 8 (column tail inside a 32-column tile), K = 3 tiles
    for (M, N, K) in ((1000, 328, 192), (300, 76, 128)):  # 76: N % 8 != 0 -> the 8-byte store path
        x, w, b = randn_h(M, K, seed=1), randn_h(N, K, seed=2, scale=K ** -0.5), randn_h(N, seed=3, scale=0.3)
        r = randn_h(M, N, seed=4)
        xf, wf, bf, rf = x.float().cpu(), w.float().cpu(), b.float().cpu(), r.float().cpu()
        base = xf @ wf.t()
        for act in (0, 1, 2, 4):
            y = eng.linear(x, w, b, act=act, residual=r)
            assert_close(y, ACTS[act](base + bf) + rf, what=f"tile {tile} linear {M}x{N}x{K} act {act} +res")
        y = eng.linear(x, w, None)
        assert_close(y, base, what=f"tile {tile} linear {M}x{N}x{K} plain")


@pytest.mark.parametrize("tile", TILES)
def test_conv_epilogues_every_tile(eng, tile_override, tile):
    tile_override(tile)
    B, H, W, Cin, Cout = 3, 12, 20, 64, 136
    x, w, b = randn_h(B, H, W, Cin, seed=5), randn_h(Cout, 9 * Cin, seed=6, scale=(9 * Cin) ** -0.5), randn_h(Cout, seed=7, scale=0.3)
    shift, res = randn_h(B, Cout, seed=8), randn_h(B, H, W, Cout, seed=9)
    wt = w.float().cpu().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    conv = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), wt, b.float().cpu(), padding=1).permute(0, 2, 3, 1)
    sf, rf = shift.float().cpu()[:, None, None, :], res.float().cpu()
    y = eng.conv2d(x, w, b, shift=shift)                                  # ResnetBlock2D conv1 + time embedding
    assert_close(y, conv + sf, what=f"tile {tile} conv +shift")
    y = eng.conv2d(x, w, b, residual=res, out_scale=0.5)                   # conv2 + skip, output_scale_factor
    assert_close(y, conv * 0.5 + rf, what=f"tile {tile} conv scale +res")
    y = eng.conv2d(x, w, b, residual=res, act=4, residual_before_act=True)  # ResNet basic block: relu(conv + identity)
    assert_close(y, F.relu(conv + rf), what=f"tile {tile} conv relu(conv+res)")
    y = eng.conv2d(x, w, b, shift=shift, residual=res, act=1)               # both vectors at once (the tile-by-tile residual path)
    assert_close(y, F.silu(conv + sf) + rf, what=f"tile {tile} conv +shift silu +res")


@pytest.mark.parametrize("tile", TILES)
def test_f32_accumulate_and_transposed_every_tile(eng, tile_override, tile):
    from genima_amd import train_ops as T

    tile_override(tile)
    M, N, K = 200, 136, 128
    a, w = randn_h(M, K, seed=10), randn_h(N, K, seed=11, scale=K ** -0.5)
    ref = a.float().cpu() @ w.float().cpu().t()
    out = torch.full((M, N), 0.25, device="cuda", dtype=torch.float32)
    T.gemm(eng, a, w, out, M, N, K, K, K, N, f32_out=True, accumulate=True)
    T.gemm(eng, a, w, out, M, N, K, K, K, N, f32_out=True, accumulate=True)
    assert_close(out, 2 * ref + 0.25, what=f"tile {tile} f32 accumulate")
    # batch-transposed output (V^T for the attention kernel): y[b, n, m_local], row stride pad_cols
    Bn, rows, pad = 2, 100, 104
    b = randn_h(N, seed=12, scale=0.3)
    y = eng.linear(a.view(Bn, rows, K), w, b, transposed_out=True, rows_per_batch=rows, pad_cols=pad)
    want = (ref + b.float().cpu()).view(Bn, rows, N).permute(0, 2, 1)
    assert_close(y.view(Bn, N, pad)[:, :, :rows], want, what=f"tile {tile} transposed")
    # two destinations (q | k row-major + V^T in one launch): columns [0, 2C) and [2C, 3C)
    Cq = 96
    w3, b3 = randn_h(3 * Cq, K, seed=13, scale=K ** -0.5), randn_h(3 * Cq, seed=14, scale=0.3)
    qk, vt = eng.linear(a.view(Bn, rows, K), w3, b3, split_n=2 * Cq, rows_per_batch=rows, pad_cols=pad)
    full = a.float().cpu() @ w3.float().cpu().t() + b3.float().cpu()
    assert_close(qk.reshape(M, 2 * Cq), full[:, : 2 * Cq], what=f"tile {tile} q|k part")
    assert_close(vt.view(Bn, Cq, pad)[:, :, :rows], full[:, 2 * Cq:].view(Bn, rows, Cq).permute(0, 2, 1), what=f"tile {tile} V^T part")


def test_linear_random_shapes_and_tiles(eng, tile_override):
    """Seeded sweep: random (M, N, K) -- row / column / reduction tails everywhere --, random tile, random epilogue (bias, residual before or
    after the activation, activation) against torch; the tails decide which loader / epilogue branches run, so the fixed shapes above are
    not enough on their own.  Every case is also held to the per-element f64 bound of tests/gemm_ref.py."""
    import random

    rnd = random.Random(1234)
    for case in range(80):
        tile = rnd.choice(TILES)
        M = rnd.choice([1, 7, 31, 33, 64, 100, 129, 255, 300, 777, 1024, 2050])
        N = 4 * rnd.randint(1, 100) if rnd.random() < 0.5 else rnd.choice([64, 128, 160, 320, 328, 640, 72, 8])
        K = 8 * rnd.randint(1, 40) if rnd.random() < 0.5 else rnd.choice([64, 128, 320, 1024])
        act = rnd.choice([0, 0, 1, 2, 4])
        use_b, use_r, rfirst = rnd.random() < 0.7, rnd.random() < 0.6, rnd.random() < 0.3
        tile_override(tile)
        x, w = randn_h(M, K, seed=case), randn_h(N, K, seed=1000 + case, scale=K ** -0.5)
        b = randn_h(N, seed=2000 + case, scale=0.3) if use_b else None
        r = randn_h(M, N, seed=3000 + case) if use_r else None
        if use_r and rfirst and act:
            # residual before the activation goes through conv2d's flag; Linear adds it after: build the conv equivalent (1x1)
            y = eng.conv2d(x.view(1, 1, M, K), w, b, ksize=1, residual=r.view(1, 1, M, N), act=act, residual_before_act=True).view(M, N) if K % 8 == 0 else None
            ref = ACTS[act](x.float().cpu() @ w.float().cpu().t() + (b.float().cpu() if use_b else 0) + r.float().cpu())
        else:
            y = eng.linear(x, w, b, act=act, residual=r)
            ref = ACTS[act](x.float().cpu() @ w.float().cpu().t() + (b.float().cpu() if use_b else 0)) + (r.float().cpu() if use_r else 0)
        if y is not None:
            assert_close(y, ref, what=f"case {case}: tile {tile} {M}x{N}x{K} act {act} bias {use_b} res {use_r} first {rfirst}")
            # (splitk left at 1: the planner may split the K = 1024 small-M cases 2 ways, 2 additions beside 2 x 1024 in the bound's count)
            r64 = gemm_ref.gemm_ref(torch.float64, x.cpu(), w.cpu(), b.cpu() if use_b else None, res=r.cpu() if use_r else None,
                                    res_first=bool(use_r and rfirst and act), act=act)
            gemm_ref.assert_within(y, r64.y, r64.bound, f"case {case}: tile {tile} {M}x{N}x{K} act {act} bias {use_b} res {use_r} first {rfirst}, f64 bound")


def test_conv_random_shapes_and_tiles(eng, tile_override):
    """Seeded sweep of the implicit-GEMM conv: kernel 1 / 3, stride 1 / 2, virtual concat, fused nearest-2x upsample, ragged maps and
    channel counts, random tile, shift / residual epilogues -- against torch's conv2d on the same f16 inputs, and per element against the f64 im2col
    reference and bound of tests/gemm_ref.py."""
    import random

    rnd = random.Random(4321)
    for case in range(48):
        tile = rnd.choice(TILES)
        B, H, W = rnd.choice([1, 2, 3]), rnd.choice([5, 8, 12, 17]), rnd.choice([6, 8, 16, 19])
        C1, C2 = 8 * rnd.randint(1, 20), rnd.choice([0, 0, 8 * rnd.randint(1, 12)])
        Cout = 4 * rnd.randint(2, 60)
        k = rnd.choice([1, 3, 3])
        stride = rnd.choice([1, 1, 2]) if k == 3 else 1
        ups = k == 3 and stride == 1 and rnd.random() < 0.25
        tile_override(tile)
        x = randn_h(B, H, W, C1, seed=case)
        x2 = randn_h(B, H, W, C2, seed=500 + case) if C2 else None
        Cin = C1 + C2
        w = randn_h(Cout, k * k * Cin, seed=1000 + case, scale=(k * k * Cin) ** -0.5)
        b = randn_h(Cout, seed=1500 + case, scale=0.3)
        xin = torch.cat([x, x2], -1) if C2 else x
        xt = xin.float().cpu().permute(0, 3, 1, 2)
        if ups:
            xt = F.interpolate(xt, scale_factor=2.0, mode="nearest")
        wt = w.float().cpu().view(Cout, k, k, Cin).permute(0, 3, 1, 2)
        ref = F.conv2d(xt, wt, b.float().cpu(), stride=stride, padding=k // 2).permute(0, 2, 3, 1)
        shift = randn_h(B, Cout, seed=2000 + case) if rnd.random() < 0.4 else None
        res = randn_h(*ref.shape, seed=2500 + case) if rnd.random() < 0.5 else None
        y = eng.conv2d(x, w, b, ksize=k, stride=stride, x2=x2, shift=shift, residual=res, upsample2x=ups)
        want = ref + (shift.float().cpu()[:, None, None, :] if shift is not None else 0) + (res.float().cpu() if res is not None else 0)
        assert_close(y, want, what=f"case {case}: tile {tile} conv k{k} s{stride} ups {ups} {C1}+{C2}->{Cout} @{H}x{W} b{B}")
        r64 = gemm_ref.conv_ref(torch.float64, x.cpu(), x2.cpu() if C2 else None, w.cpu(), b.cpu(), k, stride, None, ups,
                                shift.cpu() if shift is not None else None, res.cpu() if res is not None else None)
        gemm_ref.assert_within(y, r64.y, r64.bound, f"case {case}: tile {tile} conv k{k} s{stride} ups {ups} {C1}+{C2}->{Cout} @{H}x{W} b{B}, f64 bound")


DMA_TILES = [t for t in TILES if gemm_tiles()[t].family in (GEMM_DMA, GEMM_RING)]  # the kernels that carry the LayerNorm fold (the library maps the others onto them)


def _fold(w, gamma, beta, b):
    """packing.fold_layernorms on one Linear (same arithmetic: f16-rounded W * gamma, f32 row sums of the rounded matrix, c2 in f16)."""
    wg = (w.float() * gamma.float()[None, :]).half()
    c1 = wg.float().sum(dim=1).contiguous()
    c2 = (w.float() @ beta.float() + (b.float() if b is not None else 0)).half()
    return wg.contiguous(), c1, c2


@pytest.mark.parametrize("tile", DMA_TILES)
def test_layernorm_fold_every_tile(eng, tile_override, tile):
    """gn_gemm_desc.ln_c1: Linear(LayerNorm(x)) from the RAW rows (row statistics out of the K loop's A fragments) against torch's
    layer_norm + linear in fp32 -- plain + residual, activation, GEGLU, the two-destination q | k | v epilogue; rows with a large mean
    (|mean| = 6 sigma) so that the mean * c1 cancellation is exercised; ragged M / N / K tails."""
    tile_override(tile)
    for (M, N, K) in ((1000, 328, 320), (300, 192, 200)):
        x = (randn_h(M, K, seed=21).float() * 0.7 + randn_h(M, 1, seed=22).float() * 4.0).half()
        w, b = randn_h(N, K, seed=23, scale=K ** -0.5), randn_h(N, seed=24, scale=0.3)
        gamma, beta = (1.0 + 0.3 * randn_h(K, seed=25).float()).half(), randn_h(K, seed=26, scale=0.2)
        r = randn_h(M, N, seed=27)
        ln = F.layer_norm(x.float().cpu(), (K,), gamma.float().cpu(), beta.float().cpu(), 1e-5)
        base = ln @ w.float().cpu().t() + b.float().cpu()
        wg, c1, c2 = _fold(w, gamma, beta, b)
        y = eng.linear(x, wg, c2, ln_c1=c1, residual=r)
        assert_close(y, base + r.float().cpu(), what=f"tile {tile} ln-fold {M}x{N}x{K} +res")
        y = eng.linear(x, wg, c2, ln_c1=c1, act=2)
        assert_close(y, F.gelu(base), what=f"tile {tile} ln-fold {M}x{N}x{K} gelu")
    # GEGLU (hidden | gate interleaved in 32-column blocks by packing.pack_geglu) and the q | k | v two-destination epilogue
    from genima_amd.packing import pack_geglu

    M, K, Nh = 520, 320, 192
    x = (randn_h(M, K, seed=31).float() + randn_h(M, 1, seed=32).float() * 3.0).half()
    w, b = randn_h(2 * Nh, K, seed=33, scale=K ** -0.5), randn_h(2 * Nh, seed=34, scale=0.3)
    gamma, beta = (1.0 + 0.3 * randn_h(K, seed=35).float()).half(), randn_h(K, seed=36, scale=0.2)
    ln = F.layer_norm(x.float().cpu(), (K,), gamma.float().cpu(), beta.float().cpu(), 1e-5)
    full = ln @ w.float().cpu().t() + b.float().cpu()
    want = full[:, :Nh] * F.gelu(full[:, Nh:])
    wp, bp = pack_geglu(w.float(), b.float())
    wg, c1, c2 = _fold(wp.cuda(), gamma, beta, bp.cuda())
    y = eng.linear(x, wg, c2, ln_c1=c1, act=5)  # (tiles whose wave tile is narrower than a hidden | gate pair: the library substitutes 128 x 128)
    assert_close(y, want, what=f"tile {tile} ln-fold GEGLU")
    Bn, rows, pad, Cq = 2, 260, 320, 96
    w3 = randn_h(3 * Cq, K, seed=37, scale=K ** -0.5)
    wg, c1, c2 = _fold(w3, gamma, beta, None)
    qk, vt = eng.linear(x.view(Bn, rows, K), wg, c2, ln_c1=c1, split_n=2 * Cq, rows_per_batch=rows, pad_cols=pad)
    full = ln @ w3.float().cpu().t()
    assert_close(qk.reshape(M, 2 * Cq), full[:, : 2 * Cq], what=f"tile {tile} ln-fold q|k")
    assert_close(vt.view(Bn, Cq, pad)[:, :, :rows], full[:, 2 * Cq:].view(Bn, rows, Cq).permute(0, 2, 1), what=f"tile {tile} ln-fold V^T")
