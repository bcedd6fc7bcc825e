"""-m gpu: the 3x3 conv from an LDS-resident patch in 64-channel groups on 128 x 160 output tiles (csrc/conv_patch.hip, gn_conv3x3_patch) --
the UNet / ControlNet ResnetBlock2D convs at 320 / 640 output channels -- against (a) torch fp32 `conv2d(q16(silu(x * scale + shift)))` on the
same f16-rounded inputs at the 1e-3 bar, (b) the GroupNorm launch + gn_gemm it replaces (rel L2 < 2e-4: the MFMA sees the same f16 values, only
the K order differs), and at graph level against the gate-closed route and the fp32 block.  Shapes: one tile whose whole halo is outside the
image, interior halos both ways, two samples of very different scale (a halo row that read the neighbouring sample would fail the bar),
1 / 3 / 5 channel groups, 1 / 2 output tiles."""
import pytest
import torch
import torch.nn.functional as F

from genima_amd import packing
from genima_amd._lib import ACT_NONE, ACT_SILU, GenimaHipError
from util import assert_close, q16, rel_l2

pytestmark = pytest.mark.gpu

G, EPS = 32, 1e-5


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


def _case(B, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g) * 1.5 + 0.3 * torch.randn(B, Cin, 1, 1, generator=g)
    x = q16(x * torch.tensor([1.0, 37.0, 0.05][:B]).view(B, 1, 1, 1))  # samples of very different scale: GroupNorm brings each back to O(1)
    w = q16(torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5)
    bias = q16(torch.randn(Cout, generator=g) * 0.2)
    gamma, beta = q16(1.0 + 0.2 * torch.randn(Cin, generator=g)), q16(0.2 * torch.randn(Cin, generator=g))
    res = q16(torch.randn(B, Cout, H, W, generator=g))
    return x, w, bias, gamma, beta, res


_refs = {}


def _reference(B, H, W, Cin, Cout):
    """torch fp32 on the f16-rounded inputs, computed once per shape: (inputs, normalised input, conv + bias)."""
    key = (B, H, W, Cin, Cout)
    if key not in _refs:
        c = _case(B, H, W, Cin, Cout, seed=H + Cin + Cout)
        x, w, bias, gamma, beta, _ = c
        n = q16(F.silu(F.group_norm(x, G, gamma, beta, EPS)))
        _refs[key] = (c, n, F.conv2d(n, w, bias, padding=1))
    return _refs[key]


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 8, 16, 64, 160), (2, 16, 32, 192, 320), (2, 16, 32, 320, 320), (2, 8, 16, 320, 160), (1, 16, 32, 64, 320)])
def test_conv3x3_patch_vs_torch_and_unfused(engine, B, H, W, Cin, Cout):
    (x, w, bias, gamma, beta, _), _, ref = _reference(B, H, W, Cin, Cout)
    xd, wd, bd = _nhwc(x).half().cuda(), packing.pack_conv_weight(w).cuda(), bias.half().cuda()
    gd, bed = gamma.half().cuda(), beta.half().cuda()
    assert engine.conv2d_patch_supported(xd, Cout)
    st = engine.groupnorm_stats(xd, gd, bed, G, EPS)
    n = engine.groupnorm(xd, gd, bed, G, EPS, act=ACT_SILU)
    y0 = engine.conv2d(n, wd, bd)  # the launches it replaces
    y = engine.conv2d_patch(xd, st, wd, bd, act=ACT_SILU)
    assert_close(_nchw(y), ref, what=f"conv3x3_patch {Cin}->{Cout} {H}x{W}")
    e = rel_l2(y, y0.float())
    assert e < 2e-4, e
    assert torch.equal(y, engine.conv2d_patch(xd, st, wd, bd, act=ACT_SILU)), "two runs are bit-identical"
    # ... and as the plain conv on the normalised tensor (the default route of graphs.emit_resnet)
    e = rel_l2(engine.conv2d_patch(n, None, wd, bd, act=ACT_NONE), y0.float())
    assert e < 2e-4, e


def test_conv3x3_patch_plain_conv(engine):
    """scsh == NULL, act NONE: the plain conv (zero padding from the out-of-range DMA lanes)."""
    x, w, bias, _, _, _ = _case(2, 16, 32, 192, 160, seed=9)
    x = q16(x.clamp(-8, 8))
    y = engine.conv2d_patch(_nhwc(x).half().cuda(), None, packing.pack_conv_weight(w).cuda(), bias.half().cuda(), act=ACT_NONE)
    assert_close(_nchw(y), F.conv2d(x, w, bias, padding=1), what="patch conv, no GroupNorm")


def test_conv3x3_patch_epilogues(engine):
    """bias + per-sample time shift (a column slice of a wider table, the two samples' shifts differ); bias + residual with ldr > Cout; ldo > Cout
    with the output pre-filled by a sentinel: columns >= Cout keep it."""
    B, H, W, Cin, Cout = 2, 16, 32, 192, 320
    (x, w, bias, gamma, beta, res), _, ref = _reference(B, H, W, Cin, Cout)
    xd, wd, bd = _nhwc(x).half().cuda(), packing.pack_conv_weight(w).cuda(), bias.half().cuda()
    st = engine.groupnorm_stats(xd, gamma.half().cuda(), beta.half().cuda(), G, EPS)
    g = torch.Generator().manual_seed(5)
    table = q16(torch.randn(B, 3 * Cout + 64, generator=g))
    table[1] *= 3.0
    off = Cout + 64
    td = table.half().cuda()
    y = engine.conv2d_patch(xd, st, wd, bd, shift=td[:, off:off + Cout], ldshift=td.shape[1])
    assert_close(_nchw(y), ref + table[:, off:off + Cout].view(B, Cout, 1, 1), what="bias + time shift")
    wide = torch.zeros(B, H, W, Cout + 24, dtype=torch.float16, device="cuda")
    wide[..., :Cout] = _nhwc(res).half().cuda()
    y = engine.conv2d_patch(xd, st, wd, bd, residual=wide[..., :Cout])
    assert_close(_nchw(y), ref + res, what="bias + residual, ldr > Cout")
    out = torch.full((B, H, W, Cout + 40), 7.5, dtype=torch.float16, device="cuda")
    y = engine.conv2d_patch(xd, st, wd, bd, out=out[..., :Cout])
    assert_close(_nchw(out[..., :Cout]), ref, what="ldo > Cout")
    assert bool((out[..., Cout:] == 7.5).all()), "columns >= Cout keep the sentinel"
    assert y.data_ptr() == out.data_ptr()


@pytest.mark.parametrize("C1,C2", [(64, 128), (128, 64)])
def test_conv3x3_patch_two_sources_equal_the_materialised_cat(engine, C1, C2):
    B, H, W, Cout = 2, 16, 32, 320
    (x, w, bias, gamma, beta, _), _, ref = _reference(B, H, W, C1 + C2, Cout)
    xd, wd, bd = _nhwc(x).half().cuda(), packing.pack_conv_weight(w).cuda(), bias.half().cuda()
    xa, xb = xd[..., :C1].contiguous(), xd[..., C1:].contiguous()
    gd, bed = gamma.half().cuda(), beta.half().cuda()
    st = engine.groupnorm_stats(xd, gd, bed, G, EPS)
    st2 = engine.groupnorm_stats(xa, gd, bed, G, EPS, x2=xb)
    assert_close(st2, st.float(), rel=1e-5, what="statistics over the two sources")
    assert engine.conv2d_patch_supported(xa, Cout, xb)
    y = engine.conv2d_patch(xd, st, wd, bd)
    y2 = engine.conv2d_patch(xa, st, wd, bd, x2=xb)
    assert torch.equal(y, y2), "[x | x2] must equal the same call on the materialised cat, bit for bit"
    assert_close(_nchw(y2), ref, what=f"two sources {C1} + {C2}")


def test_conv3x3_patch_recorded_program_equals_eager(engine):
    from genima_amd.engine import Engine

    B, H, W, Cin, Cout = 2, 16, 32, 192, 320
    (x, w, bias, gamma, beta, res), _, _ = _reference(B, H, W, Cin, Cout)
    xd, wd, bd, rd = _nhwc(x).half().cuda(), packing.pack_conv_weight(w).cuda(), bias.half().cuda(), _nhwc(res).half().cuda()
    gd, bed = gamma.half().cuda(), beta.half().cuda()
    eager = engine.conv2d_patch(xd, engine.groupnorm_stats(xd, gd, bed, G, EPS), wd, bd, residual=rd)
    R = Engine("cuda:0", record=True, autotune=False)
    y = R.conv2d_patch(xd, R.groupnorm_stats(xd, gd, bed, G, EPS, name="s"), wd, bd, residual=rd, name="y")
    m = R.meta[-1]
    assert m["kind"] == "conv3x3" and m["shape"] == (B * H * W, Cout, 9 * Cin) and m["flops"] == 2.0 * B * H * W * Cout * 9 * Cin
    R.run()
    R.synchronize()
    assert torch.equal(y, eager)


def test_conv3x3_patch_rejects_unsupported_shapes(engine):
    def z(*s):
        return torch.zeros(*s, dtype=torch.float16, device="cuda")

    assert engine.conv2d_patch_supported(z(1, 8, 16, 64), 160)
    assert not engine.conv2d_patch_supported(z(1, 8, 16, 96), 160)  # Cin % 64
    assert not engine.conv2d_patch_supported(z(1, 8, 16, 64), 128)  # Cout % 160
    assert not engine.conv2d_patch_supported(z(1, 12, 16, 64), 160)  # H % 8
    assert not engine.conv2d_patch_supported(z(1, 8, 24, 64), 160)  # W % 16
    assert not engine.conv2d_patch_supported(z(1, 8, 16, 96), 160, z(1, 8, 16, 32))  # C1 % 64 with x2
    for x, x2, cout in ((z(1, 8, 16, 96), None, 160), (z(1, 8, 16, 64), None, 128), (z(1, 12, 16, 64), None, 160), (z(1, 8, 24, 64), None, 160),
                        (z(1, 8, 16, 96), z(1, 8, 16, 32), 160)):
        cin = x.shape[-1] + (x2.shape[-1] if x2 is not None else 0)
        out = torch.full(tuple(x.shape[:3]) + (cout,), 3.0, dtype=torch.float16, device="cuda")
        with pytest.raises(GenimaHipError):
            engine.conv2d_patch(x, None, z(cout, 9 * cin), x2=x2, act=ACT_NONE, out=out)
        assert bool((out == 3.0).all()), "an unsupported problem launches nothing"


# ---- graph level: graphs.emit_resnet with the row gate opened --------------------------------------------------------------------------------
def _block(Cin, Cout, temb, seed, shortcut):
    g = torch.Generator().manual_seed(seed)
    sd = {"r.norm1.weight": 1.0 + 0.1 * torch.randn(Cin, generator=g), "r.norm1.bias": 0.1 * torch.randn(Cin, generator=g),
          "r.conv1.weight": torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5, "r.conv1.bias": 0.1 * torch.randn(Cout, generator=g),
          "r.norm2.weight": 1.0 + 0.1 * torch.randn(Cout, generator=g), "r.norm2.bias": 0.1 * torch.randn(Cout, generator=g),
          "r.conv2.weight": torch.randn(Cout, Cout, 3, 3, generator=g) * (9 * Cout) ** -0.5, "r.conv2.bias": 0.1 * torch.randn(Cout, generator=g)}
    if shortcut:
        sd["r.conv_shortcut.weight"] = torch.randn(Cout, Cin, 1, 1, generator=g) * Cin ** -0.5
        sd["r.conv_shortcut.bias"] = 0.1 * torch.randn(Cout, generator=g)
    sd = {k: q16(v) for k, v in sd.items()}
    x = q16(torch.randn(2, Cin, 16, 32, generator=g) * 1.3)
    shift = q16(torch.randn(2, Cout, generator=g) * torch.tensor([0.5, 2.0]).view(2, 1)) if temb else None
    h = F.conv2d(F.silu(F.group_norm(x, G, sd["r.norm1.weight"], sd["r.norm1.bias"], EPS)), sd["r.conv1.weight"], sd["r.conv1.bias"], padding=1)
    if temb:
        h = h + shift.view(2, Cout, 1, 1)
    h = F.conv2d(F.silu(F.group_norm(h, G, sd["r.norm2.weight"], sd["r.norm2.bias"], EPS)), sd["r.conv2.weight"], sd["r.conv2.bias"], padding=1)
    ref = h + (F.conv2d(x, sd["r.conv_shortcut.weight"], sd["r.conv_shortcut.bias"]) if shortcut else x)
    return sd, x, shift, ref


def _emit(E, W, x, x2, shift, patch, fuse_gn=False):
    """graphs.emit_resnet recorded on a fresh engine -> (output, the conv ops' (name-less) meta rows)."""
    from genima_amd import graphs

    if shift is not None:  # the block's slice of a wider time-shift table (graphs._shift_for)
        table = torch.zeros(2, shift.shape[1] + 96, dtype=torch.float16, device="cuda")
        table[:, 32:32 + shift.shape[1]] = shift.half().cuda()
        W = dict(W)
        W["__meta__"] = {"temb_slices": {"r": (32, shift.shape[1])}}
        W["r.time_emb_proj.weight"] = table  # (only its presence is looked at)
    else:
        table = None
    E.conv_patch, E.conv_patch_min_rows, E.conv_patch_fuse_gn = patch, 0, fuse_gn
    y = graphs.emit_resnet(E, W, "r", x, x2, table, G, EPS)
    convs = [m for m in E.meta if m["kind"].startswith("conv")]
    E.run()
    E.synchronize()
    return y.float(), convs


@pytest.mark.parametrize("fuse_gn", [False, True])
def test_encoder_style_block_on_the_patch_route(engine, fuse_gn):
    """320 -> 320 with a time shift, B = 2, 16 x 32: conv1 (time shift) and conv2 (residual) both from the patch -- behind the GroupNorm launch
    (GN_CONV_PATCH_FUSE_GN=0) and with the GroupNorm applied inside the patch (the default)."""
    from genima_amd.engine import Engine

    sd, x, shift, ref = _block(320, 320, True, 21, False)
    W = packing.pack_state_dict(sd, "cuda")
    xd = _nhwc(x).half().cuda()
    y1, c1 = _emit(Engine("cuda:0", record=True, autotune=False), W, xd, None, shift, True, fuse_gn)
    y0, c0 = _emit(Engine("cuda:0", record=True, autotune=False), W, xd, None, shift, False)
    assert [m.get("route") for m in c1] == ["patch", "patch"] and [m.get("route") for m in c0] == [None, None]
    assert [(m["kind"], m["shape"]) for m in c1] == [(m["kind"], m["shape"]) for m in c0], "the per-op table keeps its rows"
    assert rel_l2(y1, y0) < 3e-4, rel_l2(y1, y0)
    assert rel_l2(_nchw(y1), ref) < 2e-3, rel_l2(_nchw(y1), ref)


@pytest.mark.parametrize("fuse_gn", [False, True])
def test_decoder_style_block_conv1_patch_conv2_k_append(engine, fuse_gn):
    """concat 320 + 320 -> 320 with conv_shortcut: conv1 on the patch route (on the GroupNorm launch's concatenation, or -- fuse_gn -- reading its two
    sources itself), conv2 + shortcut stay one k_append launch."""
    from genima_amd.engine import Engine

    sd, x, shift, ref = _block(640, 320, True, 22, True)
    W = packing.pack_state_dict(sd, "cuda")
    assert "r.conv2sc.weight" in W
    xd = _nhwc(x).half().cuda()
    xa, xb = xd[..., :320].contiguous(), xd[..., 320:].contiguous()
    y1, c1 = _emit(Engine("cuda:0", record=True, autotune=False), W, xa, xb, shift, True, fuse_gn)
    y0, c0 = _emit(Engine("cuda:0", record=True, autotune=False), W, xa, xb, shift, False)
    assert len(c1) == 2 and c1[0].get("route") == "patch" and c1[0]["shape"] == (1024, 320, 9 * 640)
    assert c1[1].get("route") is None and c1[1]["shape"] == (1024, 320, 9 * 320 + 640), "conv2 + conv_shortcut: one k_append launch"
    assert [(m["kind"], m["shape"]) for m in c1] == [(m["kind"], m["shape"]) for m in c0]
    assert rel_l2(y1, y0) < 3e-4, rel_l2(y1, y0)
    assert rel_l2(_nchw(y1), ref) < 2e-3, rel_l2(_nchw(y1), ref)


def test_default_gates_leave_a_b1_program_alone(engine, monkeypatch):
    """With the default gates a B = 1 program (64 x 64 x 320: 4096 rows) records exactly the ops of GN_CONV_PATCH=0."""
    from genima_amd import graphs
    from genima_amd.engine import Engine

    sd, _, _, _ = _block(320, 320, False, 23, False)
    W = packing.pack_state_dict(sd, "cuda")
    x = torch.randn(1, 64, 64, 320, device="cuda").half()
    kinds = []
    for env in ("1", "0"):
        monkeypatch.setenv("GN_CONV_PATCH", env)
        E = Engine("cuda:0", record=True, autotune=False)
        assert E.conv_patch == (env == "1") and E.conv_patch_min_rows == 32768
        graphs.emit_resnet(E, W, "r", x, None, None, G, EPS)
        kinds.append([(m["kind"], m["shape"], m.get("route")) for m in E.meta])
    assert kinds[0] == kinds[1]
