"""-m gpu: every entry point of csrc/act_train.hip (plus gn_film's forward) on its own, against a float64 CPU reference evaluated from
the same f16-rounded / u8 inputs (tests/act_ops_ref.py: closed forms and torch autograd, nothing of genima_amd).

Bounds.  An f16 output of a short f32 formula: |got - ref64| <= ulp16(ref64) + M32 * sum|terms|.  The f32 loss sums:
|got - ref64| <= (n * 2^-24 + M32) * sum|t_i| with n the longest addition chain.  Moves and single-rounding ops: bit equality.  Each
M32_* is 4 x the worst |f32 - f64| / sum|terms| that act_ops_ref.m32_of measures for the same formula in torch float32 on the CPU on the
inputs built below (the factor covers the device's fast exp and FMA contraction) -- taken from the reference, never from a kernel's
output."""
import pytest
import torch

import act_ops_ref as R
from genima_amd import train_ops as T
from genima_amd._lib import ACT_NONE, ACT_RELU, ACT_SILU

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")

# measured on the CPU (m32_of over the inputs of this file), then x 4:
M32_FILM = 4 * 9.46e-8       # film_terms, worst of NONE 5.78e-8 / RELU 5.54e-8 / SILU 9.46e-8 -> 3.78e-7
M32_FILM_BWD = 4 * 0.0       # film_bwd_terms, NONE / RELU: 0.0 (dz * (1 + gamma) and dz * x are products of 11-bit factors: exact in f32) -> 0
M32_CVAE = 4 * 9.11e-8       # cvae_sample_terms, shapes 9.11e-8 / 6.55e-8 -> 3.64e-7
M32_CVAE_BWD = 4 * 1.43e-7   # cvae_bwd_terms, shapes 1.40e-7 / 1.43e-7 -> 5.72e-7
M32_LOSS = 4 * 7.51e-9       # act_loss_terms (terms in f32, summed in f64), worst of both layouts x mask x info: 7.51e-9 -> 3.00e-8
M32_LOSS_GRAD = 4 * 1.47e-7  # act_loss_grad_terms, worst of both layouts x mask: 1.47e-7 -> 5.88e-7
# warp_bilinear_terms: 0 on the zero / integer / half-pixel / edge fields (exact weights), 4.31e-6 / 1.05e-5 on the random +-3 px fields of
# the two shapes -- the f32 rounding of x + dx (half an ulp of a coordinate below 32: 9.5e-7 px) moves the weights by that much, which is
# large against sum w|v| wherever the four weighted taps are small -> 4.20e-5
M32_WARP = 4 * 1.05e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(t):
    return t.to(F16)


# ---- FiLM forward / backward ----------------------------------------------------------------------------------------------------------
FILM_B, FILM_ROWS, FILM_C = 3, 50, 24


def film_inputs():
    """x [150, 24], one [3, 64] FiLM buffer whose columns 8:32 / 32:56 are gamma / beta (NaN elsewhere), dy [150, 24].  gamma is a multiple
    of 2^-8 so that (1 + gamma) * x is exact in f32 and the sign of z is the same in f32 and f64; z == 0 exactly is planted two ways."""
    g = _gen(11)
    x = _h(torch.randn(FILM_B * FILM_ROWS, FILM_C, generator=g))
    film = torch.full((FILM_B, 64), NAN, dtype=F16)
    film[:, 8:32] = _h((torch.randn(FILM_B, FILM_C, generator=g) * 0.5 * 256).round().clamp(-512, 512) / 256)
    film[:, 32:56] = _h(torch.randn(FILM_B, FILM_C, generator=g))
    dy = _h(torch.randn(FILM_B * FILM_ROWS, FILM_C, generator=g))
    film[0, 8 + 3], film[0, 32 + 3], film[1, 32 + 5] = 1.0, -1.0, 0.0
    x[0:50:7, 3] = 0.5    # z = 2 * 0.5 - 1 = 0 (sample 0, channel 3)
    x[50:100:9, 5] = 0.0  # z = (1 + gamma) * 0 + 0 = 0 (sample 1, channel 5)
    return x, film, dy


@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_SILU])
def test_film_forward(engine, act):
    x, film, _ = film_inputs()
    gamma, beta = film[:, 8:32], film[:, 32:56]
    ref, terms = R.film_terms(F64, x, gamma, beta, FILM_ROWS, act)
    print("m32 film", R.m32_of(R.film_terms, x, gamma, beta, FILM_ROWS, act))
    fd = film.cuda()
    out = torch.full_like(x, NAN, device="cuda")
    engine.film(x.cuda(), fd[:, 8:32], fd[:, 32:56], FILM_ROWS, act, out=out)
    R.assert_f16_formula(out, ref, terms, M32_FILM, f"film act {act}")
    z0 = ((1 + gamma.double()).repeat_interleave(FILM_ROWS, 0) * x.double() + beta.double().repeat_interleave(FILM_ROWS, 0)) == 0
    assert int(z0.sum()) >= 14 and bool((out.cpu()[z0] == 0).all())


@pytest.mark.parametrize("with_copies", [True, False])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU])
def test_film_bwd(engine, act, with_copies):
    x, film, dy = film_inputs()
    gamma, beta = film[:, 8:32], film[:, 32:56]
    dx_ref, dz_ref = R.film_autograd(x, gamma, beta, FILM_ROWS, act, dy)
    dzx_ref = dz_ref * x.double()
    print("m32 film_bwd", R.m32_of(R.film_bwd_terms, dy, x, gamma, beta, FILM_ROWS, act))
    fd = film.cuda()
    dx = torch.full_like(x, NAN, device="cuda")
    dz, dzx = (torch.full_like(dx, NAN), torch.full_like(dx, NAN)) if with_copies else (None, None)
    T.film_bwd(engine, dy.cuda(), x.cuda(), fd[:, 8:32], fd[:, 32:56], FILM_ROWS, act, dx, dz, dzx)
    R.assert_f16_formula(dx, dx_ref, dx_ref.abs(), M32_FILM_BWD, f"film_bwd dx act {act}")
    if with_copies:
        R.assert_f16_formula(dz, dz_ref, dz_ref.abs(), M32_FILM_BWD, f"film_bwd dz act {act}")
        R.assert_f16_formula(dzx, dzx_ref, dzx_ref.abs(), M32_FILM_BWD, f"film_bwd dzx act {act}")
    if act == ACT_RELU:  # relu'(0) = 0 at the planted exact zeros (torch's convention and the kernel's z <= 0)
        z0 = ((1 + gamma.double()).repeat_interleave(FILM_ROWS, 0) * x.double() + beta.double().repeat_interleave(FILM_ROWS, 0)) == 0
        assert int(z0.sum()) >= 14 and bool((dx_ref[z0] == 0).all()) and bool((dx.cpu()[z0] == 0).all())


def test_film_bwd_refuses_other_activations(engine):
    x, film, dy = film_inputs()
    fd, xd, dyd = film.cuda(), x.cuda(), dy.cuda()
    dx = torch.full_like(xd, NAN)
    rc = engine.lib.gn_film_bwd(engine._ctx, dyd.data_ptr(), xd.data_ptr(), fd[:, 8:32].data_ptr(), fd[:, 32:56].data_ptr(), 64, FILM_ROWS,
                                x.shape[0], FILM_C, ACT_SILU, dx.data_ptr(), None, None)
    assert rc != 0, "gn_film_bwd implements NONE / RELU only: anything else must be an error, not a launch"
    assert bool(torch.isnan(dx).all())


# ---- dropout / add_f32_to_f16: the same IEEE operations as the reference, bit for bit -------------------------------------------------
def test_dropout_bits(engine):
    g = _gen(12)
    n, keep_p = 1000, 0.9
    x = _h(torch.randn(n, generator=g))
    mask = (torch.rand(n, generator=g) < keep_p).to(torch.uint8)
    assert 0 < int(mask.sum()) < n
    scale = 1.0 / keep_p
    ref = torch.where(mask.bool(), (x.float() * torch.tensor(scale, dtype=F32)).half(), torch.zeros(n, dtype=F16))
    out = T.dropout(engine, x.cuda(), mask.cuda(), scale)
    assert R.bits_equal(out, ref)  # +0 exactly where the mask drops, -0 included where x * scale is -0


def test_add_f32_to_f16_bits(engine):
    g = _gen(13)
    B, C, ld_src, ld_dst = 3, 20, 24, 40
    src = torch.randn(B, ld_src, generator=g)
    src[:, C:] = NAN  # the padding of the sums is not to be read
    dst = _h(torch.randn(B, ld_dst, generator=g))
    ref = dst.clone()
    ref[:, :C] = (dst[:, :C].float() + src[:, :C]).half()
    d = dst.cuda().view(-1)
    T.add_f32_to_f16(engine, src.cuda(), d, ld_dst, B, C)
    assert R.bits_equal(d.view(B, ld_dst), ref)  # columns >= C untouched


# ---- CVAE reparametrisation -----------------------------------------------------------------------------------------------------------
CVAE_SHAPES = [(5, 32, 64, 32), (3, 20, 72, 24)]  # (B, L, ld_info, ldz)


def cvae_inputs(B, L, ld_info, ldz):
    g = _gen(14 + B)
    info = torch.full((B, ld_info), NAN, dtype=F16)
    info[:, :L] = _h(torch.randn(B, L, generator=g))
    lv = torch.linspace(-6.0, 4.0, B * L)[torch.randperm(B * L, generator=g)].view(B, L)
    info[:, L:2 * L] = _h(lv)
    if ld_info > 2 * L:
        info[:, 2 * L:] = 0.5  # finite filler: cvae_bwd's wrapper returns zeros there whatever the kernel does with it
    eps = torch.randn(B, L, generator=g)
    dz = torch.full((B, ldz), NAN, dtype=F16)
    dz[:, :L] = _h(torch.randn(B, L, generator=g))
    return info, eps, dz


@pytest.mark.parametrize("B,L,ld_info,ldz", CVAE_SHAPES)
def test_cvae_sample(engine, B, L, ld_info, ldz):
    info, eps, _ = cvae_inputs(B, L, ld_info, ldz)
    assert float(info[:, L:2 * L].min()) == -6.0 and float(info[:, L:2 * L].max()) == 4.0
    ref, terms = R.cvae_sample_terms(F64, info, eps, L)
    print("m32 cvae_sample", R.m32_of(R.cvae_sample_terms, info, eps, L))
    z = T.cvae_sample(engine, info.cuda(), eps.cuda(), L, ldz)
    assert tuple(z.shape) == (B, ldz)
    R.assert_f16_formula(z[:, :L], ref, terms, M32_CVAE, "cvae_sample")
    assert bool((z[:, L:] == 0).all())


@pytest.mark.parametrize("B,L,ld_info,ldz", CVAE_SHAPES)
def test_cvae_bwd(engine, B, L, ld_info, ldz):
    info, eps, dz = cvae_inputs(B, L, ld_info, ldz)
    kl_scale = 256.0 * 10.0 / B  # loss_scale * kl_weight / B
    ref = R.cvae_bwd_autograd(info, eps, dz[:, :L], L, kl_scale)
    closed, terms = R.cvae_bwd_terms(F64, info, eps, dz[:, :L], L, kl_scale)
    assert float((closed - ref).abs().max()) <= 1e-12 * float(terms.max())  # the terms belong to the formula autograd differentiates
    print("m32 cvae_bwd", R.m32_of(R.cvae_bwd_terms, info, eps, dz[:, :L], L, kl_scale))
    dinfo = T.cvae_bwd(engine, info.cuda(), eps.cuda(), dz.cuda(), L, kl_scale)
    assert tuple(dinfo.shape) == (B, ld_info)
    R.assert_f16_formula(dinfo[:, :2 * L], ref, terms, M32_CVAE_BWD, "cvae_bwd")
    assert bool((dinfo[:, 2 * L:] == 0).all())


# ---- calculate_loss -------------------------------------------------------------------------------------------------------------------
LOSS_B, LOSS_T, LOSS_TR, LOSS_L, LOSS_LD_INFO, KL_WEIGHT, GRAD_SCALE = 3, 20, 24, 32, 72, 10.0, 256.0
LOSS_LAYOUTS = [(8, 8, 0), (7, 16, 32)]  # (A, ld, bs_hat - T_rows * ld)


def loss_inputs(A):
    g = _gen(20 + A)
    B, T_ = LOSS_B, LOSS_T
    a_hat = _h(torch.randn(B, T_, A, generator=g))
    actions = torch.randn(B, T_, A, generator=g)
    actions[0, :5, :3] = a_hat[0, :5, :3].float()  # exact L1 ties: sign 0
    actions[1, 15:, 1] = a_hat[1, 15:, 1].float()
    a_hat[..., -1] = _h(torch.randn(B, T_, generator=g) * 2)
    a_hat[0, 0, -1], a_hat[0, 1, -1], a_hat[0, 2, -1], a_hat[0, 3, -1], a_hat[0, 4, -1] = 0.0, 30.0, -30.0, 30.0, -30.0
    a_hat[1, 0, -1], a_hat[1, 1, -1] = 0.0, 30.0
    actions[..., -1] = (torch.rand(B, T_, generator=g) < 0.5).float()
    actions[0, :5, -1] = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0])  # logits 0 / +30 / -30 against both targets
    actions[1, :2, -1] = torch.tensor([0.0, 0.0])
    info = torch.full((B, LOSS_LD_INFO), NAN, dtype=F16)
    info[:, :LOSS_L] = _h(torch.randn(B, LOSS_L, generator=g))
    info[:, LOSS_L:2 * LOSS_L] = _h(torch.randn(B, LOSS_L, generator=g) * 1.5)
    is_pad = torch.zeros(B, T_, dtype=torch.bool)
    is_pad[1, 14:] = True  # the tail of one sample
    is_pad[2, :] = True    # all of another
    return a_hat, actions, info, is_pad


def _run_act_loss(E, a_hat, actions, info, is_pad, A, ld, gap):
    """-> (out4, d_a_hat flat with a NaN guard): gn_act_loss on a padded [B][T_rows][ld] a_hat of batch stride T_rows * ld + gap whose
    padding is NaN (never to be read), into a NaN-prefilled d_a_hat."""
    B, T_, Tr = LOSS_B, LOSS_T, LOSS_TR
    bs = Tr * ld + gap
    buf = torch.full((B, bs), NAN, dtype=F16)
    buf[:, :Tr * ld].view(B, Tr, ld)[:, :T_, :A] = a_hat
    a_d, act_d = buf.cuda(), actions.cuda()
    d = torch.full((B * bs + 64,), NAN, dtype=F16, device="cuda")
    out4 = torch.full((4,), NAN, dtype=F32, device="cuda")
    pad_d = None if is_pad is None else is_pad.to(torch.uint8).cuda()
    info_d = None if info is None else info.cuda()
    rc = E.lib.gn_act_loss(E._ctx, a_d.data_ptr(), ld, bs, act_d.data_ptr(), None if pad_d is None else pad_d.data_ptr(),
                           None if info_d is None else info_d.data_ptr(), LOSS_LD_INFO, B, T_, Tr, A, LOSS_L, KL_WEIGHT, GRAD_SCALE,
                           out4.data_ptr(), d.data_ptr())
    assert rc == 0, E.lib.gn_last_error()
    return out4.cpu(), d.cpu()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A,ld,gap", LOSS_LAYOUTS)
def test_act_loss(engine, A, ld, gap, masked):
    a_hat, actions, info, is_pad = loss_inputs(A)
    is_pad = is_pad if masked else None
    B, T_, Tr = LOSS_B, LOSS_T, LOSS_TR
    assert int((a_hat[..., :-1].float() == actions[..., :-1]).sum()) >= 20
    ref4, grad = R.act_loss_autograd(a_hat, actions, is_pad, info, LOSS_L, KL_WEIGHT)
    chk4, terms4 = R.act_loss_terms(F64, a_hat, actions, is_pad, info, LOSS_L, KL_WEIGHT)
    assert float(((chk4 - ref4).abs() / terms4).max()) <= 1e-13  # the terms are those of the sums autograd differentiates
    gchk, gterms = R.act_loss_grad_terms(F64, a_hat, actions, is_pad, GRAD_SCALE)
    assert float((gchk - GRAD_SCALE * grad).abs().max()) <= 1e-13 * float(gterms.max())
    print("m32 act_loss", R.m32_of(R.act_loss_terms, a_hat, actions, is_pad, info, LOSS_L, KL_WEIGHT),
          "grad", R.m32_of(R.act_loss_grad_terms, a_hat, actions, is_pad, GRAD_SCALE))
    out4, d = _run_act_loss(engine, a_hat, actions, info, is_pad, A, ld, gap)
    n = R.cdiv(B * Tr * ld, 256) + 8
    R.assert_f32_sum(out4, ref4, terms4, n, M32_LOSS, f"act_loss out4 A {A} ld {ld} masked {masked}")
    bs = Tr * ld + gap
    dd = d[:B * bs].view(B, bs)
    dm = dd[:, :Tr * ld].reshape(B, Tr, ld)
    R.assert_f16_formula(dm[:, :T_, :A], GRAD_SCALE * grad, gterms, M32_LOSS_GRAD, "act_loss d_a_hat")
    ties = a_hat[..., :-1].float() == actions[..., :-1]
    assert bool((dm[:, :T_, :A - 1][ties] == 0).all()), "an exact L1 tie has gradient 0"
    if masked:
        assert bool((dm[1, 14:T_, :A] == 0).all()) and bool((dm[2, :T_, :A] == 0).all()) and bool((dm[1, :14, :A - 1][~ties[1, :14]] != 0).all())
    # the padding of d_a_hat is written with exact zeros; whatever lies between one sample's rows and the next sample is not touched
    assert R.bits_equal(dm[:, T_:, :], torch.zeros(B, Tr - T_, ld, dtype=F16)), "rows [T, T_rows) of d_a_hat must be +0"
    assert R.bits_equal(dm[:, :, A:], torch.zeros(B, Tr, ld - A, dtype=F16)), "columns [A, ld) of d_a_hat must be +0"
    assert R.bits_equal(dd[:, Tr * ld:], torch.full((B, gap), NAN, dtype=F16)), "bytes between T_rows * ld and bs_hat must stay as they were"
    assert R.bits_equal(d[B * bs:], torch.full((64,), NAN, dtype=F16)), "wrote past the last sample"


def test_act_loss_without_info(engine):
    A, ld, gap = LOSS_LAYOUTS[1]
    a_hat, actions, _, is_pad = loss_inputs(A)
    ref4, grad = R.act_loss_autograd(a_hat, actions, is_pad, None, LOSS_L, KL_WEIGHT)
    _, terms4 = R.act_loss_terms(F64, a_hat, actions, is_pad, None, LOSS_L, KL_WEIGHT)
    _, gterms = R.act_loss_grad_terms(F64, a_hat, actions, is_pad, GRAD_SCALE)
    out4, d = _run_act_loss(engine, a_hat, actions, None, is_pad, A, ld, gap)
    assert float(out4[3]) == 0.0, "no info: kl is exactly 0"
    R.assert_f32_sum(out4[:3], ref4[:3], terms4[:3], R.cdiv(LOSS_B * LOSS_TR * ld, 256) + 8, M32_LOSS, "act_loss out4, info=None")
    dm = d[:LOSS_B * (LOSS_TR * ld + gap)].view(LOSS_B, -1)[:, :LOSS_TR * ld].reshape(LOSS_B, LOSS_TR, ld)
    R.assert_f16_formula(dm[:, :LOSS_T, :A], GRAD_SCALE * grad, gterms, M32_LOSS_GRAD, "act_loss d_a_hat, info=None")


# ---- bilinear warp --------------------------------------------------------------------------------------------------------------------
WARP_SHAPES = [(2, 13, 17, 8), (1, 16, 16, 16)]


def warp_inputs(B, H, W, C):
    g = _gen(30 + H)
    img = _h(torch.randn(B, H, W, C, generator=g))
    zero = torch.zeros(H, W, 2)
    shift = zero.clone()
    shift[..., 0], shift[..., 1] = 2.0, -1.0
    half = torch.full((H, W, 2), 0.5)
    edge = zero.clone()
    edge[:, 0, 0] = -1.0      # column 0 samples x = -1 exactly: outside
    edge[:, W - 3, 0] = 2.0   # column W - 3 lands exactly on W - 1: that pixel, with no weight on the column beyond
    edge[0, 1:W - 3, 1] = -1.0  # row 0 samples y = -1 exactly
    edge[H - 2, 1:W - 3, 1] = 1.0  # row H - 2 lands exactly on H - 1
    outside = torch.full((H, W, 2), float(W + H + 5))
    rnd = torch.rand(H, W, 2, generator=g) * 6 - 3
    return img, dict(zero=zero, shift=shift, half=half, edge=edge, outside=outside, rnd=rnd)


def _warp(E, img_d, disp):
    out = torch.full_like(img_d, NAN)
    disp_d = disp.contiguous().cuda()
    B, H, W, C = img_d.shape
    rc = E.lib.gn_warp_bilinear(E._ctx, img_d.data_ptr(), out.data_ptr(), disp_d.data_ptr(), B, H, W, C)
    assert rc == 0, E.lib.gn_last_error()
    return out.cpu()


@pytest.mark.parametrize("B,H,W,C", WARP_SHAPES)
def test_warp_bilinear(engine, B, H, W, C):
    img, fields = warp_inputs(B, H, W, C)
    img_d = img.cuda()
    print("m32 warp", max(R.m32_of(R.warp_bilinear_terms, img, fields[k]) for k in ("half", "rnd")))
    for name, disp in fields.items():
        got = _warp(engine, img_d, disp)
        ref = R.grid_sample_warp(img, disp)          # F.grid_sample in f64, grid from pixel coordinates
        ref2, terms = R.warp_bilinear_terms(F64, img, disp)  # the plain four-tap sampler
        assert float((ref - ref2).abs().max()) <= 1e-12, name
        R.assert_f16_formula(got, ref, terms, M32_WARP, f"warp {name} vs grid_sample")
        R.assert_f16_formula(got, ref2, terms, M32_WARP, f"warp {name} vs plain sampler")
        if name == "zero":
            assert R.bits_equal(got, img)
        elif name == "shift":
            want = torch.zeros_like(img)
            want[:, 1:, :W - 2] = img[:, :H - 1, 2:]
            assert R.bits_equal(got, want)
        elif name == "edge":
            assert bool((got[:, :, 0] == 0).all()) and bool((got[:, 0, 1:W - 3] == 0).all())
            assert torch.equal(got[:, 1:H - 2, W - 3], img[:, 1:H - 2, W - 1]) and torch.equal(got[:, H - 2, 1:W - 3], img[:, H - 1, 1:W - 3])
        elif name == "outside":
            assert R.bits_equal(got, torch.zeros_like(img))
        else:
            assert float(got.abs().max()) > 0


def test_warp_bilinear_refuses_aliasing(engine):
    img, fields = warp_inputs(*WARP_SHAPES[0])
    img_d, disp_d = img.cuda(), fields["rnd"].cuda()
    B, H, W, C = img.shape
    rc = engine.lib.gn_warp_bilinear(engine._ctx, img_d.data_ptr(), img_d.data_ptr(), disp_d.data_ptr(), B, H, W, C)
    assert rc != 0, "in == out would read pixels another thread has already overwritten"
    assert R.bits_equal(img_d, img)
