"""-m gpu: the small layout / elementwise kernels of csrc/elementwise.hip and csrc/backward.hip that no other test calls on their own
(gn_copy4d, gn_gather_rows, gn_argmax_rows_i32, gn_add_noise, gn_scale_cat_pad, gn_image_normalize_u8, gn_latent_sample, gn_fill_f32,
gn_reduce_rows_f32), each against a float64 / exact CPU reference from the same inputs (tests/act_ops_ref.py).  Bounds as in
tests/test_act_train_ops_gpu.py: moves are compared bit for bit, f16 outputs of a short f32 formula within
ulp16(ref64) + M32 * sum|terms|, the f32 row sums within n * 2^-24 * sum|t_i|."""
import pytest
import torch
import torch.nn.functional as F

import act_ops_ref as R
from genima_amd import train_ops as T
from genima_amd._lib import check

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAN = float("nan")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# measured on the CPU (act_ops_ref.m32_of over the inputs of this file), then x 4:
M32_ADD_NOISE = 4 * 1.06e-7   # add_noise_terms: 1.06e-7 -> 4.24e-7
M32_SCALE_CAT = 4 * 5.95e-8   # scale_cat_pad_terms (one product), Cpad 8 and 16: 5.95e-8 -> 2.38e-7
M32_NORMALIZE = 4 * 9.36e-8   # image_normalize_terms, every byte value x 3 channels, cpad 8 and 4: 9.36e-8 -> 3.74e-7
M32_LATENT = 4 * 1.31e-7      # latent_sample_terms, ld_eps 4 and 8: 1.31e-7 -> 5.24e-7


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _h(t):
    return t.to(F16)


def _guarded(shape, guard=64):
    """-> (NaN-filled f16 device tensor of ``shape``, the flat allocation it is the head of): ``guard`` more NaNs lie behind it."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + guard,), NAN, dtype=F16, device="cuda")
    return flat[:n].view(shape), flat


def _guard_intact(flat, n):
    return bool(torch.isnan(flat[n:]).all())


# ---- gn_copy4d ------------------------------------------------------------------------------------------------------------------------
class _NanEmpty:
    """Stands in for the ``torch`` name inside genima_amd.train_ops: its ``empty`` hands the wrapper a NaN-prefilled destination with a NaN
    guard band behind it (``flats`` keeps the whole allocations); everything else is torch's."""

    def __init__(self):
        self.flats = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        assert dtype == F16
        view, flat = _guarded(tuple(shape))
        self.flats.append(flat)
        return view


def test_concat_channels(engine, monkeypatch):
    g = _gen(40)
    a, b = _h(torch.randn(2, 3, 5, 8, generator=g)), _h(torch.randn(2, 3, 5, 24, generator=g))
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.concat_channels(engine, a.cuda(), b.cuda())
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr()
    assert R.bits_equal(out, torch.cat([a, b], -1))  # every element covered: no NaN is left
    assert _guard_intact(fake.flats[0], out.numel())


def test_upsample_nearest2x(engine, monkeypatch):
    x = _h(torch.randn(2, 3, 5, 16, generator=_gen(41)))
    fake = _NanEmpty()
    monkeypatch.setattr(T, "torch", fake)
    out = T.upsample_nearest2x(engine, x.cuda())
    assert len(fake.flats) == 1 and out.data_ptr() == fake.flats[0].data_ptr()
    ref = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).to(F16)
    assert R.bits_equal(out, ref)
    assert _guard_intact(fake.flats[0], out.numel())


def test_copy4d_generic_strides(engine):
    """Sizes (2, 3, 5, 7), runs of L = 16, eight distinct strides (all multiples of 8, the destination's leave gaps): any two axes or
    strides swapped lands somewhere else.  Both buffers are large enough for every assignment of these strides to these sizes."""
    sizes, L = (2, 3, 5, 7), 16
    ist, ost = (1840, 608, 120, 16), (2712, 896, 176, 24)
    span = 6 * (2712 + 1840 + 896 + 608) + L
    src = _h(torch.randn(span, generator=_gen(42)))
    want = torch.full((span + 64,), NAN, dtype=F16)
    for i0 in range(sizes[0]):
        for i1 in range(sizes[1]):
            for i2 in range(sizes[2]):
                for i3 in range(sizes[3]):
                    i = i0 * ist[0] + i1 * ist[1] + i2 * ist[2] + i3 * ist[3]
                    o = i0 * ost[0] + i1 * ost[1] + i2 * ost[2] + i3 * ost[3]
                    want[o:o + L] = src[i:i + L]
    dst, flat = _guarded((span,))
    engine.copy4d(src.cuda(), dst, sizes, ist, ost, L)
    assert R.bits_equal(flat, want)  # the runs, the NaN gaps between them and the guard band behind
    assert int((~torch.isnan(want)).sum()) == 2 * 3 * 5 * 7 * L


# ---- gathers ---------------------------------------------------------------------------------------------------------------------------
def test_gather_rows(engine):
    B, L, D = 4, 77, 40
    x = _h(torch.randn(B, L, D, generator=_gen(43)))
    idx = torch.tensor([0, L - 1, 31, 5], dtype=torch.int32)
    out = engine.gather_rows(x.cuda(), idx.cuda())
    assert R.bits_equal(out, x[torch.arange(B), idx.long()])


def test_argmax_rows_i32(engine):
    rows, cols = 70, 77
    x = torch.randint(-1000, 1000, (rows, cols), generator=_gen(44), dtype=torch.int32)
    x[0, :] = 7                                      # one long tie: index 0
    x[1, 10], x[1, 40], x[1, 76] = 5000, 5000, 5000  # ties: the first wins
    x[2, :] = torch.randint(-2 ** 31, -1, (cols,), generator=_gen(45), dtype=torch.int64).to(torch.int32)  # all negative
    x[3, 0] = 2 ** 31 - 1                            # maximum at column 0
    x[4, cols - 1] = 2 ** 31 - 1                     # maximum at the last column
    x[69, cols - 1], x[69, cols - 2] = 9000, 9000    # last row (second block of 64), tie at the end
    xl = x.long()
    ref = (xl == xl.max(1, keepdim=True).values).to(torch.int8).argmax(1).to(torch.int32)  # first index of the maximum
    assert ref[0] == 0 and ref[1] == 10 and ref[3] == 0 and ref[4] == cols - 1 and ref[69] == cols - 2
    out = engine.argmax_rows(x.cuda())
    assert out.dtype == torch.int32 and torch.equal(out.cpu(), ref)


# ---- short f32 formulas ---------------------------------------------------------------------------------------------------------------
def add_noise_inputs():
    g = _gen(46)
    B, n = 3, 1000
    x0, noise = _h(torch.randn(B, n, generator=g)), _h(torch.randn(B, n, generator=g))
    ac = torch.tensor([0.9991, 0.5, 0.0047])
    return x0, noise, ac.sqrt(), (1 - ac).sqrt()


@pytest.mark.parametrize("alias", [False, True])
def test_add_noise(engine, alias):
    x0, noise, a, c = add_noise_inputs()
    ref, terms = R.add_noise_terms(F64, x0, noise, a, c)
    print("m32 add_noise", R.m32_of(R.add_noise_terms, x0, noise, a, c))
    x0_d = x0.cuda()
    out, flat = (x0_d, None) if alias else _guarded(tuple(x0.shape))
    got = engine.add_noise(x0_d, noise.cuda(), a.cuda(), c.cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    R.assert_f16_formula(got, ref, terms, M32_ADD_NOISE, f"add_noise alias {alias}")
    if not alias:
        assert _guard_intact(flat, x0.numel()) and R.bits_equal(x0_d, x0)


def scale_cat_pad_inputs():
    g = _gen(47)
    return _h(torch.randn(300, 8, generator=g)), _h(torch.randn(300, 8, generator=g)), 0.18215, 1.0 / 14.6146


@pytest.mark.parametrize("cpad", [8, 16])
def test_scale_cat_pad(engine, cpad):
    x, x2, s1, s2 = scale_cat_pad_inputs()  # rows of width 8 of which 4 + 4 columns are taken
    ref, terms = R.scale_cat_pad_terms(F64, x, 4, x2, 4, cpad, s1, s2)
    print("m32 scale_cat_pad", R.m32_of(R.scale_cat_pad_terms, x, 4, x2, 4, cpad, s1, s2))
    out, flat = _guarded((300, cpad))
    engine.scale_cat_pad(x.cuda(), 4, x2.cuda(), 4, cpad, s1, s2, out=out)
    R.assert_f16_formula(out, ref, terms, M32_SCALE_CAT, f"scale_cat_pad cpad {cpad}")
    assert R.bits_equal(out[:, 8:], torch.zeros(300, cpad - 8, dtype=F16)) and _guard_intact(flat, 300 * cpad)
    assert s1 != s2  # two different scales: a swap of the two would show


def normalize_inputs():
    v = torch.arange(256, dtype=torch.uint8)
    img = torch.stack([v, v.flip(0), v.roll(101)], -1)  # every byte value in every channel
    tail = torch.randint(0, 256, (7, 3), generator=_gen(48), dtype=torch.uint8)
    return torch.cat([img, tail], 0)  # 256 + a ragged 7 pixels


@pytest.mark.parametrize("cpad", [8, 4])
def test_image_normalize_u8(engine, cpad):
    img = normalize_inputs()
    for c in range(3):
        assert len(set(img[:256, c].tolist())) == 256
    ref, terms = R.image_normalize_terms(F64, img, IMAGENET_MEAN, IMAGENET_STD, cpad)
    print("m32 normalize", R.m32_of(R.image_normalize_terms, img, IMAGENET_MEAN, IMAGENET_STD, cpad))
    out = engine.image_normalize_u8(img.cuda(), IMAGENET_MEAN, IMAGENET_STD, cpad)
    assert tuple(out.shape) == (263, cpad)
    R.assert_f16_formula(out, ref, terms, M32_NORMALIZE, f"image_normalize_u8 cpad {cpad}")
    assert R.bits_equal(out[:, 3:], torch.zeros(263, cpad - 3, dtype=F16))


def latent_inputs(ld_eps):
    g = _gen(49)
    P, Cl = 300, 4
    mom = _h(torch.randn(P, 8, generator=g))
    mom[:, Cl:] = _h(torch.randn(P, Cl, generator=g) * 3)
    mom[0:P:11, Cl + 1], mom[3:P:13, Cl + 2] = 25.0, -40.0  # beyond both clamp ends (-30, 20)
    eps = torch.full((P, ld_eps), NAN, dtype=F16)
    eps[:, :Cl] = _h(torch.randn(P, Cl, generator=g))
    return mom, eps


@pytest.mark.parametrize("ld_eps", [4, 8])
def test_latent_sample(engine, ld_eps):
    mom, eps = latent_inputs(ld_eps)
    scale = 0.18215
    ref, terms = R.latent_sample_terms(F64, mom, eps, 4, scale, 8)
    assert float(ref.abs().max()) < 65000 and float(mom[:, 4:].max()) == 25.0 and float(mom[:, 4:].min()) == -40.0
    print("m32 latent_sample", R.m32_of(R.latent_sample_terms, mom, eps, 4, scale, 8))
    out = T.latent_sample(engine, mom.cuda(), eps.cuda(), 4, scale, ld_out=8)
    assert tuple(out.shape) == (300, 8)
    R.assert_f16_formula(out, ref, terms, M32_LATENT, f"latent_sample ld_eps {ld_eps}")
    assert R.bits_equal(out[:, 4:], torch.zeros(300, 4, dtype=F16))


# ---- f32 fills and sums ---------------------------------------------------------------------------------------------------------------
def test_fill_f32(engine):
    flat = torch.full((1000 + 64,), NAN, dtype=F32, device="cuda")
    T.fill_f32(engine, flat[:1000], -2.5)
    assert R.bits_equal(flat[:1000], torch.full((1000,), -2.5)) and bool(torch.isnan(flat[1000:]).all())


def test_reduce_rows_f32_every_row_count(engine):
    """out[g][c] (+)= sum_r part[g][r][c] for every R in 1 .. 40 (the unrolled-by-16 loop's every remainder, four waves striding the rows),
    plain and accumulating; the partials end right where four rows of NaNs begin (a loop that runs one unrolled step too far reads them)."""
    groups, cols, Rmax = 2, 70, 40
    g = _gen(50)
    master = torch.randn(groups * Rmax * cols, generator=g)
    base = torch.randn(groups, cols, generator=g)
    base_d = base.cuda()
    for Rn in range(1, Rmax + 1):
        n_el = groups * Rn * cols
        part = torch.full((n_el + 4 * cols,), NAN, dtype=F32)
        part[:n_el] = master[:n_el]
        part_d = part.cuda()
        p64 = master[:n_el].view(groups, Rn, cols).double()
        for acc in (0, 1):
            out = torch.cat([base_d.view(-1), torch.full((64,), NAN, device="cuda")])
            check(engine.lib.gn_reduce_rows_f32(engine._ctx, part_d.data_ptr(), out.data_ptr(), groups, Rn, cols, acc), "gn_reduce_rows_f32")
            ref = p64.sum(1) + (base.double() if acc else 0)
            terms = p64.abs().sum(1) + (base.double().abs() if acc else 0)
            got = out.cpu()
            assert bool(torch.isnan(got[groups * cols:]).all()), (Rn, acc)
            R.assert_f32_sum(got[:groups * cols].view(groups, cols), ref, terms, R.cdiv(Rn, 4) + 4, 0.0, f"reduce_rows R {Rn} accumulate {acc}")
