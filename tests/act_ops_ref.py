"""CPU references for the per-kernel parity tests of the ACT-update and small layout kernels (tests/test_act_train_ops_gpu.py,
tests/test_small_ops_gpu.py, tests/test_act_augment_cpu.py).

TEST INFRASTRUCTURE ONLY.  Every function here is a closed-form torch expression (or torch autograd) evaluated on the CPU from the
kernel's own f16-rounded / u8 / i32 inputs; none of it goes through genima_amd.  A ``*_terms`` function takes the working dtype
first: float64 gives the reference, float32 restates the kernel's f32 arithmetic so that ``m32_of`` can measure how far plain
f32 evaluation strays from the f64 value on a test's inputs (the tests' M32_* constants are 4 x that figure: the factor covers the
device's fast exp and FMA contraction, which the CPU restatement does not have).  Each returns (value, sum of |terms|): the error
bounds are relative to the magnitude of what was added up, not to the (possibly cancelled) result.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
F64 = torch.float64
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 4  # include/genima_hip.h


# ---- error bounds ------------------------------------------------------------------------------------------------------------------
def ulp16(ref: Tensor) -> Tensor:
    """Spacing of the f16 grid just above |half(ref)|: the distance from the correctly rounded f16 value of ``ref`` to its farther
    neighbour (2^-24 in the subnormal range)."""
    a = ref.to(torch.float16).to(F64).abs()
    _, e = torch.frexp(a)  # a = m * 2^e, m in [0.5, 1)
    e = torch.where(a == 0, torch.full_like(e, -13), e).clamp_min(-13)
    return torch.ldexp(torch.ones_like(a), e - 11)


def assert_f16_formula(got: Tensor, ref: Tensor, terms: Tensor, m32: float, what: str = ""):
    """|got - ref64| <= ulp16(ref64) + m32 * sum|terms|: the kernel's f32 value is within m32 * sum|terms| of the exact one, so its f16
    rounding is the correctly rounded value or that value's neighbour."""
    got, ref, terms = got.detach().cpu().to(F64), ref.detach().to(F64), terms.detach().to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err, bound = (got - ref).abs(), ulp16(ref) + m32 * terms
    worst = int((err - bound).argmax())
    print(f"{what}: max err/bound {float((err / bound).max()):.3f}, max |err| {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (f"{what}: |got - ref| {float(err.flatten()[worst]):.6e} > bound {float(bound.flatten()[worst]):.6e} at flat "
                                        f"index {worst} (got {float(got.flatten()[worst])!r}, ref {float(ref.flatten()[worst])!r})")


def assert_f32_sum(got: Tensor, ref: Tensor, terms: Tensor, n: int, m32: float = 0.0, what: str = ""):
    """|got - ref64| <= n * 2^-24 * sum|t_i| (+ m32 * sum|t_i|): an f32 sum whose longest addition chain has ``n`` links."""
    got, ref, terms = got.detach().cpu().to(F64), ref.detach().to(F64), terms.detach().to(F64)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err, bound = (got - ref).abs(), (n * 2.0 ** -24 + m32) * terms
    print(f"{what}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, max |err| {float(err.max()):.3e}")
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), (f"{what}: |got - ref| {float(err.flatten()[worst]):.6e} > bound {float(bound.flatten()[worst]):.6e} at flat "
                                        f"index {worst} (got {float(got.flatten()[worst])!r}, ref {float(ref.flatten()[worst])!r})")


def m32_of(fn, *args, **kw) -> float:
    """Worst |f32 evaluation - f64 evaluation| / sum|terms| of ``fn(dtype, *args)`` -> (value, terms) (or a list of such pairs)."""
    r64, r32 = fn(F64, *args, **kw), fn(torch.float32, *args, **kw)
    if isinstance(r64, tuple):
        r64, r32 = [r64], [r32]
    worst = 0.0
    for (v64, t64), (v32, _) in zip(r64, r32):
        rel = (v32.to(F64) - v64).abs() / t64.clamp_min(1e-300)
        worst = max(worst, float(rel[t64 > 0].max()) if bool((t64 > 0).any()) else 0.0)
    return worst


def bits_equal(a: Tensor, b: Tensor) -> bool:
    """Bit equality of two f16 / f32 tensors (NaN payloads and the sign of zero included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ---- FiLM --------------------------------------------------------------------------------------------------------------------------
def _act(z: Tensor, act: int) -> Tensor:
    return {ACT_NONE: lambda v: v, ACT_RELU: torch.relu, ACT_SILU: lambda v: v * torch.sigmoid(v)}[act](z)


def film_terms(dt, x: Tensor, gamma: Tensor, beta: Tensor, rows_per_film: int, act: int):
    """y = act((1 + gamma[b]) * x + beta[b]), b = row // rows_per_film; x [rows, C], gamma / beta [B, C]."""
    g1 = (1 + gamma.to(dt)).repeat_interleave(rows_per_film, 0)
    b = beta.to(dt).repeat_interleave(rows_per_film, 0)
    p = g1 * x.to(dt)
    # |d silu / dz| <= 1.1: an error in z reaches y scaled by at most that
    return _act(p + b, act), (p.abs() + b.abs()) * (1.1 if act == ACT_SILU else 1.0)


def film_autograd(x: Tensor, gamma: Tensor, beta: Tensor, rows_per_film: int, act: int, dy: Tensor):
    """-> (dx, dz): f64 autograd of act(z), z = (1 + gamma_b) x + beta_b, seeded with dy; dz is the gradient at the pre-activation."""
    x64 = x.to(F64).requires_grad_(True)
    z = (1 + gamma.to(F64)).repeat_interleave(rows_per_film, 0) * x64 + beta.to(F64).repeat_interleave(rows_per_film, 0)
    z.retain_grad()
    _act(z, act).backward(dy.to(F64))
    return x64.grad, z.grad


def film_bwd_terms(dt, dy: Tensor, x: Tensor, gamma: Tensor, beta: Tensor, rows_per_film: int, act: int):
    """Closed form of the backward -> [(dx, |dx|), (dz, |dz|), (dzx, |dzx|)] (each a single product)."""
    g1 = (1 + gamma.to(dt)).repeat_interleave(rows_per_film, 0)
    z = g1 * x.to(dt) + beta.to(dt).repeat_interleave(rows_per_film, 0)
    dz = dy.to(dt) * (z > 0).to(dt) if act == ACT_RELU else dy.to(dt)
    dx, dzx = dz * g1, dz * x.to(dt)
    return [(dx, dx.abs()), (dz, dz.abs()), (dzx, dzx.abs())]


# ---- CVAE reparametrisation ---------------------------------------------------------------------------------------------------------
def cvae_sample_terms(dt, info: Tensor, eps: Tensor, L: int):
    mu, lv = info[:, :L].to(dt), info[:, L:2 * L].to(dt)
    n = torch.exp(lv / 2) * eps.to(dt)
    return mu + n, mu.abs() + n.abs()


def cvae_bwd_autograd(info: Tensor, eps: Tensor, dz: Tensor, L: int, kl_scale: float) -> Tensor:
    """f64 autograd of sum(z * dz) + kl_scale * sum_b KL_b with respect to info[:, :2L]."""
    i64 = info[:, :2 * L].to(F64).clone().requires_grad_(True)
    mu, lv = i64[:, :L], i64[:, L:]
    z = mu + torch.exp(lv / 2) * eps.to(F64)
    kl = (-0.5 * (1 + lv - mu * mu - torch.exp(lv))).sum()
    ((z * dz.to(F64)).sum() + kl_scale * kl).backward()
    return i64.grad


def cvae_bwd_terms(dt, info: Tensor, eps: Tensor, dz: Tensor, L: int, kl_scale: float):
    """Closed form -> (dinfo [B, 2L], terms)."""
    mu, lv, g = info[:, :L].to(dt), info[:, L:2 * L].to(dt), dz.to(dt)
    s = torch.exp(lv / 2)
    a, b = 0.5 * g * eps.to(dt) * s, 0.5 * kl_scale * (s * s - 1)
    return (torch.cat([g + kl_scale * mu, a + b], 1),
            torch.cat([g.abs() + (kl_scale * mu).abs(), a.abs() + 0.5 * kl_scale * (s * s + 1)], 1))


# ---- calculate_loss -----------------------------------------------------------------------------------------------------------------
def act_loss_autograd(a_hat: Tensor, actions: Tensor, is_pad, info, L: int, kl_weight: float):
    """``calculate_loss`` in f64 with autograd.  a_hat [B, T, A] (f16 values), actions f32 [B, T, A], is_pad bool [B, T] or None, info
    [B, >= 2L] or None -> (out4 = (loss, l1, gripper, kl), d(l1 + gripper) / d a_hat)."""
    x = a_hat.to(F64).clone().requires_grad_(True)
    y = actions.to(F64)
    keep = torch.ones(x.shape[:2], dtype=F64) if is_pad is None else (~is_pad).to(F64)
    l1 = (F.l1_loss(x[..., :-1], y[..., :-1], reduction="none") * keep[..., None]).mean()
    grip = (0.05 * F.binary_cross_entropy_with_logits(x[..., -1], y[..., -1], reduction="none") * keep).mean()
    if info is None:
        kl = torch.zeros((), dtype=F64)
    else:
        mu, lv = info[:, :L].to(F64), info[:, L:2 * L].to(F64)
        kl = (-0.5 * (1 + lv - mu * mu - torch.exp(lv))).sum(1).mean()
    (l1 + grip).backward()
    return torch.stack([l1 + grip + kl * kl_weight, l1, grip, kl]).detach(), x.grad


def act_loss_terms(dt, a_hat: Tensor, actions: Tensor, is_pad, info, L: int, kl_weight: float):
    """The per-element terms of the four outputs evaluated in ``dt`` and summed in f64 (so that only the term arithmetic, not the
    summation order, separates dt = float32 from float64) -> (out4, sum|t_i| of each output)."""
    x, y = a_hat.to(dt), actions.to(dt)
    B, T, A = x.shape
    keep = torch.ones(B, T, dtype=dt) if is_pad is None else (~is_pad).to(dt)
    t1 = ((x[..., :-1] - y[..., :-1]).abs() * keep[..., None]).to(F64) / (B * T * (A - 1))
    xg, yg = x[..., -1], y[..., -1]
    pos = [torch.clamp_min(xg, 0), torch.log1p(torch.exp(-xg.abs())), (xg * yg).abs()]
    tg = (0.05 * (pos[0] - xg * yg + pos[1]) * keep).to(F64) / (B * T)
    tg_abs = (0.05 * (pos[0] + pos[1] + pos[2]) * keep).to(F64) / (B * T)
    if info is None:
        tk = tk_abs = torch.zeros(1, dtype=F64)
    else:
        mu, lv = info[:, :L].to(dt), info[:, L:2 * L].to(dt)
        tk = (-0.5 * (1 + lv - mu * mu - torch.exp(lv))).to(F64) / B
        tk_abs = (0.5 * (1 + lv.abs() + mu * mu + torch.exp(lv))).to(F64) / B
    s1, sg, sk = t1.sum(), tg.sum(), tk.sum()
    a1, ag, ak = t1.abs().sum(), tg_abs.sum(), tk_abs.sum()
    return torch.stack([s1 + sg + sk * kl_weight, s1, sg, sk]), torch.stack([a1 + ag + ak * kl_weight, a1, ag, ak])


def act_loss_grad_terms(dt, a_hat: Tensor, actions: Tensor, is_pad, grad_scale: float):
    """Closed form of grad_scale * d(l1 + gripper) / d a_hat -> (grad, terms)."""
    x, y = a_hat.to(dt), actions.to(dt)
    B, T, A = x.shape
    keep = torch.ones(B, T, dtype=dt) if is_pad is None else (~is_pad).to(dt)
    g1 = torch.sign(x[..., :-1] - y[..., :-1]) * keep[..., None] / (B * T * (A - 1)) * grad_scale
    sg = torch.sigmoid(x[..., -1])
    gg = 0.05 * (sg - y[..., -1]) * keep / (B * T) * grad_scale
    gg_abs = 0.05 * (sg + y[..., -1].abs()) * keep / (B * T) * grad_scale
    return torch.cat([g1, gg[..., None]], -1), torch.cat([g1.abs(), gg_abs[..., None]], -1)


# ---- bilinear warp ------------------------------------------------------------------------------------------------------------------
def warp_bilinear_terms(dt, img: Tensor, disp: Tensor):
    """Plain bilinear, zero-fill sampler: out[b, y, x, :] = bilinear(img[b], x + disp[y, x, 0], y + disp[y, x, 1]); img [B, H, W, C], disp
    [H, W, 2] in pixels.  The four taps are gathered by index: no grid_sample, no normalised coordinates."""
    img, disp = img.to(dt), disp.to(dt)
    B, H, W, C = img.shape
    sx = torch.arange(W, dtype=dt)[None, :] + disp[..., 0]
    sy = torch.arange(H, dtype=dt)[:, None] + disp[..., 1]
    fx, fy = torch.floor(sx), torch.floor(sy)
    ax, ay = sx - fx, sy - fy
    out, terms = torch.zeros_like(img), torch.zeros_like(img)
    for t in range(4):
        xx, yy = (fx + (t & 1)).long(), (fy + (t >> 1)).long()
        w = (ax if t & 1 else 1 - ax) * (ay if t >> 1 else 1 - ay)
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = img[:, yy.clamp(0, H - 1), xx.clamp(0, W - 1), :] * (w * ok.to(dt))[None, :, :, None]
        out, terms = out + v, terms + v.abs()
    return out, terms


def warp_bilinear(img: Tensor, disp: Tensor) -> Tensor:
    return warp_bilinear_terms(F64, img, disp)[0]


def grid_sample_warp(img: Tensor, disp: Tensor) -> Tensor:
    """The same warp through F.grid_sample in f64 (bilinear, zeros, align_corners=False) with the grid built from pixel coordinates as
    g = (2 (x + dx) + 1) / W - 1 (and likewise for y); img [B, H, W, C] -> [B, H, W, C]."""
    img, disp = img.to(F64), disp.to(F64)
    B, H, W, C = img.shape
    gx = (2 * (torch.arange(W, dtype=F64)[None, :] + disp[..., 0]) + 1) / W - 1
    gy = (2 * (torch.arange(H, dtype=F64)[:, None] + disp[..., 1]) + 1) / H - 1
    grid = torch.stack([gx, gy], -1)[None].expand(B, H, W, 2)
    out = F.grid_sample(img.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out.permute(0, 2, 3, 1).contiguous()


# ---- short elementwise formulas -----------------------------------------------------------------------------------------------------
def add_noise_terms(dt, x0: Tensor, noise: Tensor, a: Tensor, c: Tensor):
    """out[b] = a[b] * x0[b] + c[b] * noise[b]; x0 / noise [B, n], a / c f32 [B]."""
    p, q = a.to(dt)[:, None] * x0.to(dt), c.to(dt)[:, None] * noise.to(dt)
    return p + q, p.abs() + q.abs()


def scale_cat_pad_terms(dt, x: Tensor, c1: int, x2: Tensor, c2: int, cpad: int, scale: float, scale2: float):
    """[x[:, :c1] * scale | x2[:, :c2] * scale2 | 0 ...] -> [pixels, cpad] (the scales as the f32 values the kernel receives)."""
    s1, s2 = torch.tensor(scale, dtype=torch.float32).to(dt), torch.tensor(scale2, dtype=torch.float32).to(dt)
    out = torch.zeros(x.shape[0], cpad, dtype=dt)
    out[:, :c1], out[:, c1:c1 + c2] = x[:, :c1].to(dt) * s1, x2[:, :c2].to(dt) * s2
    return out, out.abs()


def image_normalize_terms(dt, img: Tensor, mean, std, cpad: int):
    """uint8 [pixels, 3] -> [pixels, cpad]: (v / 255 - mean_c) / std_c, zero beyond channel 3.  In f64 that expression as written; in
    f32 the multiply-add v * m_c + a_c it is folded into, with m_c = 1 / (255 std_c) and a_c = -mean_c / std_c rounded to f32."""
    out, terms = torch.zeros(img.shape[0], cpad, dtype=dt), torch.zeros(img.shape[0], cpad, dtype=dt)
    for c in range(3):
        v = img[:, c].to(dt)
        if dt == F64:
            out[:, c] = (v / 255.0 - mean[c]) / std[c]
        else:
            out[:, c] = v * torch.tensor(1.0 / (255.0 * std[c]), dtype=dt) + torch.tensor(-mean[c] / std[c], dtype=dt)
        terms[:, c] = v / (255.0 * std[c]) + abs(mean[c] / std[c])
    return out, terms


def latent_sample_terms(dt, mom: Tensor, eps: Tensor, C: int, scale: float, ld_out: int):
    """(mean + exp(clamp(logvar, -30, 20) / 2) * eps) * scale -> [pixels, ld_out], zero padded; mom [pixels, >= 2C], eps [pixels, >= C]."""
    mean, lv = mom[:, :C].to(dt), mom[:, C:2 * C].to(dt).clamp(-30.0, 20.0)
    s = torch.tensor(scale, dtype=torch.float32).to(dt)
    n = torch.exp(0.5 * lv) * eps[:, :C].to(dt)
    out, terms = torch.zeros(mom.shape[0], ld_out, dtype=dt), torch.zeros(mom.shape[0], ld_out, dtype=dt)
    out[:, :C], terms[:, :C] = (mean + n) * s, (mean.abs() + n.abs()) * s
    return out, terms


def cdiv(a: int, b: int) -> int:
    return -(-a // b)

