"""-m "not gpu": the host side of the 8-bit blockwise AdamW (genima_amd/optim8.py) -- the two dynamic code maps and the block table over
the tiny and the SD-Turbo ControlNet layouts -- and ``restate_step``: a pure-torch restatement of one 8-bit AdamW step (csrc/optim8.hip's
operation sequence, any float dtype), the yardstick of tests/test_adamw8_gpu.py, checked here against itself in f32 vs f64.

Measured here (CPU, `_ragged_case()` below: 5 parameters of 4096 / 4097 / 5121 / 8200 / 1048576 elements, |g| log-uniform over 6 decades):
after 1 step the f32 restatement's codes equal the f64 one's (0 + 0 of 1 070 090 first- / second-moment codes differ), parameter rel-L2
3.9e-8; after 5 steps 3 + 37 codes differ (share 1.9e-5) -- a code that differs once changes that element's moment by a code gap, so its
later codes drift further: the largest index distance is 2 -- and the parameter rel-L2 is 2.8e-6."""
from collections import OrderedDict

import numpy as np
import torch

from genima_amd import configs, optim8, schema
from genima_amd.packing import pack_state_dict
from genima_amd.training import flat_layout

HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def expand_blocks(table: torch.Tensor):
    """Block table -> (flat element index, code index, block id) of every covered element, int64 each."""
    idx, cidx, bid = [], [], []
    for b, (off, coff, ln) in enumerate(optim8.table_blocks(table)):
        idx.append(torch.arange(off, off + ln))
        cidx.append(torch.arange(coff, coff + ln))
        bid.append(torch.full((ln,), b, dtype=torch.int64))
    return torch.cat(idx), torch.cat(cidx), torch.cat(bid)


def nearest_code(cmap: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Index of the entry of the ascending map nearest to x; halfway -> the lower index (csrc/optim8.hip nearest_code)."""
    lo = (torch.searchsorted(cmap, x.contiguous(), right=True) - 1).clamp_(0, 255)  # the last entry <= x (0 when x is below the map)
    hi = (lo + 1).clamp_(max=255)
    return torch.where((cmap[hi] - x) < (x - cmap[lo]), hi, lo)


def restate_step(state: dict, grad: torch.Tensor, expand, step: int, clip_coef=None, grad_scale: float = 1.0, *, lr, beta1, beta2, eps, wd,
                 dtype=torch.float32):
    """One 8-bit blockwise AdamW step on ``state`` = dict(p [n] dtype, m_codes / v_codes uint8 [n8], m_absmax / v_absmax [n_blocks] dtype), in
    place, in ``dtype`` arithmetic, operation by operation as the kernel: scalars are the f32 values the library receives, derived
    scalars (1 - beta, bias corrections, ...) are formed in ``dtype``.  ``clip_coef``: the f32 device scalar's value or None."""
    idx, cidx, bid = expand
    f = np.float32 if dtype == torch.float32 else np.float64
    lr, b1, b2, eps, wd, gsc = (f(np.float32(v)) for v in (lr, beta1, beta2, eps, wd, grad_scale))
    one = f(1.0)
    gs = gsc * (f(np.float32(clip_coef)) if clip_coef is not None else one)
    bc1, bc2 = f(1.0 - np.power(np.float64(b1), step)), f(1.0 - np.power(np.float64(b2), step))  # an f64 power, rounded once (the host code)
    decay, omb1, omb2, rbc2, slr = one - lr * wd, one - b1, one - b2, np.sqrt(bc2), lr / bc1
    S, U = optim8.dynamic_map(True).to(dtype), optim8.dynamic_map(False).to(dtype)
    nb = state["m_absmax"].numel()
    g = grad[idx].to(dtype) * float(gs)
    m0 = S[state["m_codes"][cidx].long()] * state["m_absmax"][bid]
    v0 = U[state["v_codes"][cidx].long()] * state["v_absmax"][bid]
    mi = m0 * float(b1) + g * float(omb1)
    vi = v0 * float(b2) + (g * float(omb2)) * g
    denom = vi.sqrt() / float(rbc2) + float(eps)
    state["p"][idx] = state["p"][idx] * float(decay) - (mi / denom) * float(slr)
    am = torch.zeros(nb, dtype=dtype).scatter_reduce_(0, bid, mi.abs(), "amax")
    av = torch.zeros(nb, dtype=dtype).scatter_reduce_(0, bid, vi, "amax")
    rm = torch.where(am > 0, 1.0 / am, torch.zeros_like(am))
    rv = torch.where(av > 0, 1.0 / av, torch.zeros_like(av))
    state["m_codes"][cidx] = nearest_code(S, mi * rm[bid]).to(torch.uint8)
    state["v_codes"][cidx] = nearest_code(U, vi * rv[bid]).to(torch.uint8)
    state["m_absmax"], state["v_absmax"] = am, av
    return mi, vi  # the unquantised new moments (for the quantisation-bound test)


def fresh_state(p: torch.Tensor, table: torch.Tensor, n8: int, dtype=torch.float32) -> dict:
    nb = table.shape[0]
    return dict(p=p.to(dtype).clone(), m_codes=torch.zeros(n8, dtype=torch.uint8), v_codes=torch.zeros(n8, dtype=torch.uint8),
                m_absmax=torch.zeros(nb, dtype=dtype), v_absmax=torch.zeros(nb, dtype=dtype))


def _ragged_case(seed: int = 0, sizes=(4096, 4097, 256 * 20 + 1, 8200, 1 << 20)):
    """A flat buffer of ragged parameters at multiples of 8 (TrainParams' packing): -> (layout, numel, master, [5 gradients])."""
    layout, off = OrderedDict(), 0
    for i, n in enumerate(sizes):
        layout[f"w{i}"] = (off, (n,))
        off += (n + 7) // 8 * 8
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(off, generator=gen) * 0.05
    grads = []
    for _ in range(5):  # |g| log-uniform over [1e-5, 10], random sign: six decades
        mag = 10.0 ** (torch.rand(off, generator=gen) * 6.0 - 5.0)
        grads.append(mag * torch.where(torch.rand(off, generator=gen) < 0.5, -1.0, 1.0))
    return layout, off, p, grads


def _meta_layout(cfg):
    sd = OrderedDict((n, torch.empty(tuple(shape), device="meta")) for n, shape in schema.controlnet_schema(cfg).items())
    return flat_layout(pack_state_dict(sd, "meta", dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------------- tests
def test_code_maps():
    S, U = optim8.dynamic_map(True), optim8.dynamic_map(False)
    for m in (S, U):
        assert m.shape == (256,) and m.dtype == torch.float32
        assert bool((m[1:] > m[:-1]).all()), "strictly increasing"
        assert int((m == 0).sum()) == 1 and float(m[-1]) == 1.0
    assert float(S[0]) < 0 and abs(float(S[0]) + 0.99296875) < 1e-6
    assert float(U[0]) == 0.0
    assert int((S > 0).sum()) == 128 and int((S < 0).sum()) == 127  # 127 of either sign + {0, 1}


def _check_table(layout, numel):
    table, small, n8, n_small = optim8.build_block_table(layout)
    cover = torch.zeros(numel, dtype=torch.int32)
    bounds = {}
    for name, (off, shape) in layout.items():
        n = 1
        for s in shape:
            n *= s
        bounds[name] = (off, off + n, n)
    big = [(a, b) for a, b, n in bounds.values() if n >= optim8.MIN_8BIT_SIZE]
    starts = torch.tensor([a for a, _ in big])
    ends = torch.tensor([b for _, b in big])
    o = table[:, 0]
    ln = table[:, 1] & 511
    co = table[:, 1] >> 9
    assert int(ln.min()) >= 1 and int(ln.max()) <= optim8.BLOCK
    assert bool((o % 8 == 0).all())  # 16-byte aligned float4 rows for the kernel
    owner = torch.searchsorted(starts, o.contiguous(), right=True) - 1  # the quantised parameter each block starts in ...
    assert bool((owner >= 0).all()) and bool((o + ln <= ends[owner]).all()), "a block crosses a layout boundary"
    assert torch.equal(co, torch.cumsum(ln, 0) - ln) and int(ln.sum()) == n8  # codes are compact, in table order
    cover.index_add_(0, torch.repeat_interleave(o, ln) + (torch.arange(n8) - torch.repeat_interleave(co, ln)), torch.ones(n8, dtype=torch.int32))
    for a, b in big:
        assert bool((cover[a:b] == 1).all())
    assert int(cover.sum()) == sum(b - a for a, b in big) == n8  # ... and nothing else is covered
    # small parameters: all in the fp32 ranges, nothing else there
    scover = torch.zeros(numel, dtype=torch.int32)
    for a, b in small:
        scover[a:b] += 1
    for a, b, n in bounds.values():
        assert bool((scover[a:b] == (1 if n < optim8.MIN_8BIT_SIZE else 0)).all())
    assert int(scover.sum()) == n_small == sum(n for _, _, n in bounds.values() if n < optim8.MIN_8BIT_SIZE)
    assert all(small[i][1] < small[i + 1][0] for i in range(len(small) - 1)), "adjacent ranges are merged, in order"
    return table.shape[0], len(small), n8, n_small


def test_block_table_tiny_and_sd_turbo():
    for cfg, name in ((configs.TINY_CONTROLNET, "tiny"), (configs.SD_TURBO_CONTROLNET, "sd-turbo")):
        layout, numel = _meta_layout(cfg)
        nb, ns, n8, n_small = _check_table(layout, numel)
        state = 2 * n8 + 8 * nb + 8 * n_small
        print(f"{name}: {numel} elements, {nb} blocks, {ns} fp32 ranges, n8 {n8}, n_small {n_small}: state {state} bytes = "
              f"{state / (8 * numel):.4f} of fp32's {8 * numel}")
        assert state < 0.26 * 8 * numel
        assert bool(((optim8.build_block_table(layout)[0][:, 1] >> 9) % 4 == 0).all())  # every block's four-code groups are aligned dwords


def test_block_table_ragged():
    layout, numel, _, _ = _ragged_case()
    layout["bias"] = (numel, (320,))
    layout["gamma"] = (numel + 320, (320,))
    nb, ns, n8, n_small = _check_table(layout, numel + 640)
    assert ns == 1 and n_small == 640 and n8 == 4096 + 4097 + 5121 + 8200 + (1 << 20)


def run_restatement(dtype, steps, clip_coef=None, grad_scale=1.0):
    layout, numel, p, grads = _ragged_case()
    table, _, n8, _ = optim8.build_block_table(layout)
    ex = expand_blocks(table)
    st = fresh_state(p, table, n8, dtype)
    for k in range(steps):
        restate_step(st, grads[k], ex, k + 1, clip_coef, grad_scale, dtype=dtype, **HYPER)
    return st


def code_diff(a: torch.Tensor, b: torch.Tensor):
    """-> (number of differing codes, the largest index distance)."""
    d = (a.int() - b.int()).abs()
    return int((d != 0).sum()), int(d.max())


def test_restatement_f32_against_f64():
    for steps in (1, 5):
        a, b = run_restatement(torch.float32, steps), run_restatement(torch.float64, steps)
        n = a["m_codes"].numel()
        dm, wm = code_diff(a["m_codes"], b["m_codes"])
        dv, wv = code_diff(a["v_codes"], b["v_codes"])
        e = float((a["p"].double() - b["p"]).norm() / b["p"].norm())
        print(f"{steps} step(s): f32 vs f64 restatement: {dm} + {dv} of {n} codes differ (max distance {max(wm, wv)}), parameter rel-L2 {e:.2e}")
        assert (dm + dv) < 0.01 * 2 * n, "inputs must keep the f32 restatement within 1 % of the f64 codes"
        # (no bar on the index distance here: one differing code feeds the next step's moment, so f32 and f64 drift apart step by step --
        #  2 after 5 steps; the GPU test holds the kernel to a distance of 1 from the f32 restatement, the same arithmetic)
        assert e < 1e-5
        assert float((a["m_absmax"].double() - b["m_absmax"]).abs().max()) <= 1e-6 * float(b["m_absmax"].max())
    # the update moves the parameters at all, and every block got an absmax
    assert float((a["p"] - _ragged_case()[2]).abs().max()) > 1e-4 and bool((a["m_absmax"] > 0).all()) and bool((a["v_absmax"] > 0).all())
