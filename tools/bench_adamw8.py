"""The optimizer pass alone on a ControlNet's flat buffers: gn_adamw_flat (fp32 moments) against gn_adamw8_flat (8-bit blockwise moments,
csrc/optim8.hip), alternating, device events, warmed up; GB/s of the bytes each pass actually moves.

    python tools/bench_adamw8.py [--family sd-turbo] [--rounds 5] [--iters 10]
"""
import argparse
import os
import sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import configs, optim8, schema  # noqa: E402
from genima_amd import train_ops as T  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402
from genima_amd.packing import pack_state_dict  # noqa: E402
from genima_amd.training import flat_layout  # noqa: E402

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="sd-turbo")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    cfg = configs.family(args.family)["controlnet"]
    sd = OrderedDict((n, torch.empty(tuple(s), device="meta")) for n, s in schema.controlnet_schema(cfg).items())
    layout, numel = flat_layout(pack_state_dict(sd, "meta", dtype=torch.float32))
    table, small, n8, n_small = optim8.build_block_table(layout)
    E = Engine("cuda:0")
    dev = E.device
    gen = torch.Generator(device=dev).manual_seed(0)
    master = torch.randn(numel, device=dev, generator=gen) * 0.05
    grad = torch.randn(numel, device=dev, generator=gen)
    half = torch.zeros(numel, dtype=torch.float16, device=dev)
    m, v = torch.zeros(numel, device=dev), torch.zeros(numel, device=dev)
    tab = table.to(dev)
    mc, vc = torch.zeros(n8, dtype=torch.uint8, device=dev), torch.zeros(n8, dtype=torch.uint8, device=dev)
    ma, va = torch.zeros(table.shape[0], device=dev), torch.zeros(table.shape[0], device=dev)
    S, U = optim8.dynamic_map(True).to(dev), optim8.dynamic_map(False).to(dev)
    clip = torch.tensor([1.0, 1.0, 0.0], device=dev)
    hp = (1e-5, 0.9, 0.999, 1e-8, 1e-2)
    step = [0]

    def fp32():  # zero_grad off: the same gradient serves every iteration
        T.adamw(E, master, grad, m, v, *hp, step[0], clip, 1.0, half_out=half, zero_grad=False)

    def q8():
        T.adamw8(E, master, grad, mc, vc, ma, va, tab, S, U, *hp, step[0], clip, 1.0, half_out=half, zero_grad=False)

    ms_, vs_ = torch.zeros(n_small, device=dev), torch.zeros(n_small, device=dev)

    def small_ranges():  # what the trainer adds to the 8-bit launch: one gn_adamw_flat launch per fp32 range
        at = 0
        for a, b in small:
            T.adamw(E, master[a:b], grad[a:b], ms_[at:at + b - a], vs_[at:at + b - a], *hp, step[0], clip, 1.0, half_out=half[a:b], zero_grad=False)
            at += b - a

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(E.stream):
            a.record(E.stream)
            for _ in range(args.iters):
                step[0] += 1
                fn()
            b.record(E.stream)
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    for fn in (fp32, q8, small_ranges):  # warm-up
        step[0] = 0
        timed(fn)
    res = {"fp32": [], "8bit": [], "small": []}
    for _ in range(args.rounds):  # alternating
        res["fp32"].append(timed(fp32))
        res["8bit"].append(timed(q8))
        res["small"].append(timed(small_ranges))
    # bytes moved with zero_grad off: the gradient is read only (4 instead of 8 bytes per element)
    bytes32 = numel * (4 + 8 + 8 + 8 + 2)
    bytes8 = n8 * (4 + 8 + 2 + 2 + 2) + table.shape[0] * (16 + 16)
    print(f"{args.family} ControlNet flat buffer: {numel} elements, {n8} quantised in {table.shape[0]} blocks, {n_small} in {len(small)} fp32 ranges")
    for name, nbytes in (("fp32", bytes32), ("8bit", bytes8)):
        ts = sorted(res[name])
        med = ts[len(ts) // 2]
        print(f"{name:5s} ms per pass: " + " ".join(f"{t:.3f}" for t in res[name]) + f" | median {med:.3f} ms, {nbytes / 1e9:.2f} GB moved (gradient read "
              f"only), {nbytes / med / 1e6:.0f} GB/s = {nbytes / med / 1e6 / HBM_PEAK_GBS:.1%} of {HBM_PEAK_GBS:.0f} GB/s")
    print(f"small {len(small)} gn_adamw_flat launches over the fp32 ranges ({n_small} elements), ms per optimizer step (back to back on one stream): "
          + " ".join(f"{t:.3f}" for t in res["small"]))


if __name__ == "__main__":
    main()
