"""Micro-benchmark of the train-time augmentation kernels (csrc/augment.hip) at B = 8, 512^2, 8 channels: us per launch of the colour
jitter (three launches: mean, final, apply), the 3x3 Gaussian blur, the nearest affine warp and the reflect-pad crop, and the whole
``augment_data`` chain ``colorjitter,blur,affine,crop`` on a ControlNet batch.  Each pass of blur / affine / crop reads and writes
B * H * W * 16 bytes (33.5 MB each way).  Needs an MI355X; device-event timing after warm-up.

    python tools/bench_augment.py [--batch 8] [--resolution 512] [--iters 50] [--out bench_augment.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import augment  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402


def timeit(E, fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    a, e = E.event(), E.event()
    E.event_record(a)
    for _ in range(iters):
        fn()
    E.event_record(e)
    return E.event_elapsed_ms(a, e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, R = args.batch, args.resolution
    E = Engine(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.zeros(B, R, R, 8, dtype=torch.float16, device=dev)
    x[..., :3] = torch.rand(B, R, R, 3, device=dev, generator=g).half()
    px = torch.zeros_like(x)
    px[..., :3] = (torch.rand(B, R, R, 3, device=dev, generator=g) * 2 - 1).half()
    out = torch.empty_like(x)
    m = augment.affine_inverse_matrix(7.3, (12, -9), 1.04, (1.0, 0.0))
    order, factors = (3, 1, 0, 2), (1.1, 0.9, 1.05, 0.03)
    mbytes = B * R * R * 8 * 2 / 1e6
    res = dict(batch=B, resolution=R, channels=8, mb_each_way=mbytes)
    res["color_jitter_us"] = timeit(E, lambda: augment.color_jitter(E, x, order, factors, out=out), args.iters)
    res["gaussian_blur_us"] = timeit(E, lambda: augment.gaussian_blur(E, x, 1.3, out=out), args.iters)
    res["affine_nearest_us"] = timeit(E, lambda: augment.affine(E, x, m, out=out), args.iters)
    res["reflect_pad_crop_us"] = timeit(E, lambda: augment.reflect_pad_crop(E, x, 1, 3), args.iters)
    batch = dict(pixel_values=px, conditioning_pixel_values=x)
    gen = torch.Generator().manual_seed(0)
    res["chain_us"] = timeit(E, lambda: augment.augment_data(E, "colorjitter,blur,affine,crop", batch, gen), args.iters)
    for k in ("gaussian_blur_us", "affine_nearest_us", "reflect_pad_crop_us"):
        res[k.replace("_us", "_gbps")] = 2 * mbytes / res[k] * 1e3  # MB / us is TB/s, so x 1e3
    for k, v in res.items():
        print(f"{k:>24}: {v:10.2f}" if isinstance(v, float) else f"{k:>24}: {v}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
