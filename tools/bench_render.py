"""Timing of the sphere renderer on a real MI355X (medians over rounds, alternating settings):

  * us of one ``gn_render_spheres`` launch at B views x 256^2, ``samples`` samples, both composites and both f16 tiled outputs, and the
    bytes that launch moves.  Device events round ``--iters`` back-to-back launches (a window of about half a second): that is the
    LAUNCH RATE from Python on WARM caches (the 11.8 MB stay in L2 / MALL), an upper bound of the kernel's own time; the kernel's time is
    the ``rocprofv3 --kernel-trace --stats`` figure of
    ``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_render.py --texture_dir DIR --kernel-only``;
  * ms per batch of ``to_device`` on a ``DataLoader(cache="device")`` batch whose targets are read from the cache against one whose
    targets are drawn (``render_targets``), on a tree that ``render_episode`` wrote.  (The loader-fed train step: tools/bench_loader.py
    ``--render-textures``.)

    python tools/bench_render.py --texture_dir DIR [--views 4] [--samples 4] [--rounds 5] [--iters 40000] [--out render_microbench.json]
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genima_amd import data as D  # noqa: E402
from genima_amd import render as R  # noqa: E402


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40000)
    ap.add_argument("--kernel-only", action="store_true", help="launch the kernel --rounds x 200 times and exit (for a kernel-trace run)")
    ap.add_argument("--texture_dir", required=True, help="directory of the five sphere_<colour>_stripe_texture.png files")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genima_amd.engine import Engine
    from genima_amd.pipeline import HashTokenizer

    dev = torch.device("cuda", 0)
    E = Engine(dev)
    B, H, W = args.views, 256, 256
    cfg, traj, frames = R.synthetic_episode(66, seed=7, texture_dir=args.texture_dir, action_horizon=20)
    views = [v for ts in range((B + 3) // 4) for v in R.pack_step(traj, cfg, ts, R.tile_cameras(cfg.cameras))][:B]
    sc = {k: torch.from_numpy(v).to(dev) for k, v in R.pack_views(views).items()}
    atlas = torch.from_numpy(R.load_atlas(args.texture_dir)).to(dev)
    bg, bg2 = (torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    blend = torch.full((B,), 0.8, dtype=torch.float64, device=dev)
    n_tiled = (B + 3) // 4
    outs = dict(full=torch.empty_like(bg), rnd=torch.empty_like(bg), occupied=torch.empty((B, H, W), dtype=torch.uint8, device=dev),
                full_f16=torch.zeros((n_tiled, 2 * H, 2 * W, 8), dtype=torch.float16, device=dev),
                rnd_f16=torch.zeros((n_tiled, 2 * H, 2 * W, 8), dtype=torch.float16, device=dev))

    def launch():
        E.render_spheres(sc["cams"], sc["spheres"], sc["tex_index"], sc["count"], atlas, H, W, args.samples, bg=bg, bg2=bg2, blend=blend,
                         n_tiled=n_tiled, **outs)

    if args.kernel_only:
        for _ in range(args.rounds * 200):
            launch()
        E.synchronize()
        return

    def kernel_us(fn, iters=args.iters):
        for _ in range(200):
            fn()
        a, e = E.event(), E.event()
        E.event_record(a)
        for _ in range(iters):
            fn()
        E.event_record(e)
        E.synchronize()
        return E.event_elapsed_ms(a, e) / iters * 1e3

    res = dict(views=B, samples=args.samples, H=H, W=W, spheres_per_view=sc["count"].tolist())
    res["iters_per_round"] = args.iters
    res["render_spheres_us"] = summary([kernel_us(launch) for _ in range(args.rounds)])
    # read: two backgrounds; written: two uint8 composites, the mask, two f16 NHWC-8 images (the atlas and the view data stay in cache)
    res["bytes_moved"] = B * H * W * (3 + 3 + 3 + 3 + 1 + 16 + 16)
    res["warm_cache_gb_per_s_at_median"] = res["bytes_moved"] / res["render_spheres_us"]["median"] / 1e3

    # ---- to_device: targets read from the device cache against targets drawn
    tok = HashTokenizer(1024)
    with tempfile.TemporaryDirectory() as root:
        base = os.path.join(root, "bench_task", "variation0")
        ep = os.path.join(base, "episodes", "episode0")
        os.makedirs(ep)
        with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
            pickle.dump(["bench"], f)
        R.render_episode(traj, frames, ep, cfg, engine=E)
        ds = D.RLBenchDataset(root, tasks="bench_task", num_demos=1, image_type="tiled_rgb_rendered", conditioning_image_type="tiled_rgb")
        loaders = {"cache_device_png_targets": D.DataLoader(ds, 8, tok, 512, seed=0, cache="device"),
                   "cache_device_render_targets": D.DataLoader(ds, 8, tok, 512, seed=0, cache="device", render_targets=R.TrajectorySource(cfg))}

        def epoch_ms(ld):
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            for b in ld:
                D.to_device(E, b)
                n += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        for ld in loaders.values():
            epoch_ms(ld)  # the caches fill
        times = {k: [] for k in loaders}
        for _ in range(args.rounds):
            for k, ld in loaders.items():
                times[k].append(epoch_ms(ld))
        res["loader_plus_to_device_ms_per_batch"] = {k: summary(v) for k, v in times.items()}
        res["loader_batch"], res["loader_examples"] = 8, len(ds)
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
