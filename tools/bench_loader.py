"""Benchmark of the training DataLoader (genima_amd/data.py) on a synthetic PNG tree in the on-disk layout ``RLBenchDataset`` reads:

  * batches/s of the loader alone for ``cache=None`` (one decode thread: the loader before the frame cache), ``decode_workers=8``,
    ``cache="host"`` and ``cache="device"`` from epoch 2 on (epoch 1 fills the cache and is reported apart);
  * ms per batch of ``to_device`` (upload / gather + conversion, synchronised) for the uncached and the device-cached batch;
  * us of ``gn_gather_u8_to_f16`` and ``gn_image_u8_to_f16`` at B x resolution^2 (device events);
  * ms per loader-fed ``train_step`` of the SD-Turbo family for ``cache=None`` against ``cache="device"`` from epoch 2 on, and per step on one
    resident synthetic batch (what bench_train.py times), all three alternating in one process; with ``--render-textures DIR`` also, in the
    same alternation, ``cache="device"`` on a tree that ``render_episode`` wrote against the same loader with ``render_targets`` (targets
    drawn on the device instead of read); with ``--view-augment SPEC`` on top of that, in the same alternation, that ``render_targets``
    loader with ``view_augment=SPEC`` (the camera-pose and light augmentation with re-drawn targets), its difference to the loader without it
    beside that loader's own spread, us of ``gn_view_augment_tiled`` alone on one of its batches beside the bytes it moves, and the share of
    pixels the turned cameras reveal.

The frames are generated (smooth structure + sensor noise, ~400 KB per 512^2 PNG); real renders compress better and decode faster.  Every
setting is timed ``--rounds`` times, alternating, after a warm-up epoch; the spread over the rounds is printed beside the median.  Needs an
MI355X.

    python tools/bench_loader.py [--batch 8] [--resolution 512] [--examples 64] [--rounds 3] [--no-train] [--render-textures DIR] [--view-augment SPEC] [--out bench_loader.json]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import data as D  # noqa: E402
from genima_amd import render as Rn  # noqa: E402


def write_tree(root, n_examples, R):
    """One task, two episodes, ``n_examples`` tiled examples (the reader drops each episode's last frame): 2 * (n_examples + 2) files."""
    from PIL import Image

    rng = np.random.RandomState(0)
    base = os.path.join(root, "bench_task", "variation0")
    os.makedirs(os.path.join(base, "episodes"))
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["bench"], f)
    yy, xx = np.mgrid[0:R, 0:R].astype(np.float32) / R
    per_ep = n_examples // 2 + 1
    for e in range(2):
        for kind in ("rgb", "rgb_rendered"):
            d = os.path.join(base, "episodes", f"episode{e}", kind)
            os.makedirs(d)
            for i in range(per_ep):
                ph = rng.uniform(0, 6.28, 3)
                img = np.stack([127 + 100 * np.sin(6.28 * (xx * (c + 1) + yy * (3 - c)) + ph[c]) for c in range(3)], -1)
                img[R // 4: R // 2, R // 3: 2 * R // 3] = rng.randint(0, 256, 3)  # a flat "object"
                img = np.clip(img + rng.normal(0, 2.0, img.shape), 0, 255).astype(np.uint8)  # sensor noise
                Image.fromarray(img).save(os.path.join(d, f"{i}.png"))
    return D.RLBenchDataset(root, tasks="bench_task", num_demos=2)


def write_rendered_tree(root, n_examples, R, texture_dir, E):
    """Two generated episodes (``render.synthetic_episode``) rendered by ``render_episode``: ``n_examples`` tiled examples whose targets
    are the spheres drawn over their conditioning frames, with the ``traj.npz`` a ``render_targets`` loader draws them from."""
    assert R == 512, "the rendered tree is the 2x2 tiling of 256^2 views"
    base = os.path.join(root, "bench_task", "variation0")
    per_ep = n_examples // 2 + 2  # L steps -> L - 1 tiled frames, of which the reader drops the last
    for e in range(2):
        cfg, traj, frames = Rn.synthetic_episode(per_ep, seed=e, texture_dir=texture_dir, action_horizon=20)
        Rn.render_episode(traj, frames, os.path.join(base, "episodes", f"episode{e}"), cfg, engine=E)
    with open(os.path.join(base, "variation_descriptions.pkl"), "wb") as f:
        pickle.dump(["bench"], f)
    return D.RLBenchDataset(root, tasks="bench_task", num_demos=2, image_type="tiled_rgb_rendered", conditioning_image_type="tiled_rgb"), cfg


def epoch_seconds(loader, consume=None):
    t0 = time.perf_counter()
    n = 0
    for b in loader:
        if consume is not None:
            consume(b)
        n += 1
    if consume is not None:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def summary(xs, scale=1.0):
    return dict(median=statistics.median(xs) * scale, min=min(xs) * scale, max=max(xs) * scale, n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--examples", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--family", default="sd-turbo")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--render-textures", default=None, help="directory of the five sphere textures: also time a loader whose targets are drawn "
                    "on the device (DataLoader(render_targets=...)) against cache=\"device\" on a tree that render_episode wrote (resolution 512)")
    ap.add_argument("--view-augment", default=None, help="a perturb.parse spec or preset (camera_pose+light_color): also time the render_targets "
                    "loader with view_augment=SPEC, and gn_view_augment_tiled alone (needs --render-textures)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.view_augment and not args.render_textures:
        ap.error("--view-augment needs --render-textures: the augmentation re-draws the targets a render_targets loader draws")
    from genima_amd import configs
    from genima_amd.engine import Engine
    from genima_amd.pipeline import HashTokenizer

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, R = args.batch, args.resolution
    fam = configs.family(args.family)
    tok = HashTokenizer(fam["text"]["vocab_size"])
    E = Engine(dev, autotune=True)
    res = dict(batch=B, resolution=R, examples=args.examples, rounds=args.rounds)
    with tempfile.TemporaryDirectory() as root:
        ds = write_tree(root, args.examples, R)
        files = sorted({p for e in ds.examples for p in (e["image"], e["conditioning_image"])})
        res["files"], res["png_kb_mean"] = len(files), sum(os.path.getsize(p) for p in files) / len(files) / 1e3
        t0 = time.perf_counter()
        for p in files[:20]:
            with open(p, "rb") as f:
                D.resize_center_crop_u8(f.read(), R)
        res["decode_ms_per_png"] = (time.perf_counter() - t0) / 20 * 1e3

        def loader(**kw):
            return D.DataLoader(ds, B, tok, R, shuffle=True, seed=0, **kw)

        # ---- the loader alone
        settings = {"cache_none": loader(), "decode_workers_8": loader(decode_workers=8), "cache_host": loader(cache="host"),
                    "cache_device": loader(cache="device"), "cache_host_workers_8": loader(cache="host", decode_workers=8)}
        first = {k: epoch_seconds(ld) for k, ld in settings.items()}  # warm-up; the caches fill here
        res["loader_epoch1_batches_per_s"] = {k: 1.0 / v for k, v in first.items()}
        times = {k: [] for k in settings}
        for _ in range(args.rounds):
            for k, ld in settings.items():
                times[k].append(1.0 / epoch_seconds(ld))
        res["loader_batches_per_s"] = {k: summary(v) for k, v in times.items()}

        # ---- to_device, synchronised (fresh loaders: the device cache above was never uploaded)
        plain, cached = loader(), loader(cache="device")
        todev = lambda b: D.to_device(E, b)  # noqa: E731
        epoch_seconds(plain, todev), epoch_seconds(cached, todev)
        times = {"cache_none": [], "cache_device": []}
        for _ in range(args.rounds):
            times["cache_none"].append(epoch_seconds(plain, todev))
            times["cache_device"].append(epoch_seconds(cached, todev))
        res["loader_plus_to_device_ms_per_batch"] = {k: summary(v, 1e3) for k, v in times.items()}
        res["device_cache_mb"] = cached.cache.nbytes / 1e6

        # ---- the kernels (device events)
        frames = torch.randint(0, 256, (B, R, R, 3), dtype=torch.uint8, device=dev)
        ptrs = torch.tensor([frames[(i * 3) % B].data_ptr() for i in range(B)], dtype=torch.int64, device=dev)

        def kernel_us(fn, iters=100):
            for _ in range(10):
                fn()
            a, e = E.event(), E.event()
            E.event_record(a)
            for _ in range(iters):
                fn()
            E.event_record(e)
            E.synchronize()
            return E.event_elapsed_ms(a, e) / iters * 1e3
        ks = {"gather_u8_to_f16_us": [], "image_u8_to_f16_us": []}
        for _ in range(args.rounds):
            ks["gather_u8_to_f16_us"].append(kernel_us(lambda: E.gather_u8_to_f16(ptrs, (R, R), 8, 2.0, -1.0)))
            ks["image_u8_to_f16_us"].append(kernel_us(lambda: E.image_u8_to_f16(frames, 8, 2.0, -1.0)))
        res.update({k: summary(v) for k, v in ks.items()})
        res["kernel_bytes_mb"] = B * R * R * (3 + 16) / 1e6

        # ---- loader-fed train_step
        if not args.no_train:
            from genima_amd import schema, weights
            from genima_amd.packing import pack_state_dict
            from genima_amd.scheduler import DDPMScheduler
            from genima_amd.training import ControlNetTrainer

            synth = lambda sch, seed: weights.synth_state_dict(sch, seed, device=dev)  # noqa: E731
            tr = ControlNetTrainer(E, fam["unet"], fam["controlnet"], pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), dev, up_phases=False),
                                   synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-5)
            tr.attach_frozen(fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), dev), fam["text"],
                             pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), dev), DDPMScheduler(), seed=1234,
                             augmentations="crop,colorjitter")
            plain, cached = loader(), loader(cache="device")
            resident = D.to_device(E, next(iter(loader(prefetch=0))))
            n_batches = len(plain)
            step = lambda b: tr.train_step(b)  # noqa: E731
            epoch_seconds(cached, step)  # warm-up: kernels, tune table, and the cache fills

            def resident_seconds():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n_batches):
                    tr.train_step(resident)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n_batches
            drawn = {}
            if args.render_textures:  # the same number of examples, their targets rendered: read back as PNGs, or drawn in to_device
                ds2, cfg2 = write_rendered_tree(os.path.join(root, "rendered_tree"), args.examples, R, args.render_textures, E)
                drawn = {"rendered_tree_cache_device": D.DataLoader(ds2, B, tok, R, shuffle=True, seed=0, cache="device"),
                         "rendered_tree_cache_device_render_targets": D.DataLoader(ds2, B, tok, R, shuffle=True, seed=0, cache="device",
                                                                                   render_targets=Rn.TrajectorySource(cfg2))}
                base_key, aug_key = "rendered_tree_cache_device_render_targets", "rendered_tree_cache_device_render_targets_view_augment"
                if args.view_augment:
                    drawn[aug_key] = D.DataLoader(ds2, B, tok, R, shuffle=True, seed=0, cache="device", render_targets=Rn.TrajectorySource(cfg2),
                                                  view_augment=args.view_augment)
                for ld in drawn.values():
                    epoch_seconds(ld, step)  # the caches fill
            times = {"cache_none": [], "cache_device": [], "resident_synthetic_batch": [], **{k: [] for k in drawn}}
            for _ in range(args.rounds):
                times["cache_none"].append(epoch_seconds(plain, step))
                times["cache_device"].append(epoch_seconds(cached, step))
                for k, ld in drawn.items():
                    times[k].append(epoch_seconds(ld, step))
                times["resident_synthetic_batch"].append(resident_seconds())
            res["train_step_ms"] = {k: summary(v, 1e3) for k, v in times.items()}
            if args.view_augment and drawn:
                from genima_amd import perturb

                base, aug = res["train_step_ms"][base_key], res["train_step_ms"][aug_key]
                va = dict(spec=args.view_augment, setting=perturb.parse(args.view_augment).describe(), baseline=base_key,
                          train_step_delta_ms=aug["median"] - base["median"], baseline_spread_ms=base["max"] - base["min"])
                va["delta_exceeds_baseline_spread"] = abs(va["train_step_delta_ms"]) > va["baseline_spread_ms"]
                # the kernel alone, on the tables of one of the loader's own batches and frames that lie apart on the device
                host = next(iter(D.DataLoader(ds2, B, tok, R, shuffle=True, seed=0, prefetch=0, render_targets=Rn.TrajectorySource(cfg2),
                                              view_augment=args.view_augment)))
                M, colour = (host["render_views"][k].to(dev) for k in ("M", "colour"))
                n = int(M.shape[0])
                out_u8 = torch.empty((n, R, R, 3), dtype=torch.uint8, device=dev)
                out_f16 = torch.empty((n, R, R, 8), dtype=torch.float16, device=dev)
                rev = torch.empty((n, 4), dtype=torch.int32, device=dev)
                fn = lambda: E.view_augment_tiled(M, colour, R // 2, R // 2, frames=ptrs[:n], out_u8=out_u8, out_f16=out_f16, n_revealed=rev)  # noqa: E731
                va["kernel_us"] = summary([kernel_us(fn) for _ in range(args.rounds)])
                va["kernel_mb"] = dict(read_u8=n * R * R * 3 / 1e6, write_u8=n * R * R * 3 / 1e6, write_f16=n * R * R * 16 / 1e6)
                # the revealed share over one epoch of the loader's batches: per tile camera, and over the cameras the setting turns
                counts = torch.zeros(4, dtype=torch.int64, device=dev)
                seen = 0
                for b in drawn[aug_key]:
                    r = D.to_device(E, b)["view_revealed"]
                    counts += r.sum(dim=0)
                    seen += int(r.shape[0])
                share = (counts.double() / (seen * (R // 2) ** 2)).tolist()
                va["revealed_share_per_tile_camera"] = dict(zip(Rn.tile_cameras(cfg2.cameras), share))
                turned = [s for s in share if s > 0]
                va["revealed_share_of_turned_cameras"] = sum(turned) / len(turned) if turned else 0.0
                res["view_augment"] = va
            res["train_family"], res["train_steps_per_epoch"] = args.family, n_batches
    print(json.dumps(res, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
