"""A/B of the ControlNet train step with and without the sphere-weighted loss (``attach_frozen(sphere_loss_weight=)``, csrc/loss_weight.hip):
SD-Turbo, B = 8, 512^2, on a resident synthetic batch whose targets are the joint spheres of ``render.synthetic_episode`` drawn by
gn_render_spheres over random frames (tiled 2 x 2 views, the trainer's layout) and whose conditioning images are the frames themselves.
Two trainers (weight 0 and weight 4) share the frozen weights and alternate in ONE process, whole rounds of steps each, the order swapped
every round; prints the median (min - max) ms per step of each setting and the marked fraction of the target pixels, writes them as JSON.
Needs an MI355X.  Every step runs under its own time limit: a step that exceeds --step-timeout seconds ends the process with a traceback.

    python tools/bench_sphere_loss.py [--rounds 5] [--steps 5] [--warmup 3] [--weight 4] [--out profiles/sphere_loss_ab.json]
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genima_amd import configs, render, schema, weights  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402
from genima_amd.packing import pack_state_dict  # noqa: E402
from genima_amd.scheduler import DDPMScheduler  # noqa: E402
from genima_amd.training import ControlNetTrainer  # noqa: E402


def sphere_batch(E, B, texture_dir, seed=7):
    """-> the train batch (f16 NHWC-8 on the device): targets in [-1, 1] with the spheres drawn, conditioning images in [0, 1] without."""
    dev, H, W = E.device, 256, 256
    cfg, traj, _ = render.synthetic_episode(B + 21, seed=seed, texture_dir=texture_dir, action_horizon=20)
    views = [v for ts in range(B) for v in render.pack_step(traj, cfg, ts, render.tile_cameras(cfg.cameras))]
    g = torch.Generator(device=dev).manual_seed(seed)
    frames = torch.randint(0, 256, (4 * B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    target = render.render_views(E, render.pack_views(views), render.load_atlas(texture_dir), H, W, 4, bg=frames, want=("full_f16",))["full_f16"]
    tiled = frames.view(B, 2, 2, H, W, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, 3).contiguous()
    cond = E.image_u8_to_f16(tiled, 8, 1.0, 0.0).clone()
    fam = configs.family("sd-turbo")
    V = fam["text"]["vocab_size"]
    ids = torch.zeros(B, 77, dtype=torch.int32)
    ids[:, :14] = torch.tensor([V - 2] + [320 + i for i in range(12)] + [V - 1], dtype=torch.int32)
    return dict(pixel_values=target.clone(), conditioning_pixel_values=cond, input_ids=ids.to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per setting after the warm-up (at least 5 for the table in DESIGN.md)")
    ap.add_argument("--steps", type=int, default=5, help="train steps per round and setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weight", type=float, default=4.0)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one step (the first ones autotune) may take before the process is ended")
    ap.add_argument("--sphere_textures", default=os.path.join(ROOT, "tests", "golden", "sphere_textures"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_loss_ab.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    fam = configs.family("sd-turbo")
    synth = lambda sch, seed: weights.synth_state_dict(sch, seed, device=dev)  # noqa: E731
    unet_W = pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), dev, up_phases=False)
    vae_W = pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), dev)
    text_W = pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), dev)
    trainers = {}
    for lam in (0.0, args.weight):
        tr = ControlNetTrainer(Engine(dev, autotune=True), fam["unet"], fam["controlnet"], unet_W, synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-5)
        tr.attach_frozen(fam["vae"], vae_W, fam["text"], text_W, DDPMScheduler(), seed=1234, sphere_loss_weight=lam)
        trainers[lam] = tr
    batch = sphere_batch(trainers[0.0].E, args.batch, args.sphere_textures)

    def steps(tr, n):
        """n steps, each under its own time limit; -> ms per step"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            faulthandler.dump_traceback_later(args.step_timeout, exit=True)
            loss = tr.train_step(batch)
            if i == n - 1:
                loss = float(loss)  # waits for the round's last step
            faulthandler.cancel_dump_traceback_later()
        return (time.perf_counter() - t0) / n * 1e3, loss

    for lam, tr in trainers.items():
        ms, loss = steps(tr, args.warmup)
        print(f"warm-up weight {lam:g}: {ms:8.2f} ms per step, loss {loss:.5f}", flush=True)
    times = {lam: [] for lam in trainers}
    for r in range(args.rounds):
        for lam in (list(trainers) if r % 2 == 0 else list(trainers)[::-1]):
            ms, _ = steps(trainers[lam], args.steps)
            times[lam].append(ms)
    fraction = float(trainers[args.weight].last["sphere_fraction"])
    res = dict(family="sd-turbo", batch=args.batch, resolution=512, rounds=args.rounds, steps_per_round=args.steps, warmup=args.warmup,
               sphere_fraction=fraction, ms_per_step={})
    for lam, ts in times.items():
        res["ms_per_step"][f"{lam:g}"] = dict(median=statistics.median(ts), min=min(ts), max=max(ts), rounds=ts)
        print(f"sphere_loss_weight {lam:g}: {statistics.median(ts):8.2f} ms per step ({min(ts):.2f} - {max(ts):.2f}) over {len(ts)} rounds of {args.steps} steps", flush=True)
    print(f"marked fraction of the target pixels: {fraction:.4%}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
