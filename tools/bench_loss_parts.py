"""A/B of the ControlNet train step with and without the loss read-out (``attach_frozen(loss_parts=)``, gn_mse_loss_parts in
csrc/loss_weight.hip), and the time of one held-out ``eval_loss`` batch: SD-Turbo, B = 8, 512^2, on the resident synthetic sphere batch of
``tools/bench_sphere_loss.py``.  Two trainers (loss_parts 0 and 10) share the frozen weights and alternate in ONE process, whole rounds of
steps each, the order swapped every round; prints the median (min - max) ms per step of each setting, the summary the table gives, and the
median (min - max) ms of ``eval_loss`` over the five default timesteps; writes them as JSON.  Needs an MI355X.  Every step and every
``eval_loss`` call runs under its own time limit: one that exceeds --step-timeout seconds ends the process with a traceback.

    python tools/bench_loss_parts.py [--rounds 5] [--steps 5] [--warmup 3] [--parts 10] [--out profiles/loss_parts_ab.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_sphere_loss import sphere_batch  # noqa: E402
from genima_amd import configs, schema, train_loop, weights  # noqa: E402
from genima_amd import train_ops as T  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402
from genima_amd.packing import pack_state_dict  # noqa: E402
from genima_amd.scheduler import DDPMScheduler  # noqa: E402
from genima_amd.training import ControlNetTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per setting after the warm-up (at least 5 for the table in DESIGN.md)")
    ap.add_argument("--steps", type=int, default=5, help="train steps per round and setting")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", type=int, default=10, help="timestep buckets of the second trainer")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one step (the first ones autotune) or one eval_loss call may take before the process is ended")
    ap.add_argument("--sphere_textures", default=os.path.join(ROOT, "tests", "golden", "sphere_textures"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_parts_ab.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    fam = configs.family("sd-turbo")
    synth = lambda sch, seed: weights.synth_state_dict(sch, seed, device=dev)  # noqa: E731
    unet_W = pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), dev, up_phases=False)
    vae_W = pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), dev)
    text_W = pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), dev)
    trainers = {}
    for n in (0, args.parts):
        tr = ControlNetTrainer(Engine(dev, autotune=True), fam["unet"], fam["controlnet"], unet_W, synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-5)
        tr.attach_frozen(fam["vae"], vae_W, fam["text"], text_W, DDPMScheduler(), seed=1234, loss_parts=n)
        trainers[n] = tr
    batch = sphere_batch(trainers[0].E, args.batch, args.sphere_textures)

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

    for n, tr in trainers.items():
        ms, loss = steps(tr, args.warmup)
        print(f"warm-up loss_parts {n}: {ms:8.2f} ms per step, loss {loss:.5f}", flush=True)
    trainers[args.parts].loss_parts_summary(reset=True)  # the timed rounds alone
    times = {n: [] for n in trainers}
    for r in range(args.rounds):
        for n in (list(trainers) if r % 2 == 0 else list(trainers)[::-1]):
            ms, _ = steps(trainers[n], args.steps)
            times[n].append(ms)
    summary = trainers[args.parts].loss_parts_summary(reset=True)

    # one held-out batch over the default grid: forward only, five timesteps; the first call is the warm-up
    ev, ts = trainers[0], train_loop.LOSS_VALIDATOR_TIMESTEPS
    eval_ms = []
    for i in range(1 + args.rounds):
        torch.cuda.synchronize()
        faulthandler.dump_traceback_later(args.step_timeout, exit=True)
        t0 = time.perf_counter()
        table = ev.eval_loss(batch, ts, seed=0)
        host = table.cpu()
        dt = (time.perf_counter() - t0) * 1e3
        faulthandler.cancel_dump_traceback_later()
        if i:
            eval_ms.append(dt)
    held_out = T.summarize_parts(host.numpy(), fam["vae"]["latent_channels"], ts)

    res = dict(family="sd-turbo", batch=args.batch, resolution=512, rounds=args.rounds, steps_per_round=args.steps, warmup=args.warmup, ms_per_step={},
               eval_loss_ms=dict(timesteps=list(ts), median=statistics.median(eval_ms), min=min(eval_ms), max=max(eval_ms), calls=eval_ms),
               train_summary=summary, held_out_summary=held_out)
    for n, tt in times.items():
        res["ms_per_step"][f"{n}"] = dict(median=statistics.median(tt), min=min(tt), max=max(tt), rounds=tt)
        print(f"loss_parts {n}: {statistics.median(tt):8.2f} ms per step ({min(tt):.2f} - {max(tt):.2f}) over {len(tt)} rounds of {args.steps} steps", flush=True)
    print(f"eval_loss, one batch x {len(ts)} timesteps: {statistics.median(eval_ms):8.2f} ms ({min(eval_ms):.2f} - {max(eval_ms):.2f}) over {len(eval_ms)} calls", flush=True)
    print(f"training table over the timed rounds: n {summary['n']}, loss {summary['loss']:.5f}, sphere {summary['loss_sphere']:.5f}, "
          f"background {summary['loss_background']:.5f}, sphere area {summary['sphere_area']:.4%}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
