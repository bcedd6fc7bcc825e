"""Micro-benchmark of the TAESD encoder (graphs.emit_taesd_encode) with its AutoencoderTinyBlocks fused into one launch each
(csrc/taesd.hip) against the same encoder with GN_TINY_BLOCK=0 (three conv launches per block) and against the AutoencoderKL encoder
(emit_vae_encode_moments) at 512^2; single-block times at 512^2 and 256^2; with --train, one ControlNet train step with and without
--tiny_vae.  Needs an MI355X; device-event timing, every shape warmed up first.

    python tools/bench_taesd.py [--batches 1,8] [--block-batch 8] [--train] [--out bench_taesd.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import configs, graphs, packing, schema, weights  # noqa: E402
from genima_amd.engine import Engine  # noqa: E402


def timeit(E, fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    a, e = E.event(), E.event()
    E.event_record(a)
    for _ in range(iters):
        fn()
    E.event_record(e)
    return E.event_elapsed_ms(a, e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--block-batch", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--train", action="store_true", help="also time one SD-Turbo ControlNet train step, default VAE vs --tiny_vae")
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--use_8bit_adam", action="store_true", help="the train step with 8-bit blockwise AdamW moments")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    R = args.resolution
    E = Engine(dev, autotune=True)
    res = {}

    tW = packing.pack_state_dict(weights.synth_state_dict(schema.taesd_schema(configs.TAESD, decoder=False), 3), dev)
    kW = packing.pack_state_dict(weights.synth_state_dict(schema.vae_schema(configs.SD_TURBO_VAE), 3), dev)
    for B in [int(b) for b in args.batches.split(",")]:
        x8 = torch.zeros(B, R, R, 8, dtype=torch.float16, device=dev)
        x8[..., :3] = (torch.rand(B, R, R, 3, device=dev) * 2 - 1).half()
        E.tiny_block_on = True
        t_fused = timeit(E, lambda: graphs.emit_taesd_encode(E, tW, configs.TAESD, x8))
        E.tiny_block_on = False
        t_three = timeit(E, lambda: graphs.emit_taesd_encode(E, tW, configs.TAESD, x8))
        E.tiny_block_on = True
        t_kl = timeit(E, lambda: graphs.emit_vae_encode_moments(E, kW, configs.SD_TURBO_VAE, x8), iters=5)
        res[f"encoder_B{B}_{R}"] = dict(fused_ms=t_fused, three_launch_ms=t_three, kl_ms=t_kl)
        print(f"encoder B={B} {R}^2: taesd fused {t_fused:8.3f} ms | taesd three-launch {t_three:8.3f} ms | AutoencoderKL {t_kl:8.3f} ms", flush=True)

    B = args.block_batch
    p = "encoder.layers.3"
    ws = [tW[f"{p}.conv.{k}.weight"] for k in (0, 2, 4)]
    bs = [tW[f"{p}.conv.{k}.bias"] for k in (0, 2, 4)]
    for H in (512, 256, 128, 64):
        x = torch.randn(B, H, H, 64, device=dev).half()
        out = torch.empty_like(x)
        t_f = timeit(E, lambda: E.tiny_block(x, ws, bs, out=out))
        t_3 = timeit(E, lambda: graphs._emit_tiny_block(E, tW, p, x))
        fl = 3 * 2.0 * B * H * H * 64 * 576
        res[f"block_B{B}_{H}"] = dict(fused_ms=t_f, three_launch_ms=t_3, fused_tflops=fl / t_f / 1e9, three_launch_tflops=fl / t_3 / 1e9)
        print(f"block B={B} {H}^2: fused {t_f * 1e3:8.1f} us ({fl / t_f / 1e9:6.1f} TF/s) | three-launch {t_3 * 1e3:8.1f} us "
              f"({fl / t_3 / 1e9:6.1f} TF/s) | {t_3 / t_f:5.2f}x", flush=True)

    if args.train:
        res.update(train_steps(dev, R, args.block_batch, args.train_steps, args.use_8bit_adam))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def train_steps(dev, R, B, steps, use_8bit_adam=False):
    """one SD-Turbo ControlNet train step (bench_train.py's synthetic set-up) with the default VAE and with --tiny_vae"""
    from genima_amd.packing import pack_state_dict
    from genima_amd.scheduler import DDPMScheduler
    from genima_amd.training import ControlNetTrainer

    fam = configs.family("sd-turbo")
    synth = lambda sch, seed: weights.synth_state_dict(sch, seed, device=dev)  # noqa: E731
    unet_W = pack_state_dict(synth(schema.unet_schema(fam["unet"]), 1), dev, up_phases=False)
    text_W = pack_state_dict(synth(schema.clip_text_schema(fam["text"]), 4), dev)
    vaes = {False: (fam["vae"], pack_state_dict(synth(schema.vae_schema(fam["vae"]), 3), dev)),
            True: (configs.TAESD, pack_state_dict(synth(schema.taesd_schema(configs.TAESD), 3), dev))}
    g = torch.Generator(device=dev).manual_seed(77)
    V = fam["text"]["vocab_size"]
    ids = torch.zeros(B, 77, dtype=torch.int32)
    ids[:, :14] = torch.tensor([V - 2] + [320 + i for i in range(12)] + [V - 1], dtype=torch.int32)
    px = torch.zeros(B, R, R, 8, dtype=torch.float16, device=dev)
    px[..., :3] = (torch.rand(B, R, R, 3, generator=g, device=dev) * 2 - 1).half()
    cond = torch.zeros(B, R, R, 8, dtype=torch.float16, device=dev)
    cond[..., :3] = torch.rand(B, R, R, 3, generator=g, device=dev).half()
    batch = dict(pixel_values=px, conditioning_pixel_values=cond, input_ids=ids.to(dev))
    out = {}
    for tiny in (False, True):
        E = Engine(dev, autotune=True)
        tr = ControlNetTrainer(E, fam["unet"], fam["controlnet"], unet_W, synth(schema.controlnet_schema(fam["controlnet"]), 2), lr=1e-5,
                               use_8bit_adam=use_8bit_adam)
        tr.attach_frozen(vaes[tiny][0], vaes[tiny][1], fam["text"], text_W, DDPMScheduler(), seed=1234, tiny_vae=tiny)
        for _ in range(3):
            tr.train_step(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.train_step(batch)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[f"train_step_B{B}_{R}_{'tiny_vae' if tiny else 'kl_vae'}_ms"] = ms
        print(f"train step B={B} {R}^2 {'--tiny_vae' if tiny else 'default VAE'}: {ms:8.2f} ms (loss {float(loss):.4f})", flush=True)
        del tr, E
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
