"""What the ACT trainer's ElasticTransform costs per update step, with its displacement field blurred on the host (f64 numpy, the default)
and on the device (gn_elastic_field, ``field="device"``), next to one ``ACTTrainer.update``: 256^2 images, B = 8, V = 4, the full ACT
config with random weights.  Three things are timed, each with a host clock around work that ends in a stream synchronise (the host
route's cost IS host time), after warm-up, the two routes alternating inside every repetition:

  elastic branch   the field, its upload and the warp launch          (elastic_displacement[_device] + gn_warp_bilinear)
  act_augment      the whole chain with every RandomApply taken (p = 1): elastic, colour jitter, crop, Gaussian noise
  update           ACTTrainer.update on an already augmented batch

Prints one JSON line (medians in ms, with min / max); needs an MI355X.

    python tools/bench_act_augment.py [--batch 8] [--views 4] [--size 256] [--reps 20] [--warmup 3] [--out line.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import configs, weights  # noqa: E402
from genima_amd._lib import check  # noqa: E402
from genima_amd.act_training import (ACTTrainer, act_augment, act_train_schema, elastic_displacement,  # noqa: E402
                                     elastic_displacement_device)
from genima_amd.engine import Engine  # noqa: E402


def timed(E, fn):
    E.synchronize()
    t = time.perf_counter()
    fn()
    E.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_act_augment: no ROCm device (this tool measures on the GPU only)")
    dev = torch.device("cuda", 0)
    B, V, S = args.batch, args.views, args.size
    cfg = dict(configs.ACT_POLICY, image_size=S, num_views=V)
    E = Engine(dev)
    g = torch.Generator().manual_seed(0)
    img_u8 = torch.randint(0, 256, (B, V, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    x = E.image_u8_to_f16(img_u8.view(B * V, S, S, 3), 8, 1.0, 0.0)
    y = torch.empty_like(x)

    def branch(route):
        def run():
            if route == "device":
                disp = elastic_displacement_device(E, S, S, generator=g)
            else:
                disp = elastic_displacement(S, S, generator=g).to(E.device)
            check(E.lib.gn_warp_bilinear(E._ctx, x.data_ptr(), y.data_ptr(), disp.data_ptr(), B * V, S, S, 8), "gn_warp_bilinear")
        return run

    def augment(route):
        return lambda: act_augment(E, img_u8, g, p=1.0, field=route)

    res = {"tool": "bench_act_augment", "device": torch.cuda.get_device_name(0), "batch": B, "views": V, "size": S, "reps": args.reps,
           "warmup": args.warmup, "augment_p": 1.0}
    for name, make in (("elastic_branch", branch), ("act_augment", augment)):
        ms = {"host": [], "device": []}
        for i in range(args.warmup + args.reps):
            for route in ("host", "device"):
                t = timed(E, make(route))
                if i >= args.warmup:
                    ms[route].append(t)
        for route in ms:
            res[f"{name}_{route}"] = stats(ms[route])
        res[f"{name}_host_over_device"] = round(res[f"{name}_host"]["median_ms"] / res[f"{name}_device"]["median_ms"], 2)

    sd = weights.round_to(weights.synth_state_dict(act_train_schema(cfg), 61), torch.float16)
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = sd[k].abs() + 0.5
    tr = ACTTrainer(E, cfg, sd, configs.ACT_CLIP_TEXT, None)
    imgs = act_augment(E, img_u8, g, p=1.0, field="device")
    qpos = torch.randn(B, cfg["state_dim"], generator=g)
    task = torch.randn(B, cfg["lang_dim"], generator=g) * 0.5
    actions = torch.randn(B, cfg["num_queries"], cfg["action_dim"], generator=g)
    actions[..., -1] = (actions[..., -1] > 0).float()
    ms = []
    for i in range(args.warmup + args.reps):
        t = timed(E, lambda: tr.update(imgs, qpos, task, actions))
        if i >= args.warmup:
            ms.append(t)
    res["update"] = stats(ms)
    res["device_branch_below_one_update"] = res["elastic_branch_device"]["median_ms"] < res["update"]["median_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
