"""B = 1 controller call (full-size ACT, ``act_tiled`` on a 512 x 512 tile) with and without the action-ensemble op
(``GenimaACT.set_execution(5, True)``), alternating in one process: 9 blocks of 60 individually synchronised calls per setting, the op-less
call as baseline; then the op alone (HIP events around a replay of that one op of the recorded program).

    python tools/bench_ensemble.py [--out profiles/ensemble_b1_timing.json]

With ``--samples 1,2,4,8``: the full-size B = 1 tiled control call under ``set_execution(5, True, samples=R)`` for each R -- the diffusion
pipeline at batch R (5 steps, one observation and one prompt repeated, R latents), ``act_tiled`` on its R images, the combining op at the end
of the controller's program -- beside the call without samples, the settings alternating in one process: medians of individually
synchronised calls with min and max; then the new op alone beside ``gn_action_ensemble_f16``'s, between HIP events as above.

    python tools/bench_ensemble.py --samples 1,2,4,8 [--combine mean] [--out profiles/ensemble_samples_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from genima_amd import configs, weights
from genima_amd.act import GenimaACT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--samples", default=None, metavar="R[,R..]", help="time the whole tiled control call with R sampled chunks per observation")
ap.add_argument("--combine", default="mean", choices=("mean", "medoid"))
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--calls", type=int, default=12)
args = ap.parse_args()


def stats(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), n=len(v))


def op_alone_us(E, reps=50):
    """The last op of a recorded program, replayed alone between HIP events."""
    e0, e1 = E.event(), E.event()
    n = E.num_ops
    one = []
    for _ in range(reps):
        E.event_record(e0); E.run(n - 1, n); E.event_record(e1)
        E.synchronize()
        one.append(E.event_elapsed_ms(e0, e1) * 1e3)
    return round(statistics.median(one), 3), round(min(one), 3), round(max(one), 3)


def bench_samples():
    from genima_amd.pipeline import StableDiffusionControlNetPipeline

    fam = configs.family("sd-turbo")
    dev = torch.device("cuda", 0)
    pipe = StableDiffusionControlNetPipeline.from_synthetic(fam, seed=0, gen_device=dev)
    pipe.to(dev)
    for m in (pipe.vae, pipe.text_encoder, pipe.unet, pipe.controlnet):
        m._sd = None
    torch.cuda.empty_cache()
    agent = GenimaACT(fam["act"], None, fam["act_text"], None, device=dev, seed=0)
    Rs = [int(r) for r in args.samples.split(",")]
    V, Vc = pipe.text_encoder.config["vocab_size"], fam["act_text"]["vocab_size"]
    img1 = torch.from_numpy(weights.counter_bytes(100, "bench_ctrl", 512 * 512 * 3).reshape(1, 512, 512, 3)).to(dev)
    st1 = torch.randn(1, 1, fam["act"]["state_dim"], generator=torch.Generator().manual_seed(7)).to(dev)
    inputs = {}
    for R in sorted(set(Rs) | {1}):
        ids = torch.zeros(R, 77, dtype=torch.int32)
        ids[:, :14] = torch.tensor([V - 2] + [320 + i for i in range(12)] + [V - 1], dtype=torch.int32)
        tok = torch.zeros(R, 1, 77, dtype=torch.int32)
        tok[:, 0, :14] = torch.tensor([Vc - 2] + [320 + i for i in range(12)] + [Vc - 1], dtype=torch.int32)
        lat = torch.randn(R, 4, 64, 64, generator=torch.Generator().manual_seed(2)).to(torch.float16)
        inputs[R] = (ids.to(dev), img1.expand(R, -1, -1, -1).contiguous(), lat.to(dev), st1.expand(R, -1, -1).contiguous(), tok.to(dev))

    def call(R, sampled, step):
        ids, img, lat, st, tok = inputs[R]
        out = pipe(prompt_ids=ids, image=img, latents=lat, num_inference_steps=5, guidance_scale=0.0, output_type="pt")
        if sampled:
            agent.set_execution(5, True, samples=R, combine=args.combine) if agent.execution_samples != (R, args.combine) else None
        elif agent.execution is not None:
            agent.set_execution()
        return agent.act_tiled(out.images, st, tok, step=step)

    settings = [("plain_b1", 1, False)] + [(f"samples_{R}", R, True) for R in Rs]
    times = {k: [] for k, _, _ in settings}
    for k, R, sampled in settings:  # record and warm every program
        for i in range(3):
            call(R, sampled, 5 * i)
        torch.cuda.synchronize()
    for b in range(args.blocks):
        for k, R, sampled in settings:
            call(R, sampled, 0)
            for i in range(args.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(R, sampled, 5 * (i + 1))
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in times.items()}
    base = out["plain_b1"]["median_ms"]
    for k, R, sampled in settings[1:]:
        out[k]["over_plain_b1"] = round(out[k]["median_ms"] / base, 4)
        out[k]["over_R_plain_calls"] = round(out[k]["median_ms"] / (R * base), 4)
    ops = {}
    for R in Rs:  # the op alone: the last op of each sampled program, and gn_action_ensemble_f16's of the B = 1 execution program
        io = [p for p in agent._progs.values() if p.samples == (R, args.combine)][0]
        ops[f"samples_{R}_op_us"] = dict(zip(("median", "min", "max"), op_alone_us(io.engine)))
    agent.set_execution(5, True)
    ids, img, lat, st, tok = inputs[1]
    agent.act_tiled(pipe(prompt_ids=ids, image=img, latents=lat, num_inference_steps=5, guidance_scale=0.0, output_type="pt").images, st, tok, step=0)
    io = [p for p in agent._progs.values() if p.exec is not None and p.samples is None][0]
    ops["action_ensemble_f16_op_us"] = dict(zip(("median", "min", "max"), op_alone_us(io.engine)))
    out["op_alone"] = ops
    out["combine"], out["device"] = args.combine, torch.cuda.get_device_name(0)
    out["what"] = ("pipe (sd-turbo, 5 steps, batch R) + GenimaACT.act_tiled (R rows) under set_execution(5, True, samples=R), B = 1, ms per synchronised call; "
                   f"{args.blocks} alternating blocks of {args.calls} calls per setting; plain_b1: the call without samples and without an execution mode; "
                   "op_alone: the program's last op replayed between HIP events, 50 times")
    path = args.out or os.path.join(ROOT, "profiles", "ensemble_samples_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if args.samples is not None:
    bench_samples()
    sys.exit(0)

fam = configs.family("sd-turbo")
ccfg = dict(configs.TINY_ACT_CLIP_TEXT, projection_dim=512)
agent = GenimaACT(fam["act"], None, ccfg, None, device="cuda", seed=0)
B = 1
tiled = torch.from_numpy(weights.counter_bytes(9, "act", B * 512 * 512 * 3).reshape(B, 512, 512, 3)).cuda()
state = torch.randn(B, 1, fam["act"]["state_dim"], generator=torch.Generator().manual_seed(7)).cuda()
Vc = ccfg["vocab_size"]
toks = torch.zeros(B, 1, 77, dtype=torch.int32)
toks[:, 0, :5] = torch.tensor([Vc - 2, 5, 6, 7, Vc - 1], dtype=torch.int32)

def block(n, step0):
    ts = []
    for i in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.act_tiled(tiled, state, toks, step=step0 + 5 * i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)

res = {"off": [], "on": []}
for mode in ("off", "on"):  # record + warm both programs
    agent.set_execution(5, True) if mode == "on" else agent.set_execution()
    block(10, 0)
for r in range(9):
    for mode in ("off", "on"):
        agent.set_execution(5, True) if mode == "on" else agent.set_execution()
        block(3, 0)
        res[mode].append(block(60, 15))
out = {m: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), blocks=v) for m, v in res.items()}
out["delta_us"] = (out["on"]["median_ms"] - out["off"]["median_ms"]) * 1e3
# the op alone, from the recorded program (HIP events around a replay of its one op)
io = [p for p in agent._progs.values() if p.exec is not None][0]
E = io.engine
e0, e1 = E.event(), E.event()
n = E.num_ops
one = []
for _ in range(50):
    E.event_record(e0); E.run(n - 1, n); E.event_record(e1)
    one.append(E.event_elapsed_ms(e0, e1) * 1e3)
out["op_alone_us_median"] = statistics.median(one)
out["ops"] = n
args.out = args.out or os.path.join(ROOT, "profiles", "ensemble_b1_timing.json")
out["device"] = torch.cuda.get_device_name(0)
out["what"] = "GenimaACT.act_tiled, B = 1, full-size ACT, ms per synchronised call: medians of 9 alternating blocks of 60 calls; op_alone: one op replayed between HIP events"
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({k: v for k, v in out.items() if k not in ("off", "on")}), {m: (out[m]["median_ms"], out[m]["min_ms"], out[m]["max_ms"]) for m in ("off", "on")})
