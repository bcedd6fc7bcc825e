"""What attention-probability dropout costs one ACT update: one full-size ``ACTTrainer.update`` (256^2 images, B = 8, V = 4, the full ACT
config with random weights) at ``attn_dropout`` 0.0 and 0.1, the two trainers alternating update by update in ONE process, this tree at
0.0 alone, and the parent commit's library at 0.0 as the baseline.  The parent has neither the argument nor the new symbols, so its package is imported from a
checkout of its own (``--parent-tree``: a directory holding the parent commit's ``genima_amd/`` with its library built) in a process
of its own, run before and after this tree's process: the two parent runs show the spread of the baseline itself.  Each figure is
the median (with min / max) of ``--reps`` updates after ``--warmup``, a host clock around work that ends in a stream synchronise.

Prints one JSON line; needs an MI355X.

    python tools/bench_act_attn_dropout.py --parent-tree DIR [--batch 8] [--reps 20] [--warmup 3] [--out line.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def child(args):
    """Time ACTTrainer.update of the package under ``args.tree`` at each of ``args.rates``, alternating -> one JSON line {rate: stats}."""
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    from genima_amd import configs, weights
    from genima_amd.act_training import ACTTrainer, act_train_schema
    from genima_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_act_attn_dropout: no ROCm device (this tool measures on the GPU only)")
    B, V, S = args.batch, 4, 256
    cfg = dict(configs.ACT_POLICY, image_size=S, num_views=V)
    E = Engine(torch.device("cuda", 0))
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (B, V, S, S, 3), generator=g, dtype=torch.uint8).cuda()
    sd = weights.round_to(weights.synth_state_dict(act_train_schema(cfg), 61), torch.float16)
    for k in sd:
        if k.endswith("running_var"):
            sd[k] = sd[k].abs() + 0.5
    qpos = torch.randn(B, cfg["state_dim"], generator=g)
    task = torch.randn(B, cfg["lang_dim"], generator=g) * 0.5
    actions = torch.randn(B, cfg["num_queries"], cfg["action_dim"], generator=g)
    actions[..., -1] = (actions[..., -1] > 0).float()
    rates = [float(r) for r in args.rates.split(",")]
    # (the parent's trainer has no attn_dropout argument: it is passed only where it is not 0)
    trainers = {r: ACTTrainer(E, cfg, sd, configs.ACT_CLIP_TEXT, None, **({"attn_dropout": r} if r > 0 else {})) for r in rates}
    ms = {r: [] for r in rates}
    for i in range(args.warmup + args.reps):
        for r in rates:
            E.synchronize()
            t = time.perf_counter()
            trainers[r].update(imgs, qpos, task, actions)
            E.synchronize()
            if i >= args.warmup:
                ms[r].append((time.perf_counter() - t) * 1e3)
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "rates": {str(r): stats(ms[r]) for r in rates}}), flush=True)


def run_child(tree, rates, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--rates", rates, "--batch", str(args.batch), "--reps", str(args.reps),
           "--warmup", str(args.warmup)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:
        raise SystemExit(f"bench_act_attn_dropout: the run on {tree} failed (exit {out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit (its genima_amd/ with libgenima_hip.so built)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--rates", default="0.0,0.1", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"tool": "bench_act_attn_dropout", "batch": args.batch, "views": 4, "size": 256, "reps": args.reps, "warmup": args.warmup}
    # a failed run ends the tool (run_child raises): nothing more is started on the device after it
    if args.parent_tree:
        res["parent_0.0_before"] = run_child(args.parent_tree, "0.0", args)["rates"]["0.0"]
    # this tree at 0.0 in a process of its own: the parent's conditions (in the alternating pair below, two trainers share the caches)
    res["attn_dropout_0.0_alone"] = run_child(HERE, "0.0", args)["rates"]["0.0"]
    new = run_child(HERE, "0.0,0.1", args)
    res["device"] = new["device"]
    res["attn_dropout_0.0"], res["attn_dropout_0.1"] = new["rates"]["0.0"], new["rates"]["0.1"]
    if args.parent_tree:
        res["parent_0.0_after"] = run_child(args.parent_tree, "0.0", args)["rates"]["0.0"]
        med = [res[k]["median_ms"] for k in ("parent_0.0_before", "parent_0.0_after")]
        res["parent_0.0"] = {"median_ms": round(sum(med) / 2, 4), "spread_ms": round(abs(med[0] - med[1]), 4)}
    res["dropout_0.1_minus_0.0_ms"] = round(res["attn_dropout_0.1"]["median_ms"] - res["attn_dropout_0.0"]["median_ms"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
