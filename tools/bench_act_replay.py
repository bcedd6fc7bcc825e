"""What the host share of one ACT training step costs, and what the device-resident replay saves: the full ACT config with random weights,
B = 8, V = 4, 256^2 frames of ``synthetic_demo`` episodes, ``data_augmentation`` on (the agents' own fixed generator), the same transition
indices on two routes that alternate inside every repetition:

  (a) ``DeviceReplay.host_batch`` -> ``GenimaACT.update``        the batch is assembled on the host, uploaded and converted per step
  (b) ``DeviceReplay.sample``     -> ``GenimaACT.update_device`` one ``gn_replay_gather`` launch on frames that never left the device

Each figure is the median (with min / max) of ``--reps`` steps after ``--warmup``, a host clock around work that ends in a stream
synchronise; ``host_batch`` alone (numpy, no device work) and the ``gn_replay_gather`` launch alone (device events) are reported beside them.

Prints one JSON line; needs an MI355X.

    python tools/bench_act_replay.py [--batch 8] [--reps 20] [--warmup 3] [--episodes 4] [--length 40] [--out profiles/act_replay_b8.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from genima_amd import configs
    from genima_amd import replay as P
    from genima_amd.act import GenimaACT
    from genima_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_act_replay: no ROCm device (this tool measures on the GPU only)")
    B, S = args.batch, args.size
    cfg = dict(configs.ACT_POLICY, image_size=S, data_augmentation=True)
    ccfg = configs.ACT_CLIP_TEXT
    E = Engine(torch.device("cuda", 0))

    def tokens(texts):  # a fixed 5-token prompt, the end-of-text id last (the highest id marks the pooled position)
        t = np.zeros((1, 77), np.int32)
        t[0, :5] = [ccfg["vocab_size"] - 2, 3, 4, 5, ccfg["vocab_size"] - 1]
        return t

    eps = [P.synthetic_demo(args.length, seed=e, size=S) + ("open the box",) for e in range(args.episodes)]
    rp = P.DeviceReplay(eps, engine=E, action_sequence=cfg["num_queries"], batch_size=B, tokenizer=tokens, generator=torch.Generator().manual_seed(0))
    agents = {"host_batch_update": GenimaACT(cfg, None, ccfg, None, device="cuda", seed=4),
              "sample_update_device": GenimaACT(cfg, None, ccfg, None, device="cuda", seed=4)}
    ms = {k: [] for k in agents}
    ms["host_batch_alone"] = []
    sampler = iter(P.EpochSampler(rp.N, B, generator=torch.Generator().manual_seed(1)))
    for i in range(args.warmup + args.reps):
        try:
            ix = next(sampler)
        except StopIteration:
            ix = next(iter(sampler))
        for k, agent in agents.items():
            E.synchronize()
            t = time.perf_counter()
            if k == "host_batch_update":
                hb = rp.host_batch(ix)
                t_hb = time.perf_counter() - t
                agent.update(iter([hb]), i)
            else:
                agent.update_device(rp.sample(ix), i)
            E.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t) * 1e3)
                if k == "host_batch_update":
                    ms["host_batch_alone"].append(t_hb * 1e3)
    # the launch alone, indices already on the device
    idx = next(iter(P.EpochSampler(rp.N, B, generator=torch.Generator().manual_seed(2)))).to(torch.int32).cuda()
    out = E.replay_gather(rp.frame_ptr, rp.qpos, rp.action, rp.obs_index, rp.first_obs, rp.last_tr, idx, (rp.H, rp.W), rp.V, rp.fs, rp.T,
                          lang_tokens=rp.lang_tokens, episode=rp.episode)

    def launch():
        E.replay_gather(rp.frame_ptr, rp.qpos, rp.action, rp.obs_index, rp.first_obs, rp.last_tr, idx, (rp.H, rp.W), rp.V, rp.fs, rp.T,
                        lang_tokens=rp.lang_tokens, episode=rp.episode, out=out)

    us = []
    for _ in range(5):
        for _ in range(10):
            launch()
        a, e = E.event(), E.event()
        E.event_record(a)
        for _ in range(100):
            launch()
        E.event_record(e)
        E.synchronize()
        us.append(E.event_elapsed_ms(a, e) / 100 * 1e3)
    res = {"tool": "bench_act_replay", "device": torch.cuda.get_device_name(0), "batch": B, "views": rp.V, "size": S, "episodes": args.episodes,
           "length": args.length, "transitions": rp.N, "replay_device_mb": round(rp.device_bytes / 1e6, 1), "reps": args.reps, "warmup": args.warmup,
           "data_augmentation": True}
    res.update({k: stats(v) for k, v in ms.items()})
    res["device_minus_host_ms"] = round(res["sample_update_device"]["median_ms"] - res["host_batch_update"]["median_ms"], 4)
    bytes_moved = B * rp.V * rp.fs * S * S * (3 + 16)
    res["replay_gather_us"] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
                               "tb_per_s": round(bytes_moved / (statistics.median(us) * 1e-6) / 1e12, 3)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
