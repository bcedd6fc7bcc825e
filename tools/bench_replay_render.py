"""What drawing the ACT controller's random-background batch costs against gathering it from stored frames: ``tools/bench_act_replay.py``'s
configuration (the full ACT config with random weights, B = 8, V = 4, 256^2, 4 synthetic episodes of 40 steps, ``data_augmentation`` on), the
same transition indices on two routes that alternate inside every repetition:

  (a) gather-mode ``DeviceReplay.sample`` -> ``GenimaACT.update_device``   one ``gn_replay_gather`` launch over frames resident on the device
  (b) render-mode ``DeviceReplay.sample`` -> ``GenimaACT.update_device``   one ``gn_replay_render`` launch over view tables and a texture bank

Each figure is the median (with min / max) of ``--reps`` steps after ``--warmup``, a host clock around work that ends in a stream
synchronise; the two launches alone (device events, 5 x 100 launches) and the bytes each mode keeps on the device are reported beside them.
The claim checked: a rendered step is not slower than a gathered step by more than the run's own min-max spread of the gathered step.

Prints one JSON line; needs an MI355X.

    python tools/bench_replay_render.py [--batch 8] [--reps 20] [--warmup 3] [--episodes 4] [--length 40] [--textures 16]
        [--sphere_textures tests/golden/sphere_textures] [--out profiles/act_replay_render_b8.json]
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
    ap.add_argument("--textures", type=int, default=16, help="layers of the synthetic background bank")
    ap.add_argument("--sphere_textures", default=os.path.join(HERE, "tests", "golden", "sphere_textures"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from genima_amd import configs
    from genima_amd import render as R
    from genima_amd import replay as P
    from genima_amd.act import GenimaACT
    from genima_amd.engine import Engine

    if not torch.cuda.is_available():
        raise SystemExit("bench_replay_render: no ROCm device (this tool measures on the GPU only)")
    B, S = args.batch, 256  # render.synthetic_episode's geometry
    cfg = dict(configs.ACT_POLICY, image_size=S, data_augmentation=True)
    ccfg = configs.ACT_CLIP_TEXT
    E = Engine(torch.device("cuda", 0))

    def tokens(texts):  # a fixed 5-token prompt, the end-of-text id last (the highest id marks the pooled position)
        t = np.zeros((1, 77), np.int32)
        t[0, :5] = [ccfg["vocab_size"] - 2, 3, 4, 5, ccfg["vocab_size"] - 1]
        return t

    gather_eps, render_eps, rcfg = [], [], None
    for e in range(args.episodes):
        demo, frames = P.synthetic_demo(args.length, seed=e, size=S)
        rcfg, traj, _ = R.synthetic_episode(args.length, seed=7 + e, texture_dir=args.sphere_textures, action_horizon=20)
        gather_eps.append((demo, frames, "open the box"))
        render_eps.append((demo, traj, "open the box"))
    bank = np.random.RandomState(3).randint(0, 256, (args.textures, S, S, 3)).astype(np.uint8)
    kw = dict(engine=E, action_sequence=cfg["num_queries"], batch_size=B, tokenizer=tokens)
    replays = {"gather": P.DeviceReplay(gather_eps, **kw), "render": P.DeviceReplay(render_eps, render=P.RenderTargets(rcfg, bank, seed=0), **kw)}
    assert replays["gather"].N == replays["render"].N
    agents = {k: GenimaACT(cfg, None, ccfg, None, device="cuda", seed=4) for k in replays}
    ms = {k: [] for k in replays}
    rp = replays["gather"]
    sampler = iter(P.EpochSampler(rp.N, B, generator=torch.Generator().manual_seed(1)))
    for i in range(args.warmup + args.reps):
        try:
            ix = next(sampler)
        except StopIteration:
            ix = next(iter(sampler))
        for k, agent in agents.items():
            E.synchronize()
            t = time.perf_counter()
            agent.update_device(replays[k].sample(ix), i)
            E.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t) * 1e3)
    # the launches alone, indices already on the device
    idx = next(iter(P.EpochSampler(rp.N, B, generator=torch.Generator().manual_seed(2)))).to(torch.int32).cuda()
    rr = replays["render"]
    g_args = (rp.frame_ptr, rp.qpos, rp.action, rp.obs_index, rp.first_obs, rp.last_tr, idx, (rp.H, rp.W), rp.V, rp.fs, rp.T)
    r_args = (rr.cams, rr.spheres, rr.tex_index, rr.count, rr.atlas, rr.bank, rr.qpos, rr.action, rr.obs_index, rr.first_obs, rr.last_tr, idx, rr.V, rr.fs, rr.T)
    g_out = E.replay_gather(*g_args, lang_tokens=rp.lang_tokens, episode=rp.episode)
    r_out = E.replay_render(*r_args, samples=rr.samples, lang_tokens=rr.lang_tokens, episode=rr.episode)
    launches = {"replay_gather_us": lambda: E.replay_gather(*g_args, lang_tokens=rp.lang_tokens, episode=rp.episode, out=g_out),
                "replay_render_us": lambda: E.replay_render(*r_args, samples=rr.samples, draw=5, lang_tokens=rr.lang_tokens, episode=rr.episode, out=r_out)}
    res = {"tool": "bench_replay_render", "device": torch.cuda.get_device_name(0), "batch": B, "views": rp.V, "size": S, "episodes": args.episodes,
           "length": args.length, "transitions": rp.N, "textures": args.textures, "samples": rr.samples, "reps": args.reps, "warmup": args.warmup,
           "data_augmentation": True, "gather_device_mb": round(rp.device_bytes / 1e6, 3), "render_device_mb": round(rr.device_bytes / 1e6, 3),
           "render_device_bytes": {"view_tables": int(sum(t.nbytes for t in rr.host_views.values())), "bank": int(rr.host_bank.nbytes),
                                   "atlas": int(rr.host_atlas.nbytes)}}
    res["gather_update_device"], res["render_update_device"] = stats(ms["gather"]), stats(ms["render"])
    g, r = res["gather_update_device"], res["render_update_device"]
    res["render_minus_gather_ms"] = round(r["median_ms"] - g["median_ms"], 4)
    res["gather_spread_ms"] = round(g["max_ms"] - g["min_ms"], 4)
    res["render_within_gather_spread"] = bool(res["render_minus_gather_ms"] <= res["gather_spread_ms"])
    for name, launch in launches.items():
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
        res[name] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
