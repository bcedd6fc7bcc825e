"""What one batch of the open-loop evaluation costs against the bare joint call it wraps: full-size networks with synthetic weights (SD-Turbo +
ControlNet, the full ACT config), B = 8, V = 4, 256^2 views, synthetic episodes, one process, two routes on the same batch that alternate
inside every repetition:

  (a) the bare joint call: the pipeline (``output_type="pt"``) -> ``GenimaACT.act_tiled``
  (b) one evaluator batch (``OpenLoopEval.run_batch``): sample -> ``gn_render_spheres`` -> tile -> pipeline -> ``act_tiled`` -> image, sphere
      and action scores -> the oracle controller pass on the rendered target -> its action scores

Each figure is the median (with min / max) of ``--reps`` individually synchronised repetitions after ``--warmup``, a host clock around work
that ends in a stream synchronise.  The oracle controller pass alone is timed the same way, and the four launches -- the three metric kernels
and ``gn_render_spheres`` -- by device events (5 x 100 launches).  The claim checked: (b) costs no more than (a) plus the run's own min-max
spread of (a).

With ``--exec_grid`` it also times whole runs (``OpenLoopEval.run``: every batch plus the final device-to-host copy) of two evaluators over the
same agents that alternate inside every repetition -- one without ``executions`` (what the evaluator did before execution modes could be
replayed) and one with the grid (h, temporal_agg, m) in {1, 5, 10, 20} x {off, on} x {0.01} -- and the two replay launches
(``gn_openloop_exec_actions`` with h = 5 and temporal_agg, ``gn_openloop_exec_metrics``) by device events.  The claim checked there: the grid
adds a few launch-shaped kernels per setting and nothing to a run without it.

With ``--triangulate`` it times whole runs of two evaluators that alternate in the same way -- one without and one with ``triangulate=True``
-- and the ``gn_openloop_triangulate`` launch over the run's whole table by device events.  The expectation checked there: one small launch
and N * G * 128 more bytes in the final copy do not show next to the diffusion calls.

With ``--orientation`` it times whole runs of two evaluators that alternate in the same way -- one without and one with ``orientation=37``
-- and reports both per transition, the difference as a share of the run without it, and the ``gn_openloop_orientation`` launch over one
batch at K = 37 by device events (the shifts are those of the batch's own sphere table).

With ``--seeds R`` it times whole runs of two evaluators that alternate in the same way -- one without and one with ``seeds=R`` -- and
reports both per transition, their ratio (the expectation: about R generations beside one, less the work done once per batch -- the targets
and the oracle pass), the bytes the seed tables add to the final copy, and the two new launches over the finished tables of a whole run by
device events (``gn_openloop_seed_spheres``, ``gn_openloop_seed_actions`` with the joint scale).  There is no target: the cost is R
generations and is the user's to choose.

With ``--perturb SPEC`` (a preset or a spec of ``genima_amd.perturb.parse``) it times one evaluator batch (``run_batch``) of two evaluators
over the same agents that alternate inside every repetition -- one clean and one with ``perturb=SPEC`` -- and the ``gn_view_perturb`` launch
alone over one batch's frames by device events (its zeroing of the revealed counts included), beside the bytes it reads and writes.  No time
is promised: the perturbed batch is reported beside the clean batch of the same process.

Prints one JSON line; needs an MI355X.

    python tools/bench_openloop.py [--batch 8] [--reps 10] [--warmup 2] [--episodes 2] [--length 12] [--exec_grid] [--triangulate] [--orientation] [--seeds R] [--perturb SPEC]
        [--sphere_textures tests/golden/sphere_textures] [--out profiles/openloop_b8.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--length", type=int, default=12)
    ap.add_argument("--family", default="sd-turbo")
    ap.add_argument("--sphere_textures", default=os.path.join(HERE, "tests", "golden", "sphere_textures"))
    ap.add_argument("--exec_grid", action="store_true", help="also time whole runs without and with the 8-setting execution grid, and the two replay launches")
    ap.add_argument("--triangulate", action="store_true", help="also time whole runs without and with triangulate=True, and the triangulation launch")
    ap.add_argument("--orientation", action="store_true", help="also time whole runs without and with orientation=37, and the orientation launch")
    ap.add_argument("--seeds", type=int, default=None, metavar="R", help="also time whole runs without and with seeds=R, and the two seed-axis launches")
    ap.add_argument("--combine", default=None, metavar="RULE[,RULE]",
                    help="with --seeds: also time the sample-combined replay launches (mean, medoid) over the seed run's chunk table, at execution (5, agg)")
    ap.add_argument("--perturb", default=None, metavar="SPEC", help="also time one evaluator batch clean and under this perturbation, and the gn_view_perturb launch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from genima_amd import configs
    from genima_amd import render as R
    from genima_amd import replay as P
    from genima_amd.act import GenimaACT
    from genima_amd.agent import SDControlNetAgent
    from genima_amd.engine import Engine
    from genima_amd.openloop import OpenLoopEval

    if not torch.cuda.is_available():
        raise SystemExit("bench_openloop: no ROCm device (this tool measures on the GPU only)")
    B, S, cams = args.batch, 256, P.DEFAULT_CAMERAS
    tiny = args.family == "tiny"
    ccfg = configs.TINY_ACT_CLIP_TEXT if tiny else configs.ACT_CLIP_TEXT
    E = Engine(torch.device("cuda", 0))

    def tokens(texts):  # a fixed 5-token prompt, the end-of-text id last (the highest id marks the pooled position)
        t = np.zeros((1, 77), np.int32)
        t[0, :5] = [ccfg["vocab_size"] - 2, 3, 4, 5, ccfg["vocab_size"] - 1]
        return t

    eps, demos, rcfg = [], [], None
    for e in range(args.episodes):
        demo, frames = P.synthetic_demo(args.length, seed=e, size=S, cameras=cams)
        rcfg, traj, _ = R.synthetic_episode(args.length, seed=7 + e, texture_dir=args.sphere_textures, action_horizon=4)
        eps.append((demo, frames, traj, "open the box"))
        demos.append(demo)
    ns = types.SimpleNamespace(diffusion_ckpt="", sd_ckpt=f"synthetic:{args.family}", device="cuda", image_resolution=2 * S, vae_slicing=False,
                               upcast_vae=False, fused_projections=True, enable_xformers_memory_efficient_attention=True,
                               show_diffusion_progress=False, torch_compile=False, autoencoder="")
    dagent = SDControlNetAgent(ns)
    controller = GenimaACT(dict(configs.TINY_ACT_POLICY if tiny else configs.ACT_POLICY, image_size=S), None, ccfg, None, device="cuda", seed=4)
    ev = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                      batch_size=B, engine=E)
    tabs = ev._tables()
    gen = torch.Generator(device="cuda").manual_seed(0)
    idx = ev.batch_indices(0)
    with torch.inference_mode():
        batch = ev.targets(idx)
    ids = ev.prompt_ids[torch.from_numpy(ev.episode_index[idx].astype(np.int64))]

    def bare():
        with torch.inference_mode():
            out = dagent.pipe(prompt_ids=ids, image=batch["tiled"], num_inference_steps=ev.num_inference_steps, guidance_scale=ev.guidance_scale,
                              generator=gen, output_type="pt").images
            return out, controller.act_tiled(out, batch["low_dim_state"], batch["lang_tokens"])

    def oracle():
        with torch.inference_mode():
            return ev._chunk(batch["full"].view(B, ev.V, S, S, 3), batch)

    routes = {"bare_joint_call": bare, "evaluator_batch": lambda: ev.run_batch(0, tabs, gen), "oracle_controller_pass": oracle}
    ms = {k: [] for k in routes}
    for i in range(args.warmup + args.reps):
        for k, fn in routes.items():
            E.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms[k].append((time.perf_counter() - t) * 1e3)
    res = {"tool": "bench_openloop", "device": torch.cuda.get_device_name(0), "family": args.family, "batch": B, "views": ev.V, "size": S,
           "transitions": ev.N, "num_inference_steps": ev.num_inference_steps, "reps": args.reps, "warmup": args.warmup}
    for k in routes:
        res[k] = stats(ms[k])
    a, b = res["bare_joint_call"], res["evaluator_batch"]
    res["evaluator_minus_bare_ms"] = round(b["median_ms"] - a["median_ms"], 4)
    res["bare_spread_ms"] = round(a["max_ms"] - a["min_ms"], 4)
    res["evaluator_within_bare_spread"] = bool(res["evaluator_minus_bare_ms"] <= res["bare_spread_ms"])
    # the four launches alone
    out_img, a_hat = bare()
    sel = torch.from_numpy(idx).cuda()
    v = {k: t.index_select(0, sel).reshape((B * ev.V,) + tuple(t.shape[2:])).contiguous() for k, t in ev.views.items()}
    frames = batch["images_u8"].view(B * ev.V, S, S, 3)
    launches = {"image_metrics_us": lambda: E.openloop_image_metrics(out_img, batch["full"], batch["occupied"], tabs["image"]),
                "sphere_metrics_us": lambda: E.openloop_sphere_metrics(out_img, batch["full"], frames, batch["occupied"], batch["windows"], tabs["spheres"],
                                                                       threshold=ev.change_threshold),
                "action_metrics_us": lambda: E.openloop_action_metrics(a_hat, batch["action"], tabs["generated"]["rad"], joint_scale=ev.joint_std),
                "render_spheres_us": lambda: E.render_spheres(v["cams"], v["spheres"], v["tex_index"], v["count"], ev.atlas, S, S, ev.samples, bg=frames,
                                                              full=batch["full"], occupied=batch["occupied"])}
    if args.exec_grid:
        grid = [(h, agg, 0.01) for h in (1, 5, 10, 20) for agg in (False, True)]
        ev_grid = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                               batch_size=B, engine=E, executions=grid)
        runs = {"run_plain": ev.run, "run_with_grid": ev_grid.run}
        rms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():
                E.synchronize()
                t = time.perf_counter()
                fn()  # ends in its device-to-host copy
                torch.cuda.synchronize()
                if i >= args.warmup:
                    rms[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            res[k] = stats(rms[k])
        res["exec_grid"] = [list(g) for g in grid]
        res["grid_minus_plain_ms"] = round(res["run_with_grid"]["median_ms"] - res["run_plain"]["median_ms"], 4)
        res["plain_spread_ms"] = round(res["run_plain"]["max_ms"] - res["run_plain"]["min_ms"], 4)
        res["grid_launches_per_run"] = 3 * 2 * len(grid)  # per setting and row kind: one replay, two scores
        xt = ev_grid._tables()
        ev_grid.run_batch(0, xt, gen)
        x_acts = E.openloop_exec_actions(xt["chunks"]["oracle"], ev_grid.first_tr, 5, True, 0.01)
        x_out = torch.empty((ev.N, 4), dtype=torch.float32, device=E.device)
        launches["exec_actions_us"] = lambda: E.openloop_exec_actions(xt["chunks"]["oracle"], ev_grid.first_tr, 5, True, 0.01, out=x_acts)
        launches["exec_metrics_us"] = lambda: E.openloop_exec_metrics(x_acts, ev_grid.replay.action, ev_grid.first_tr, x_out, joint_scale=ev_grid.joint_std)
    if args.triangulate:
        ev_tri = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                              batch_size=B, engine=E, triangulate=True)
        runs = {"run_without_triangulate": ev.run, "run_with_triangulate": ev_tri.run}
        rms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():
                E.synchronize()
                t = time.perf_counter()
                fn()  # ends in its device-to-host copy
                torch.cuda.synchronize()
                if i >= args.warmup:
                    rms[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            res[k] = stats(rms[k])
        res["triangulate_minus_plain_ms"] = round(res["run_with_triangulate"]["median_ms"] - res["run_without_triangulate"]["median_ms"], 4)
        res["run_without_triangulate_spread_ms"] = round(res["run_without_triangulate"]["max_ms"] - res["run_without_triangulate"]["min_ms"], 4)
        res["triangulate_groups"] = int(ev_tri.point_slots_host.shape[1])
        res["triangulate_extra_copy_bytes"] = int(ev_tri.N * ev_tri.point_slots_host.shape[1] * 128)
        tt = ev_tri._tables()
        for start in range(0, ev_tri.N, B):  # every batch: the launch below is timed over the finished table of a whole run
            ev_tri.run_batch(start, tt, gen)
        t_out = ev_tri.triangulate_spheres(tt)
        launches["triangulate_us"] = lambda: E.openloop_triangulate(tt["spheres"], ev_tri.windows, ev_tri.views["cams"], ev_tri.point_slots, ev_tri.point_centres,
                                                                    t_out, min_ratio=ev_tri.tri_min_ratio, min_det=ev_tri.tri_min_det)
    if args.orientation:
        ev_ori = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                              batch_size=B, engine=E, orientation=37)
        runs = {"run_without_orientation": ev.run, "run_with_orientation": ev_ori.run}
        rms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():
                E.synchronize()
                t = time.perf_counter()
                fn()  # ends in its device-to-host copy
                torch.cuda.synchronize()
                if i >= args.warmup:
                    rms[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            res[k] = stats(rms[k])
            res[k + "_ms_per_transition"] = round(res[k]["median_ms"] / ev.N, 4)
        res["orientation_minus_plain_ms"] = round(res["run_with_orientation"]["median_ms"] - res["run_without_orientation"]["median_ms"], 4)
        res["orientation_share_of_run"] = round(res["orientation_minus_plain_ms"] / res["run_without_orientation"]["median_ms"], 5)
        res["run_without_orientation_spread_ms"] = round(res["run_without_orientation"]["max_ms"] - res["run_without_orientation"]["min_ms"], 4)
        res["orientation_candidates"] = int(ev_ori.orientation_rot.shape[0])
        res["orientation_extra_copy_bytes"] = int(ev_ori.N * ev_ori.V * ev_ori.windows.shape[2] * ev_ori.orientation_rot.shape[0] * 32)
        ot = ev_ori._tables()
        ev_ori.run_batch(0, ot, gen)  # fills the batch's rows of the sphere table: the shifts below are a real batch's
        o_shift = ev_ori.sphere_shifts(ot["spheres"][:B], B)
        launches["orientation_us"] = lambda: E.openloop_orientation(out_img, batch["full"], batch["occupied"], batch["windows"], v["cams"], v["spheres"],
                                                                    v["tex_index"], v["count"], ev.atlas, ev_ori.orientation_rot, ot["orientation"],
                                                                    samples=ev.samples, shift=o_shift)
        launches["sphere_shifts_us"] = lambda: ev_ori.sphere_shifts(ot["spheres"][:B], B)
    if args.seeds is not None:
        ev_seeds = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                                batch_size=B, engine=E, seeds=args.seeds)
        runs = {"run_without_seeds": ev.run, "run_with_seeds": ev_seeds.run}
        rms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():
                E.synchronize()
                t = time.perf_counter()
                fn()  # ends in its device-to-host copy
                torch.cuda.synchronize()
                if i >= args.warmup:
                    rms[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            res[k] = stats(rms[k])
            res[k + "_ms_per_transition"] = round(res[k]["median_ms"] / ev.N, 4)
        res["seeds"] = int(args.seeds)
        res["seeds_over_plain"] = round(res["run_with_seeds"]["median_ms"] / res["run_without_seeds"]["median_ms"], 4)
        res["run_without_seeds_spread_ms"] = round(res["run_without_seeds"]["max_ms"] - res["run_without_seeds"]["min_ms"], 4)
        st = ev_seeds._tables()
        gens = [torch.Generator(device="cuda").manual_seed(r) for r in range(args.seeds)]
        for start in range(0, ev_seeds.N, B):  # every batch: the launches below are timed over the finished tables of a whole run
            ev_seeds.run_batch(start, st, gens)
        s_sph, s_act = ev_seeds.seed_reductions(st)
        whole = st["seed"]
        plain_bytes = sum(t.numel() * t.element_size() for t in [st["image"], st["spheres"]] + list(st["generated"].values()))
        seed_bytes = sum(t.numel() * t.element_size() for t in [whole["image"], whole["spheres"], whole["chunks"], whole["demo"], s_sph]
                         + list(whole["generated"].values()) + list(s_act.values()))
        res["seeds_extra_copy_bytes"] = int(seed_bytes - plain_bytes)
        launches["seed_spheres_us"] = lambda: E.openloop_seed_spheres(whole["spheres"], s_sph, min_ratio=ev_seeds.seed_min_ratio)
        launches["seed_actions_us"] = lambda: E.openloop_seed_actions(whole["chunks"], whole["demo"], s_act["rad"], joint_scale=ev_seeds.joint_std)
        if args.combine is not None:  # the launches OpenLoopEval(combine=...) adds per execution setting and rule (two score launches follow each)
            c_out = torch.empty((ev_seeds.N, ev_seeds.A), dtype=torch.float32, device=E.device)
            c_pick = torch.empty((ev_seeds.N,), dtype=torch.int32, device=E.device)
            c_first = torch.zeros((ev_seeds.N,), dtype=torch.int32, device=E.device)  # one long episode: the most calls per step
            res["combine"] = [r.strip() for r in args.combine.split(",")]
            for rule in res["combine"]:
                launches[f"exec_actions_samples_{rule}_us"] = lambda rule=rule: E.openloop_exec_actions_samples(whole["chunks"], c_first, 5, True, combine=rule,
                                                                                                                out=c_out, pick=c_pick)
    if args.perturb is not None:
        from genima_amd import perturb as PB

        setting = PB.parse(args.perturb)
        ev_p = OpenLoopEval(dagent, controller, eps, cams, render_cfg=rcfg, stats=(P.action_stats(demos), P.proprio_stats(demos)), tokenizer=tokens,
                            batch_size=B, engine=E, perturb=setting, perturb_seed=0)
        ptabs = ev_p._tables()
        runs = {"batch_clean": lambda: ev.run_batch(0, tabs, gen), "batch_perturbed": lambda: ev_p.run_batch(0, ptabs, gen)}
        rms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():
                E.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    rms[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            res[k] = stats(rms[k])
        res["perturb"] = {"setting": setting.describe(), "seed": 0, "alternations": args.reps, "draws": PB.draw_ranges(ev_p.perturb_draws)}
        res["perturbed_minus_clean_ms"] = round(res["batch_perturbed"]["median_ms"] - res["batch_clean"]["median_ms"], 4)
        res["batch_clean_spread_ms"] = round(res["batch_clean"]["max_ms"] - res["batch_clean"]["min_ms"], 4)
        p_M = ev_p.perturb_M.index_select(0, sel).reshape(B * ev.V, 9)
        p_col = ev_p.perturb_colour.index_select(0, sel).reshape(B * ev.V, 6)
        p_out, p_cnt = torch.empty_like(frames), torch.empty((B * ev.V,), dtype=torch.int32, device=E.device)
        launches["view_perturb_us"] = lambda: E.view_perturb(frames, p_M, p_col, out=p_out, n_revealed=p_cnt)  # frames: the CLEAN evaluator's batch
        res["view_perturb_bytes"] = {"views": B * ev.V, "read_source": int(frames.numel()), "written": int(p_out.numel() + 4 * p_cnt.numel()),
                                     "tables": int(8 * (p_M.numel() + p_col.numel()))}
    for name, launch in launches.items():
        us = []
        for _ in range(5):
            for _ in range(10):
                launch()
            s, e = E.event(), E.event()
            E.event_record(s)
            for _ in range(100):
                launch()
            E.event_record(e)
            E.synchronize()
            us.append(E.event_elapsed_ms(s, e) / 100 * 1e3)
        res[name] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    wh = ev.windows_host[idx]
    res["sphere_windows"] = {"n": int(wh[..., 0].size), "non_empty": int(((wh[..., 2] > wh[..., 0]) & (wh[..., 3] > wh[..., 1])).sum()),
                             "pixels": int(((wh[..., 2] - wh[..., 0]) * (wh[..., 3] - wh[..., 1])).sum()), "change_threshold": ev.change_threshold}
    if args.perturb is not None:
        res["view_perturb_revealed_share"] = round(float(p_cnt.double().mean().item()) / (S * S), 5)
        res["view_perturb_gb_per_s"] = round((res["view_perturb_bytes"]["read_source"] + res["view_perturb_bytes"]["written"]) / (res["view_perturb_us"]["median"] * 1e-6) / 1e9, 2)
    res["image_metrics_bytes"] = int(out_img.numel() + batch["full"].numel() + batch["occupied"].numel())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
