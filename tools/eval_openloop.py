"""Score a diffusion checkpoint and a controller snapshot on held-out demos, open loop (``genima_amd.openloop.OpenLoopEval``): for every
transition of the demo tree, diffusion then the controller as the eval loop's body runs them, the generated target against the rendered
ground truth, the predicted action chunk against the demo's, and the controller again on the ground-truth target (the oracle row).

    python tools/eval_openloop.py --dataset_root /data/rlbench_data_val --tasks take_lid_off_saucepan --demos 5 \
        --sd_ckpt ./sd-turbo --diffusion_ckpt ./controlnet_out --controller_snapshot ./exp_local/snapshots/genima_controller/best.pt \
        --stats_dir ./exp_local/snapshots/genima_controller --clip_text ./clip-vit-base-patch32 --sphere_textures ./sphere_textures \
        --out openloop.json

Reads ``<dataset_root>/<task>/variation0/episodes/<episode>/{<camera>_rgb/<ts>.png, demo.npz, traj.npz[, description.txt]}`` (the camera frames
are the SCENE frames the diffusion agent sees at run time; ``tools/render_dataset.py`` writes ``traj.npz``, ``genima_amd.replay.save_demo``
``demo.npz``).  ``--stats_dir`` holds the TRAINING run's ``action_stats.json`` / ``proprio_stats.json``: the held-out demos are normalised with
those, never with their own.  Prints the summary and writes it as JSON; with a diffusion agent it carries ``image.spheres``, the per-sphere
location / mass / spread / colour scores (``--change_threshold`` sets their threshold against the observation).  ``--no_controller`` scores the
diffusion checkpoint alone (no ``--controller_snapshot`` / ``--stats_dir`` needed: the mode a ControlNet fine-tune validates in).
``--execution H[,agg[,M]]`` (repeatable; ``5``, ``5,agg``, ``5,agg,0.01``) also replays that execution mode over the run's chunks and adds, under
``executions``, the error and the step-to-step jump of the EXECUTED actions (``OpenLoopResult.execution_summary``).
``--triangulate`` also triangulates every drawn sphere across the four views (``gn_openloop_triangulate``) and adds, under ``spheres_3d``,
the 3D error in millimetres and the cross-view residuals of the generated image beside those of the ground-truth render, the floor of the
method (``OpenLoopResult.triangulation_summary``; ``--tri_min_ratio`` / ``--tri_min_det`` set which views and which crossings count).
``--orientation K[,span]`` (``37``, ``25,60``) also reads the orientation the generated spheres show: every true sphere is re-drawn at K
rotations about its own z axis over ``span`` degrees (default 180) and compared with the generated window (``gn_openloop_orientation``); under
``orientation`` the summary then carries the angular error, its contrast and ``floor_deg``, the same read-out of the ground-truth render,
which is 0 (``OpenLoopResult.orientation_summary``).
``--seeds R`` (2 .. 64) repeats the generation with the generator seeds ``--seed``, ``--seed`` + 1, ... and adds, under ``seeds``, every score
per seed with its mean and seed-to-seed standard deviation -- the noise floor a difference between two checkpoints has to beat --, per sphere
the bias of the seeds' mean centroid beside their spread about it (``variance_share``: 0 all bias, 1 all noise) and, with a controller, the
error of the seed-averaged chunk beside the mean of the seeds' errors (``gain``; ``OpenLoopResult.seed_summary``).  Everything outside that
block stays the first seed's, as without the option; the run costs R generations per transition.  A seed spread is not a success rate either,
and ``gain`` is teacher-forced: it measures an averaged chunk that only ``--combine`` below replays.
``--combine mean,medoid`` (with ``--seeds`` and ``--execution``) adds, per execution setting, the row kinds ``seed_mean`` / ``seed_medoid`` beside
``generated`` (seed 0): the same scores of what the mode executes when the R seeds' chunks of every call are combined first, as
``GenimaACT.set_execution(samples=R, combine=...)`` does in the control loop; the medoid's rows also carry ``pick_histogram`` and
``pick_is_seed0_rate``.  Still teacher-forced and no success rate; averaging across modes is the known failure the medoid exists for.
``--perturb SPEC`` (repeatable; a preset ``camera_pose`` / ``light_color``, a spec such as ``camera:pitch=-0.05..0.05,zoom=0.95..1.05`` or
``light:r=0.5..1,g=0.5..1,b=0.5..1``, two joined by ``+``; ``genima_amd.perturb.parse``) also runs ``openloop.robustness_sweep`` after the clean
run -- the same evaluator under each setting, drawn per episode with ``--perturb_seed`` -- and writes it beside the result as
``<out>.robustness.json``: per setting the scores, their change against clean (with ``--seeds`` also over the clean seed-to-seed standard
deviation), the share of revealed border and the spheres that left the view.  The camera rotation and intrinsics are exact, the light is a
per-channel gain (a stand-in), a camera translation is left out; revealed borders are mirrored scene, and a score under a perturbation is
still not a success rate.  The result file itself stays the clean run's.
Open-loop error is not a success rate: every chunk is predicted from a demo state, nothing is executed and no error compounds."""
import argparse
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import replay as P  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset_root", required=True)
    ap.add_argument("--tasks", nargs="+", default=["take_lid_off_saucepan"])
    ap.add_argument("--demos", type=int, default=5)
    ap.add_argument("--sd_ckpt", required=True, help="diffusers directory of the base model, or synthetic:<family>")
    ap.add_argument("--diffusion_ckpt", default="", help="the fine-tune's output directory (checkpoint-N/controlnet) or a ControlNet directory")
    ap.add_argument("--agent", default="SDControlNetAgent", choices=["SDControlNetAgent", "SDXLControlNetAgent", "SDPix2PixAgent"])
    ap.add_argument("--autoencoder", default="")
    ap.add_argument("--controller_snapshot", default=None, help="latest.pt / best.pt / <epoch>.pt of tools/train_act.py")
    ap.add_argument("--stats_dir", default=None, help="directory of the training run's action_stats.json and proprio_stats.json")
    ap.add_argument("--no_controller", action="store_true", help="diffusion-only mode: image and sphere scores, no action tables")
    ap.add_argument("--change_threshold", type=int, default=30, help="gn_openloop_sphere_metrics' threshold on the summed channel difference against the observation")
    ap.add_argument("--clip_text", default=None, help="transformers CLIPTextModel directory (weights and tokenizer) of the controller")
    ap.add_argument("--cameras", nargs="+", default=list(P.DEFAULT_CAMERAS))
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--action_sequence", type=int, default=20)
    ap.add_argument("--action_horizon", type=int, default=20, help="render.yaml's horizon of the drawn joint target")
    ap.add_argument("--sphere_textures", default="./sphere_textures/")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_inference_steps", type=int, default=5)
    ap.add_argument("--guidance_scale", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--execution", action="append", default=None, metavar="H[,agg[,M]]",
                    help="also score the actions an execution mode would execute: horizon H, 'agg' for temporal_agg, weight decay M (default 0.01); repeatable")
    ap.add_argument("--triangulate", action="store_true", help="also triangulate the drawn spheres across the views: the 3D error in mm and the cross-view residuals")
    ap.add_argument("--tri_min_ratio", type=float, default=0.5, help="a view counts for the generated image when its mass is at least this share of the ground truth's")
    ap.add_argument("--tri_min_det", type=float, default=1e-6, help="rays that cross worse than this (det(A) / (trace(A) / 3)^3) are left unsolved")
    ap.add_argument("--orientation", default=None, metavar="K[,span]",
                    help="also read the orientation the generated spheres show: K (odd, at most 64) candidate rotations over span degrees (default 180)")
    ap.add_argument("--seeds", type=int, default=None, metavar="R",
                    help="also repeat the generation with R (2 .. 64) generator seeds, --seed .. --seed + R - 1: per-score seed spread, per-sphere bias and spread")
    ap.add_argument("--combine", default=None, metavar="RULE[,RULE]",
                    help="with --seeds and --execution: also score what each mode executes when the seeds' chunks are combined first, by 'mean', 'medoid' or both")
    ap.add_argument("--seed_min_ratio", type=float, default=0.5, help="with --seeds: a seed found a sphere when its mass is at least this share of the ground truth's")
    ap.add_argument("--perturb", action="append", default=None, metavar="SPEC",
                    help="also score under this camera-pose / light perturbation (a preset, a spec, or two joined by '+'); repeatable; written to <out>.robustness.json")
    ap.add_argument("--perturb_seed", type=int, default=0, help="with --perturb: the seed of the per-episode draws")
    ap.add_argument("--out", default="openloop.json")
    a = ap.parse_args(argv)
    if not a.no_controller and not (a.controller_snapshot and a.stats_dir):
        ap.error("--controller_snapshot and --stats_dir are required unless --no_controller is given")
    if a.execution is not None:
        from genima_amd.openloop import parse_execution

        if a.no_controller:
            ap.error("--execution replays the controller's chunks: it cannot be combined with --no_controller")
        try:
            a.execution = [parse_execution(e) for e in a.execution]
        except ValueError as err:
            ap.error(str(err))
    if a.seeds is not None and not 2 <= a.seeds <= 64:
        ap.error(f"--seeds {a.seeds}: the number of generator seeds must lie in [2, 64]")
    if a.combine is not None:
        a.combine = tuple(r.strip() for r in a.combine.split(","))
        if a.seeds is None or a.execution is None:
            ap.error("--combine scores the combined chunk of the seeds under an execution mode: it needs --seeds and --execution")
        if not a.combine or len(set(a.combine)) != len(a.combine) or any(r not in ("mean", "medoid") for r in a.combine):
            ap.error(f"--combine {','.join(a.combine)}: distinct rules out of mean, medoid expected")
    if a.perturb is not None:
        from genima_amd import perturb as PB

        try:
            a.perturb = [PB.parse(t) for t in a.perturb]
        except ValueError as err:
            ap.error(str(err))
    if a.orientation is not None:
        from genima_amd.openloop import orientation_candidates, parse_orientation

        try:
            a.orientation = parse_orientation(a.orientation)
            orientation_candidates(**a.orientation)
        except ValueError as err:
            ap.error(str(err))
    return a


def main(argv=None):
    a = parse(argv)
    from genima_amd import agent as A
    from genima_amd import configs, harness
    from genima_amd import render as R
    from genima_amd.act import GenimaACT
    from genima_amd.openloop import OpenLoopEval, robustness_sweep

    episodes = P.list_episodes(a.dataset_root, a.tasks, a.demos)
    if not episodes:
        raise SystemExit(f"eval_openloop: no episodes under {a.dataset_root} for tasks {a.tasks}")
    rcfg = R.RenderConfig(image_width=a.image_size, image_height=a.image_size, action_horizon=a.action_horizon, texture_dir=a.sphere_textures)
    for ep in episodes:
        if not os.path.exists(os.path.join(ep, "demo.npz")):
            P.save_demo(os.path.join(ep, "demo.npz"), P.demo_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl")))
        if not os.path.exists(os.path.join(ep, "traj.npz")):
            R.save_traj(os.path.join(ep, "traj.npz"), R.traj_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl"), rcfg.cameras))
    clip_sd = tokenizer = None
    if a.clip_text:
        from genima_amd import weights
        from genima_amd.tokenizer import CLIPTokenizer

        _, clip_sd = weights.load_diffusers_dir(a.clip_text)
        tokenizer = CLIPTokenizer.from_pretrained(a.clip_text)
    ns = types.SimpleNamespace(diffusion_ckpt=a.diffusion_ckpt, sd_ckpt=a.sd_ckpt, device="cuda", image_resolution=2 * a.image_size, vae_slicing=False,
                               upcast_vae=False, fused_projections=True, enable_xformers_memory_efficient_attention=True,
                               show_diffusion_progress=False, torch_compile=False, autoencoder=a.autoencoder)
    dagent = getattr(A, a.agent)(ns)
    controller = stats = None
    if not a.no_controller:
        cfg = dict(configs.ACT_POLICY, num_queries=a.action_sequence, num_views=len(a.cameras), image_size=a.image_size, use_lang_cond=tokenizer is not None)
        controller = GenimaACT(cfg, None, configs.ACT_CLIP_TEXT, clip_sd, device="cuda", seed=a.seed)
        harness.load_controller_ckpt(controller, a.controller_snapshot)
        stats = P.load_stats(a.stats_dir)
    ev = OpenLoopEval(dagent, controller, episodes, a.cameras, render_cfg=rcfg, stats=stats, tokenizer=tokenizer, batch_size=a.batch_size,
                      num_inference_steps=a.num_inference_steps, guidance_scale=a.guidance_scale, seed=a.seed, change_threshold=a.change_threshold,
                      action_sequence=a.action_sequence, executions=a.execution, triangulate=a.triangulate, tri_min_ratio=a.tri_min_ratio,
                      tri_min_det=a.tri_min_det, orientation=a.orientation, seeds=a.seeds, seed_min_ratio=a.seed_min_ratio, combine=a.combine)
    print(f"eval_openloop: {len(episodes)} episodes, {ev.N} transitions, {ev.replay.device_bytes / 1e6:.0f} MB of frames on the device", flush=True)
    summary = ev.run().to_json(a.out)
    print(json.dumps(summary, indent=1))
    if a.perturb is not None:
        sweep = robustness_sweep(ev, a.perturb, seed=a.perturb_seed)
        path = os.path.splitext(a.out)[0] + ".robustness.json"
        with open(path, "w") as f:
            json.dump(sweep, f, indent=1)
        print(json.dumps(sweep, indent=1))
        print(f"eval_openloop: robustness sweep written to {path}", flush=True)


if __name__ == "__main__":
    main()
