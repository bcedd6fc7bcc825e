"""Train the ACT controller from a demo tree: the command line over ``genima_amd.act_train_loop.ControllerTrainLoop``, with the argument
names of the reference's step 4 (``python train_act.py ... demos=25 action_sequence=20 batch_size=8 num_train_epochs=1000``).

    python tools/train_act.py --dataset_root /data/rlbench_data_rnd_bg --tasks take_lid_off_saucepan --demos 25 --work_dir ./exp_local \
        --clip_text ./clip-vit-base-patch32

Reads ``<dataset_root>/<task>/variation0/episodes/<episode>/{<camera>_rgb/<ts>.png, demo.npz[, description.txt]}`` (a tree
``tools/render_dataset.py`` writes, plus one ``demo.npz`` per episode: ``genima_amd.replay.save_demo``; an episode that has only RLBench's
``low_dim_obs.pkl`` is converted first, which needs ``rlbench`` importable for the unpickling).  The controller learns from the
RANDOM-BACKGROUND tree (the reference's ``rlbench_data_rnd_bg``: spheres blended over a random texture, no scene), not from
``rgb_rendered``, which is the diffusion agent's.

With ``--rnd_bg_textures DIR`` no PNG tree is needed at all: every batch is drawn on the device from ``<episode>/traj.npz`` (which
``tools/render_dataset.py`` writes beside the frames; an episode with only ``low_dim_obs.pkl`` is converted too) over a texture of ``DIR``, a
fresh texture and blend factor for every frame of every batch:

    python tools/train_act.py --dataset_root /data/rlbench_data --rnd_bg_textures ./textures --sphere_textures ./sphere_textures ...

With ``--val_root DIR`` (a second tree of the same layout whose episodes hold the scene frames, ``demo.npz`` and ``traj.npz``) every snapshot
is scored on the first ``--val_demos`` held-out demos of each task -- the controller alone on the rendered ground-truth targets
(``genima_amd.openloop.controller_validator``) -- into ``validation.jsonl``, and the snapshot with the lowest normalised joint L1 is kept as
``best.pt``.  ``--val_execution H[,agg[,M]]`` ranks by the joint L1 of the actions executed under that execution mode instead.

Writes
``<work_dir>/snapshots/<experiment_name>/{latest.pt, <epoch>.pt, action_stats.json, proprio_stats.json}``.  Nothing from RoboBase or RLBench is
imported otherwise.  ``--clip_text``: a transformers ``CLIPTextModel`` directory (weights + tokenizer files) for the task-string
conditioning; without it the text tower keeps its random initialisation, which only makes sense for a dry run."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import replay as P  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset_root", required=True)
    ap.add_argument("--tasks", nargs="+", default=["take_lid_off_saucepan"])
    ap.add_argument("--demos", type=int, default=25)
    ap.add_argument("--work_dir", default="./exp_local")
    ap.add_argument("--experiment_name", default="genima_controller")
    ap.add_argument("--num_train_epochs", type=int, default=1000)
    ap.add_argument("--checkpoint_every", type=int, default=10)
    ap.add_argument("--num_checkpoints", type=int, default=3)
    ap.add_argument("--action_sequence", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--lr_backbone", type=float, default=1e-5)
    ap.add_argument("--actor_grad_clip", type=float, default=None)
    ap.add_argument("--cameras", nargs="+", default=list(P.DEFAULT_CAMERAS))
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--clip_text", default=None, help="transformers CLIPTextModel directory (weights and tokenizer)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_every", type=int, default=50)
    ap.add_argument("--rnd_bg_textures", default=None, help="directory of background textures: draw the random-background frames on the device "
                                                              "from <episode>/traj.npz instead of reading a PNG tree")
    ap.add_argument("--sphere_textures", default="./sphere_textures/", help="directory of the five sphere_<colour>_stripe_texture.png files")
    ap.add_argument("--alpha_blend", type=float, default=0.7, help="lower end of the sphere / texture blend factor (render.yaml: 0.7)")
    ap.add_argument("--render_seed", type=int, default=0, help="seed of the background draws")
    ap.add_argument("--val_root", default=None, help="held-out demo tree: score every snapshot on it (validation.jsonl) and keep the best as best.pt")
    ap.add_argument("--val_demos", type=int, default=5, help="held-out demos per task")
    ap.add_argument("--val_action_horizon", type=int, default=20, help="render.yaml's horizon of the joint targets drawn for validation")
    ap.add_argument("--val_execution", default=None, metavar="H[,agg[,M]]",
                    help="rank snapshots by the joint L1 of the actions EXECUTED under this mode (horizon H, 'agg' for temporal_agg, weight decay M) instead of whole chunks")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse(argv)
    import torch

    from genima_amd import configs
    from genima_amd.act import GenimaACT
    from genima_amd.act_train_loop import ControllerTrainLoop

    episodes = P.list_episodes(a.dataset_root, a.tasks, a.demos)
    if not episodes:
        raise SystemExit(f"train_act: no episodes under {a.dataset_root} for tasks {a.tasks}")
    for ep in episodes:
        if not os.path.exists(os.path.join(ep, "demo.npz")):
            P.save_demo(os.path.join(ep, "demo.npz"), P.demo_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl")))
    render = None
    if a.rnd_bg_textures:
        from genima_amd import render as R

        rcfg = R.RenderConfig(image_width=a.image_size, image_height=a.image_size, alpha_blend=a.alpha_blend,
                              texture_dir=a.sphere_textures)
        for ep in episodes:
            if not os.path.exists(os.path.join(ep, "traj.npz")):
                R.save_traj(os.path.join(ep, "traj.npz"), R.traj_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl"), rcfg.cameras))
        render = P.RenderTargets(rcfg, a.rnd_bg_textures, seed=a.render_seed, alpha_blend=a.alpha_blend)
    clip_sd = tokenizer = None
    if a.clip_text:
        from genima_amd import weights
        from genima_amd.tokenizer import CLIPTokenizer

        _, clip_sd = weights.load_diffusers_dir(a.clip_text)
        tokenizer = CLIPTokenizer.from_pretrained(a.clip_text)
    cfg = dict(configs.ACT_POLICY, num_queries=a.action_sequence, num_views=len(a.cameras), image_size=a.image_size, data_augmentation=True,
               use_lang_cond=tokenizer is not None, lr=a.lr, lr_backbone=a.lr_backbone, actor_grad_clip=a.actor_grad_clip)
    torch.manual_seed(a.seed)
    agent = GenimaACT(cfg, None, configs.ACT_CLIP_TEXT, clip_sd, device="cuda", seed=a.seed)
    replay = P.DeviceReplay(episodes, a.cameras, device="cuda", action_sequence=a.action_sequence, batch_size=a.batch_size, tokenizer=tokenizer,
                            image_size=a.image_size, render=render)
    what = "view tables, textures and sphere atlas" if render is not None else "frames"
    print(f"train_act: {len(episodes)} episodes, {replay.N} transitions, {replay.device_bytes / 1e6:.0f} MB of {what} on the device", flush=True)

    def log(metrics, it):
        if it % a.log_every == 0:
            print(f"iter {it}: " + " ".join(f"{k}={v:.5f}" for k, v in metrics.items()), flush=True)

    validate = None
    if a.val_root:
        from genima_amd import render as R
        from genima_amd.openloop import controller_validator, parse_execution

        execution = parse_execution(a.val_execution) if a.val_execution else None
        vcfg = R.RenderConfig(image_width=a.image_size, image_height=a.image_size, action_horizon=a.val_action_horizon, texture_dir=a.sphere_textures)
        val_eps = P.list_episodes(a.val_root, a.tasks, a.val_demos)
        for ep in val_eps:
            if not os.path.exists(os.path.join(ep, "demo.npz")):
                P.save_demo(os.path.join(ep, "demo.npz"), P.demo_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl")))
            if not os.path.exists(os.path.join(ep, "traj.npz")):
                R.save_traj(os.path.join(ep, "traj.npz"), R.traj_from_low_dim_obs(os.path.join(ep, "low_dim_obs.pkl"), vcfg.cameras))
        validate = controller_validator(val_eps, a.cameras, render_cfg=vcfg, stats=(replay.action_stats, replay.proprio_stats), tokenizer=tokenizer,
                                        batch_size=a.batch_size, engine=replay.E, execution=execution)
    ControllerTrainLoop(agent, replay, a.work_dir, a.experiment_name, a.num_train_epochs, a.checkpoint_every, a.num_checkpoints, log=log,
                        cfg={k: v for k, v in vars(a).items()}, validate=validate).train()


if __name__ == "__main__":
    main()
