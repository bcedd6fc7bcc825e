"""Draw the joint-action spheres into a recorded dataset on the device: the command line over ``genima_amd.render.render_episode``, with
the argument names and default values of the reference's ``render/cfgs/render.yaml``.

    python tools/render_dataset.py --dataset_root /data/rlbench --task take_lid_off_saucepan --episodes 25 \
        --sphere_textures ./sphere_textures --textures_path ./textures

Reads ``<dataset_root>/<task>/variation<k>/episodes/episode<i>/{<camera>_rgb/<ts>.png, traj.npz | low_dim_obs.pkl}`` and writes
``<save_path or dataset_root's parent>/<name>_rgb_rendered/...`` (and ``<name>_rnd_bg/...`` with ``--draw.rnd_bg`` and textures), as the
reference does.  ``traj.npz`` is the plain-array trajectory of genima_amd/render.py; an episode that has only RLBench's
``low_dim_obs.pkl`` is converted first, which needs ``rlbench`` importable for the unpickling."""
import argparse
import json
import os
import shutil
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genima_amd import render as R  # noqa: E402

_flag = lambda s: s.lower() in ("1", "true", "yes")  # noqa: E731


def parse(argv=None):
    d = R.RenderConfig()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset_root", default="/tmp/")
    ap.add_argument("--save_path", default=None)
    ap.add_argument("--textures_path", default="./textures")
    ap.add_argument("--sphere_textures", default=d.texture_dir, help="directory of the five sphere_<colour>_stripe_texture.png files")
    ap.add_argument("--cameras", nargs="+", default=list(d.cameras))
    ap.add_argument("--camera_scales", nargs="+", type=float, default=list(d.camera_scales))
    ap.add_argument("--task", default="take_lid_off_saucepan")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--episode_offset", type=int, default=0)
    ap.add_argument("--variation", type=int, default=0)
    ap.add_argument("--image_width", type=int, default=d.image_width)
    ap.add_argument("--image_height", type=int, default=d.image_height)
    ap.add_argument("--znear", type=float, default=d.znear)
    ap.add_argument("--zfar", type=float, default=d.zfar)
    ap.add_argument("--action_horizon", type=int, default=d.action_horizon)
    ap.add_argument("--alpha_blend", type=float, default=d.alpha_blend)
    ap.add_argument("--render.sphere.radius", dest="sphere_radius", type=float, default=d.sphere_radius)
    ap.add_argument("--render.joints", dest="joints", type=json.loads, default=dict(d.joints), help='JSON, e.g. {"wrist": [1, 3, 5], "overhead": []}')
    ap.add_argument("--draw.rgb_rendered", dest="draw_rgb_rendered", type=_flag, default=True)
    ap.add_argument("--draw.rnd_bg", dest="draw_rnd_bg", type=_flag, default=True)
    ap.add_argument("--samples", type=int, default=d.samples, choices=(1, 4))
    return ap.parse_args(argv)


def config(a) -> R.RenderConfig:
    return R.RenderConfig(cameras=a.cameras, camera_scales=a.camera_scales, image_width=a.image_width, image_height=a.image_height, znear=a.znear,
                          zfar=a.zfar, action_horizon=a.action_horizon, alpha_blend=a.alpha_blend, sphere_radius=a.sphere_radius, joints=a.joints,
                          textures_path=a.textures_path if a.draw_rnd_bg else None, draw_rgb_rendered=a.draw_rgb_rendered,
                          draw_rnd_bg=a.draw_rnd_bg, texture_dir=a.sphere_textures, samples=a.samples)


def main(argv=None):
    from PIL import Image

    a = parse(argv)
    cfg = config(a)
    root = os.path.abspath(a.dataset_root).rstrip("/")
    parent = a.save_path if a.save_path is not None else os.path.dirname(root)
    name = os.path.basename(root)
    var = f"variation{a.variation}" if a.variation != -1 else "all_variations"
    skip = lambda d, names: [n for n in names if "depth" in n or "mask" in n]  # noqa: E731  (render_data.py:389-392)
    full_root, rnd_root = os.path.join(parent, name + "_rgb_rendered"), os.path.join(parent, name + "_rnd_bg")
    for dst in [full_root] + ([rnd_root] if cfg.draw_rnd_bg else []):
        shutil.copytree(os.path.join(root, a.task), os.path.join(dst, a.task), dirs_exist_ok=True, ignore=skip)
    for e in range(a.episode_offset, a.episodes):
        rel = os.path.join(a.task, var, "episodes", f"episode{e}")
        src = os.path.join(root, rel)
        if os.path.exists(os.path.join(src, "traj.npz")):
            traj = R.load_traj(os.path.join(src, "traj.npz"))
        else:
            traj = R.traj_from_low_dim_obs(os.path.join(src, "low_dim_obs.pkl"), cfg.cameras)
        L = len(traj["gripper_open"])
        frames = {c: np.stack([np.asarray(Image.open(os.path.join(src, f"{c}_rgb", f"{i}.png")).convert("RGB")) for i in range(L)]) for c in cfg.cameras}
        R.render_episode(traj, frames, os.path.join(full_root, rel), cfg, rnd_out_dir=os.path.join(rnd_root, rel) if cfg.draw_rnd_bg else None)
        print(f"episode{e}: {L - 1} steps x {len(cfg.cameras)} cameras", flush=True)


if __name__ == "__main__":
    main()
