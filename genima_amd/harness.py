"""Simulator-free restatement of ONE control step of the reference's evaluation loop (controller/eval_genima.py:162-248), the
counterpart of BASELINE.json configs[0] (SURVEY.md section 8a row a1 / 8d "Config 1"): observation dict -> PIL views -> prompt ->
2x2 tiling -> ``diffusion_agent.infer`` -> untile -> observation overwrite -> ``controller_agent.act`` -> actions.

RLBench / CoppeliaSim / Hydra stay out of scope; what this module pins is the data contract between the simulator loop and the two
plugins, so the agents of this package can be exercised (and the reference's loop body checked against them) without a simulator:
  * views are gathered camera-major, frame-minor (``rgbs[cam * num_frames + t]``, :167-173) and tiled per frame;
  * one prompt per frame, ``f"tiled perspectives of a robot arm executing '{goal}'"`` (:178);
  * the SAME generator object is passed once per tiled image (``generator * len(tiled_images)``, :130-135, :209);
  * the pipeline output is indexed ``[0]`` for the list of images (:215, :225) and untiled with the agent's
    ``transform_to_half_resolution`` (:226-230);
  * the four camera keys ``wrist / front / right_shoulder / left_shoulder`` are overwritten by name (:231-234), every observation
    entry gets a leading batch axis on the device (:237-240), and ``act(...)[0]`` is the ``[queries, action_dim]`` plan (:243-248).
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from .tiling import tile_images, untile_images

NEGATIVE_PROMPT = "monochrome, lowres, bad anatomy, worst quality, low quality"
OVERWRITTEN_CAMERAS = ("wrist", "front", "right_shoulder", "left_shoulder")


def make_prompt(goal: str) -> str:
    return f"tiled perspectives of a robot arm executing '{goal}'"


def control_step(diffusion_agent, controller_agent, obs: Dict[str, np.ndarray], goal: str, cameras: Sequence[str], num_frames: int,
                 generator: List[torch.Generator], num_diffusion_steps: int, guidance_scale: float, device, episode_step: int = 0,
                 execution_horizon=None, temporal_agg: bool = False, samples=None, combine: str = "mean"):
    """obs: ``{'<cam>_rgb': uint8 [fs, 3, 256, 256], 'low_dim_state': f32 [fs, S], 'lang_tokens': int [fs, 1|.., 77], ...}`` as the
    RoboBase env wrapper hands it over.  Returns ``(actions np.float32 [queries, action_dim], obs_after, tiled_in, tiled_out)``;
    ``obs_after`` holds the device tensors the controller saw (camera images replaced by the generated joint-target views).
    ``execution_horizon`` / ``temporal_agg`` (controller/cfgs/eval_genima.yaml:29,33 -- knobs the reference's loop never reads): the
    controller returns the ``h = execution_horizon`` actions of the environment steps ``episode_step .. episode_step + h - 1``, ensembled over
    the overlapping chunks of the earlier calls with ``temporal_agg`` (GenimaACT.set_execution); ``actions`` is then ``[h, action_dim]``, the loop
    executes all of them and calls again with ``episode_step + h``.  ``episode_step == 0`` starts a new history.  The arguments are
    passed on with ``set_execution`` where the controller's mode (``GenimaACT.execution``) differs from them.  With neither argument given the
    controller is not touched: it returns what its own mode says (by default the whole chunk, as before).

    ``samples=R`` / ``combine`` (``GenimaACT.set_execution``): the observation is generated R times in ONE diffusion call -- the tiled image and the
    prompts repeated R times, the caller's one generator passed once per image as above, so the R noise draws come one after the other from
    its stream and R = 1 draws what a call without ``samples`` draws -- the controller sees the R generated observations as R rows, combines their
    R chunks on the device (``"mean"`` or ``"medoid"``) and executes the combined one under the execution mode.  ``tiled_out`` then holds all R
    generated images, ``obs_after`` the R rows; ``actions`` stays one plan, ``[h, action_dim]`` (h = queries with no horizon given).  Needs one
    frame per call.  With ``samples=None`` the function does what it did before."""
    from PIL import Image

    if samples is None:
        if combine != "mean":
            raise ValueError(f"control_step: combine={combine!r} needs samples=R")
        return _control_step_one(diffusion_agent, controller_agent, obs, goal, cameras, num_frames, generator, num_diffusion_steps, guidance_scale, device,
                                 episode_step, execution_horizon, temporal_agg)
    from .act import check_samples, execution_slots

    R, combine = check_samples(samples, combine)
    if num_frames != 1:
        raise ValueError(f"control_step: samples={R} takes one frame per call (the controller's rows are the samples), got num_frames={num_frames}")
    rgbs = [Image.fromarray(np.transpose(obs[f"{cam}_rgb"][0], (1, 2, 0))) for cam in cameras]
    tiled_in = tile_images(rgbs, 1)
    with torch.inference_mode():
        out = diffusion_agent.infer(images=tiled_in * R, prompts=[make_prompt(goal)] * R, negative_prompts=[NEGATIVE_PROMPT] * R,
                                    num_inference_steps=num_diffusion_steps, guidance_scale=guidance_scale, generator=generator * R)
        tiled_out = out[0]
        untiled = untile_images(tiled_out, cameras, diffusion_agent.transform_to_half_resolution)  # every camera: [R, 3, H, W]
        obs_dev = {}
        for k, v in obs.items():
            cam = k[: -len("_rgb")] if k.endswith("_rgb") else None
            if cam in OVERWRITTEN_CAMERAS:
                obs_dev[k] = torch.from_numpy(np.asarray(untiled[cam])).to(device).unsqueeze(1)  # [R, fs = 1, 3, H, W]
            else:
                t = torch.from_numpy(np.asarray(v)).to(device).unsqueeze(0)
                obs_dev[k] = t.expand(R, *t.shape[1:]).contiguous()
        mode = execution_slots(int(controller_agent.config["num_queries"]), execution_horizon, temporal_agg)
        if controller_agent.execution is None or controller_agent.execution[:2] != mode or controller_agent.execution_samples != (R, combine):
            controller_agent.set_execution(execution_horizon, temporal_agg, samples=R, combine=combine)  # (starts with an empty history)
        elif episode_step == 0:
            controller_agent.reset_execution()
        actions = controller_agent.act(obs_dev, step=episode_step, eval_mode=True)[0]
    return actions.detach().float().cpu().numpy(), obs_dev, tiled_in, tiled_out


def _control_step_one(diffusion_agent, controller_agent, obs, goal, cameras, num_frames, generator, num_diffusion_steps, guidance_scale, device, episode_step,
                      execution_horizon, temporal_agg):
    """``control_step`` without samples: one generation per frame, one controller row."""
    from PIL import Image

    rgbs = [Image.fromarray(np.transpose(obs[f"{cam}_rgb"][t], (1, 2, 0))) for cam in cameras for t in range(num_frames)]
    prompts = [make_prompt(goal)] * num_frames
    negative = [NEGATIVE_PROMPT] * num_frames
    tiled_in = tile_images(rgbs, num_frames)
    with torch.inference_mode():
        out = diffusion_agent.infer(images=tiled_in, prompts=prompts, negative_prompts=negative,
                                    num_inference_steps=num_diffusion_steps, guidance_scale=guidance_scale,
                                    generator=generator * len(tiled_in))
        tiled_out = out[0]
        untiled = untile_images(tiled_out, cameras, diffusion_agent.transform_to_half_resolution)
        obs = dict(obs)
        for cam in OVERWRITTEN_CAMERAS:
            obs[f"{cam}_rgb"] = untiled[cam]
        obs_dev = {k: torch.from_numpy(np.asarray(v)).to(device).unsqueeze(0) for k, v in obs.items()}
        if execution_horizon is not None or temporal_agg:
            from .act import execution_slots

            if (controller_agent.execution is None or getattr(controller_agent, "execution_samples", None) is not None
                    or controller_agent.execution[:2] != execution_slots(int(controller_agent.config["num_queries"]), execution_horizon, temporal_agg)):
                controller_agent.set_execution(execution_horizon, temporal_agg)  # (starts with an empty history)
            elif episode_step == 0:
                controller_agent.reset_execution()
        actions = controller_agent.act(obs_dev, step=episode_step, eval_mode=True)[0]
    return actions.detach().float().cpu().numpy(), obs_dev, tiled_in, tiled_out


def load_controller_ckpt(controller_agent, checkpoint_path, device="cpu"):
    """``Workspace.load_controller_ckpt`` (controller/eval_genima.py:91-103), statement for statement: the gate that every non-clip key
    of ``controller_agent.state_dict()`` is present in ``checkpoint["agent"]``, then ``load_state_dict(..., strict=False)``."""
    checkpoint = torch.load(checkpoint_path, map_location=device, weights_only=False)
    missing_keys = [k for k in controller_agent.state_dict().keys() if k not in checkpoint["agent"].keys() and "clip" not in k]
    if len(missing_keys) > 0:
        raise ValueError(f"Missing keys in controller checkpoint: {missing_keys}")
    controller_agent.load_state_dict(checkpoint["agent"], strict=False)
    return checkpoint


def save_snapshot(controller_agent, path, cfg=None, epoch: int = 0, num_iters: int = 0):
    """``ControllerWorkspace.save_snapshot`` (controller/train_act.py:262-279): ``{"cfg", "_epoch", "_num_iters", "agent"}`` with the
    ``clip_model`` keys filtered out of the agent's state dict, written with ``torch.save``."""
    import os

    state_dict = {k: v for k, v in controller_agent.state_dict().items() if "clip_model" not in k}
    payload = {"cfg": cfg, "_epoch": epoch, "_num_iters": num_iters, "agent": state_dict}
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(path, "wb") as f:
        torch.save(payload, f)
    return payload
