"""Training data path of the ControlNet fine-tune: RLBench PNG reader, the trainer's
pre-processing and collate, and the hand-over to the device.

Reference: ``diffusion/rlbench_dataset/rlbench_dataset.py:70-210`` (a HF ``datasets`` builder yielding {text, image, conditioning_image}),
``diffusion/train_controlnet_genima.py:870-964`` (``tokenize_captions``, Resize(bilinear) -> CenterCrop -> ToTensor (-> Normalize(0.5,
0.5) for the target), ``collate_fn`` stacking float32 NCHW tensors) and ``:775-830`` (``augment_data``, on the device here:
genima_amd/augment.py).

MI355X-first hand-over: the host decodes, resizes and crops to **uint8 NHWC** and nothing more; ``to_device`` uploads the bytes (a
quarter of the float32 NCHW volume over PCIe) and ``ToTensor`` / ``Normalize`` / NCHW -> 8-channel NHWC f16 happen in ONE HIP kernel
per tensor (``gn_image_u8_to_f16``) -- the layout ``ControlNetTrainer.train_step`` consumes directly.  ``collate_fn`` keeps the
reference's float NCHW contract for callers that want it (numpy; no torch compute).

Opt-in frame cache (``DataLoader(cache="host" | "device")``): the reference trains 100-200 epochs over one small set of files, so a
decoded frame is kept where the next epoch reads it -- in pinned host chunks, or in device chunks from which ``gn_gather_u8_to_f16``
assembles the batch (``FrameCache``, ``to_device``).  The cache assumes the files do not change during a run.

Reference quirks reproduced on purpose: the tiled caption is the truncated string
``"tiled perspectives of a robot "`` (the task description sits in a dangling f-string statement that is evaluated -- it advances
numpy's global RNG through ``np.random.choice`` -- and discarded), and the tiled reader drops the last frame of every episode.
"""
from __future__ import annotations

import io
import os
import pickle
import random
import re
import threading
from concurrent.futures import ThreadPoolExecutor
from queue import Queue
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch


def _natural_key(s: str):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]


class RLBenchDataset:
    """Index of (image, conditioning image, caption) examples in the on-disk layout ``render_data.py`` writes:
    ``<data_path>/<task>/variation<k>/episodes/<episode>/{rgb, rgb_rendered}/<i>.png`` (tiled) or ``<camera>_{rgb, rgb_rendered}`` (per
    camera), ``variation_descriptions.pkl`` beside ``episodes``.  Same constructor knobs as the reference's ``RLBenchConfig``."""

    def __init__(self, data_path: str = "/tmp/rlbench_dataset/", tasks: str = "take_lid_off_saucepan", variation: int = 0,
                 num_demos: int = 50, cameras: str = "wrist,front,left_shoulder,right_shoulder", image_type: str = "rgb_rendered",
                 conditioning_image_type: str = "rgb", tiled: bool = True, predict_future: bool = False, predict_future_horizon: int = 20):
        self.examples: List[Dict[str, str]] = []
        for task in tasks.split(","):
            var = f"variation{variation}"
            eps_folder = os.path.join(data_path, task, var, "episodes")
            with open(os.path.join(data_path, task, var, "variation_descriptions.pkl"), "rb") as f:
                descriptions = pickle.load(f)
            demos = [d for d in os.listdir(eps_folder) if os.path.isdir(os.path.join(eps_folder, d))]
            selected = sorted(os.listdir(eps_folder), key=_natural_key)[: min(len(demos), num_demos)]
            for ep in selected:
                views = [None] if tiled else cameras.split(",")
                for cam in views:
                    pre = "" if cam is None else cam + "_"
                    rgb_path = os.path.join(eps_folder, ep, pre + conditioning_image_type)
                    render_path = os.path.join(eps_folder, ep, pre + image_type)
                    np.random.choice(descriptions)  # evaluated and discarded by the reference too (rlbench_dataset.py:118-119, :170-171)
                    text = "tiled perspectives of a robot " if tiled else "a robot arm executing '"
                    n = len([f for f in os.listdir(render_path) if ".png" in f]) - (1 if tiled else 0)  # tiled: last frame dropped (:121-123)
                    for i in range(n):
                        j = min(i + predict_future_horizon, n - 1) if predict_future else i
                        self.examples.append({"text": text, "image": os.path.join(render_path, f"{j}.png"),
                                              "conditioning_image": os.path.join(rgb_path, f"{i}.png")})

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i: int) -> Dict[str, object]:
        ex = self.examples[i]
        out = {"text": ex["text"]}
        for k in ("image", "conditioning_image"):
            with open(ex[k], "rb") as f:
                out[k] = {"path": ex[k], "bytes": f.read()}
        return out


def resize_center_crop_u8(png_bytes_or_image, resolution: int) -> np.ndarray:
    """``image.convert("RGB")`` -> Resize(resolution, BILINEAR) (shorter side, aspect kept, torchvision's size rule) -> CenterCrop ->
    uint8 HWC (train_controlnet_genima.py:895-915 up to, not including, ToTensor)."""
    from PIL import Image

    im = png_bytes_or_image
    if isinstance(im, dict):
        im = im["bytes"]
    if isinstance(im, (bytes, bytearray)):
        im = Image.open(io.BytesIO(im))
    im = im.convert("RGB")
    w, h = im.size
    if min(w, h) != resolution:
        if w <= h:
            nw, nh = resolution, int(resolution * h / w)
        else:
            nw, nh = int(resolution * w / h), resolution
        im = im.resize((nw, nh), Image.BILINEAR)
        w, h = im.size
    left, top = int(round((w - resolution) / 2.0)), int(round((h - resolution) / 2.0))
    return np.asarray(im.crop((left, top, left + resolution, top + resolution)), dtype=np.uint8)


def tokenize_captions(captions: Sequence, tokenizer, proportion_empty_prompts: float = 0.0, is_train: bool = True) -> torch.Tensor:
    """train_controlnet_genima.py:870-891 (python's ``random`` for the empty-prompt draw and the multi-caption choice)."""
    out = []
    for c in captions:
        if random.random() < proportion_empty_prompts:
            out.append("")
        elif isinstance(c, str):
            out.append(c)
        elif isinstance(c, (list, np.ndarray)):
            out.append(random.choice(c) if is_train else c[0])
        else:
            raise ValueError("caption column should contain either strings or lists of strings")
    return tokenizer(out, max_length=tokenizer.model_max_length, padding="max_length", truncation=True, return_tensors="pt").input_ids


def collate_u8(examples: Sequence[Dict], tokenizer, resolution: int, proportion_empty_prompts: float = 0.0) -> Dict[str, torch.Tensor]:
    """Host half of preprocess_train + collate: uint8 NHWC stacks + token ids (pinned when a GPU is present)."""
    px = np.stack([resize_center_crop_u8(e["image"], resolution) for e in examples])
    cd = np.stack([resize_center_crop_u8(e["conditioning_image"], resolution) for e in examples])
    ids = tokenize_captions([e["text"] for e in examples], tokenizer, proportion_empty_prompts)
    batch = {"pixel_values_u8": torch.from_numpy(px), "conditioning_pixel_values_u8": torch.from_numpy(cd), "input_ids": ids}
    if torch.cuda.is_available():
        batch = {k: v.pin_memory() for k, v in batch.items()}
    return batch


def collate_fn(examples: Sequence[Dict], tokenizer, resolution: int, proportion_empty_prompts: float = 0.0) -> Dict[str, torch.Tensor]:
    """The reference's batch contract (train_controlnet_genima.py:934-964): float32 NCHW ``pixel_values`` in [-1, 1] (ToTensor +
    Normalize([0.5], [0.5])), ``conditioning_pixel_values`` in [0, 1], int64 ``input_ids`` [b, 77]."""
    b = collate_u8(examples, tokenizer, resolution, proportion_empty_prompts)
    px = b["pixel_values_u8"].numpy().astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    cd = b["conditioning_pixel_values_u8"].numpy().astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    return {"pixel_values": torch.from_numpy(np.ascontiguousarray((px - np.float32(0.5)) / np.float32(0.5))),
            "conditioning_pixel_values": torch.from_numpy(np.ascontiguousarray(cd)), "input_ids": b["input_ids"]}


def to_device(E, batch_u8: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """uint8 NHWC host batch -> what ``ControlNetTrainer.train_step`` takes: f16 NHWC 8-channel tensors on the device, ToTensor +
    Normalize fused into the byte -> half conversion kernel (target: v / 255 * 2 - 1, conditioning: v / 255).  A device-cache batch
    (``DataLoader(cache="device")``: ``frame_slots``) has its misses uploaded into their cache slots and is assembled by one
    ``gn_gather_u8_to_f16`` launch per role, all on the caller's thread and the engine's current stream; the result is the same, bit for bit."""
    dev = E.device
    if "render_views" in batch_u8:
        return _to_device_rendered(E, batch_u8)
    if "frame_slots" in batch_u8:
        return _to_device_cached(E, batch_u8)
    px = batch_u8["pixel_values_u8"].to(dev, non_blocking=True)
    cd = batch_u8["conditioning_pixel_values_u8"].to(dev, non_blocking=True)
    return {"pixel_values": E.image_u8_to_f16(px, 8, 2.0, -1.0), "conditioning_pixel_values": E.image_u8_to_f16(cd, 8, 1.0, 0.0),
            "input_ids": batch_u8["input_ids"].to(dev, non_blocking=True)}


def _to_device_cached(E, batch) -> Dict[str, torch.Tensor]:
    cache, R, slots = batch["frame_cache"], int(batch["resolution"]), batch["frame_slots"]
    dev = E.device
    cache.upload(dev, R, batch["frame_uploads"])
    staging = batch["frame_staging_u8"]
    if staging is not None:  # misses over the budget: this batch's own device copy, freed with the batch
        staging = staging.to(dev, non_blocking=True)
    fb = R * R * 3
    addr = [staging.data_ptr() + i * fb if c < 0 else cache.address(R, c, i) for c, i in slots.tolist()]
    ptrs = torch.tensor(addr, dtype=torch.int64)
    if torch.cuda.is_available():
        ptrs = ptrs.pin_memory()
    ptrs = ptrs.to(dev, non_blocking=True)
    B = len(addr) // 2  # rows 0..B-1: the targets, B..2B-1: the conditioning images
    out = {"pixel_values": E.gather_u8_to_f16(ptrs[:B], (R, R), 8, 2.0, -1.0),
           "conditioning_pixel_values": E.gather_u8_to_f16(ptrs[B:], (R, R), 8, 1.0, 0.0),
           "input_ids": batch["input_ids"].to(dev, non_blocking=True)}
    return out


def _to_device_rendered(E, batch) -> Dict[str, torch.Tensor]:
    """A ``DataLoader(render_targets=...)`` batch: the conditioning frames (uploaded, or where they lie in the device cache, through the
    same pointer table ``gn_gather_u8_to_f16`` reads) are the tiled backgrounds over which ``gn_render_spheres`` draws the targets,
    straight into the f16 NHWC-8 ``pixel_values``.  The view arrays were packed and pinned by the producer thread.

    Where the views carry ``M`` (``DataLoader(view_augment=...)``): one ``gn_view_augment_tiled`` launch reads the same frames, writes the
    warped and tinted tiled uint8 background, ``conditioning_pixel_values`` directly (scale (1, 0)) and the ``view_revealed`` table; the
    spheres are then drawn over that background with the perturbed cameras.  Without ``M`` the launches are the ones above."""
    dev, src = E.device, batch["render_source"]
    views = [batch["render_views"][k].to(dev, non_blocking=True) for k in ("cams", "spheres", "tex_index", "count")]
    aug = "M" in batch["render_views"]
    if "frame_slots" in batch:
        cache, R = batch["frame_cache"], int(batch["resolution"])
        cache.upload(dev, R, batch["frame_uploads"])
        staging = batch["frame_staging_u8"]
        if staging is not None:
            staging = staging.to(dev, non_blocking=True)
        fb = R * R * 3
        ptrs = torch.tensor([staging.data_ptr() + i * fb if c < 0 else cache.address(R, c, i) for c, i in batch["frame_slots"].tolist()],
                            dtype=torch.int64)
        ptrs = (ptrs.pin_memory() if torch.cuda.is_available() else ptrs).to(dev, non_blocking=True)
        B, bg, source = ptrs.numel(), dict(bg_frames=ptrs), dict(frames=ptrs)
        cond = None if aug else E.gather_u8_to_f16(ptrs, (R, R), 8, 1.0, 0.0)
    else:
        cd = batch["conditioning_pixel_values_u8"].to(dev, non_blocking=True)
        B, bg, source = cd.shape[0], dict(bg=cd), dict(src=cd)
        cond = None if aug else E.image_u8_to_f16(cd, 8, 1.0, 0.0)
    out = {}
    if aug:
        M, colour = (batch["render_views"][k].to(dev, non_blocking=True) for k in ("M", "colour"))
        warped = torch.empty((B, 2 * src.H, 2 * src.W, 3), dtype=torch.uint8, device=dev)
        cond = torch.empty((B, 2 * src.H, 2 * src.W, 8), dtype=torch.float16, device=dev)
        out["view_revealed"] = torch.empty((B, 4), dtype=torch.int32, device=dev)
        E.view_augment_tiled(M, colour, src.H, src.W, out_u8=warped, out_f16=cond, scale=(1.0, 0.0), n_revealed=out["view_revealed"], **source)
        bg = dict(bg=warped)
    px = torch.empty((B, 2 * src.H, 2 * src.W, 8), dtype=torch.float16, device=dev)
    E.render_spheres(*views, src.atlas_on(dev), src.H, src.W, src.samples, bg_tiled=True, n_tiled=B, full_f16=px, full_scale=(2.0, -1.0), **bg)
    return {"pixel_values": px, "conditioning_pixel_values": cond, "input_ids": batch["input_ids"].to(dev, non_blocking=True), **out}


class FrameCache:
    """Decoded training frames -- the uint8 HWC output of ``resize_center_crop_u8`` -- kept for the next epoch, keyed by
    ``(path, resolution)``: a file used in both roles, or by two loaders that share the cache, is stored once.

    Storage grows in fixed-size chunks of ``chunk_bytes`` (no single giant allocation): pinned host tensors for ``where="host"``, device
    ``torch.uint8`` tensors for ``where="device"``.  ``cache_bytes`` is a budget, not a working-set size: frames are admitted in the order
    they are first used until the chunks would exceed it; later frames are never admitted and nothing is evicted, so a frame that did not
    get in is decoded on every use, exactly as without a cache.  (Eviction would buy nothing here: every epoch reads every frame once.)

    The cache ASSUMES THAT THE FILES DO NOT CHANGE during a run: a frame is decoded once and never looked at again (no mtime or size
    check); ``clear()`` after rewriting the data.  Memory: resolution^2 * 3 bytes per frame -- 786 432 at 512^2, so a task of 25 demos
    (a few thousand frames) is 2-4 GB and eight tasks in two roles are in the order of 50 GB of the MI355X's 288 GB.

    ``hits`` / ``misses`` count frame uses served from / not found in the cache, ``decodes`` the frames decoded through it."""

    def __init__(self, where: str = "host", cache_bytes: int = 8 << 30, chunk_bytes: int = 256 << 20):
        if where not in ("host", "device"):
            raise ValueError(f"FrameCache(where={where!r}): 'host' or 'device'")
        self.where, self.cache_bytes, self.chunk_bytes = where, int(cache_bytes), int(chunk_bytes)
        self._lock = threading.Lock()
        self.clear()

    def clear(self):
        """Forget every frame and free the chunks (batches still in flight must not be handed to ``to_device`` afterwards)."""
        with self._lock:
            self._index: Dict[Tuple[str, int], Tuple[int, int]] = {}  # (path, resolution) -> (chunk, frame in chunk)
            self._caps: Dict[int, List[int]] = {}  # resolution -> frames per chunk (the last chunk is cut to the budget)
            self._chunks: Dict[int, List[torch.Tensor]] = {}  # resolution -> [frames, R, R, 3] uint8 tensors (device: made in upload())
            self._used: Dict[int, int] = {}  # resolution -> slots handed out so far
            self._free: Dict[int, List[Tuple[int, int]]] = {}  # slots given back by a failed batch
            self._pending: Dict[Tuple[int, int, int], torch.Tensor] = {}  # device cache: (resolution, chunk, frame) -> frame not uploaded yet
            self._ready = None  # device cache: event after the last upload (a gather on another stream waits for it)
            self._allocated = 0
            self.hits = self.misses = self.decodes = 0

    def __len__(self):
        return len(self._index)

    @property
    def nbytes(self) -> int:
        """Bytes of the frames held (the chunks' capacity, ``allocated_bytes``, is what the budget bounds: nbytes <= allocated_bytes <= cache_bytes)."""
        with self._lock:
            return sum(k[1] * k[1] * 3 for k in self._index)

    @property
    def allocated_bytes(self) -> int:
        return self._allocated

    # ---- producer side (the loader's thread) ----
    def lookup(self, key):
        """-> (slot, frame still waiting for its upload or None) of a cached frame, or None."""
        with self._lock:
            slot = self._index.get(key)
            if slot is None:
                self.misses += 1
                return None
            self.hits += 1
            return slot, self._pending.get((key[1],) + slot)

    def reserve(self, resolution: int) -> Optional[Tuple[int, int]]:
        """A free slot for one frame, or None when the budget is spent."""
        R, fb = resolution, resolution * resolution * 3
        with self._lock:
            if self._free.get(R):
                return self._free[R].pop()
            caps = self._caps.setdefault(R, [])
            used = self._used.get(R, 0)
            if used == sum(caps):
                cap = min(max(1, self.chunk_bytes // fb), (self.cache_bytes - self._allocated) // fb)
                if cap <= 0:
                    return None
                caps.append(cap)
                self._allocated += cap * fb
                if self.where == "host":
                    self._chunks.setdefault(R, []).append(torch.empty((cap, R, R, 3), dtype=torch.uint8, pin_memory=torch.cuda.is_available()))
            self._used[R] = used + 1
            c = len(caps) - 1
            return c, used - sum(caps[:c])

    def release(self, resolution: int, slot):
        with self._lock:
            self._free.setdefault(resolution, []).append(slot)

    def count_decodes(self, n: int):
        with self._lock:
            self.decodes += n

    def commit(self, key, slot, frame: np.ndarray):
        """The decoded ``frame`` now belongs to ``key``: copied into its host chunk, or (device cache) pinned and queued for the upload that
        ``to_device`` does.  -> (slot, pending frame or None) as ``lookup``; another loader's slot if it got there first."""
        R = key[1]
        t = torch.from_numpy(frame)
        with self._lock:
            have = self._index.get(key)
            if have is not None:
                self._free.setdefault(R, []).append(slot)
                return have, self._pending.get((R,) + have)
            if self.where == "host":
                self._chunks[R][slot[0]][slot[1]].copy_(t)
                t = None
            else:
                t = t.pin_memory() if torch.cuda.is_available() else t
                self._pending[(R,) + slot] = t
            self._index[key] = slot
            return slot, t

    def frame(self, resolution: int, slot) -> torch.Tensor:
        """Host cache: the stored frame (a view into its chunk)."""
        return self._chunks[resolution][slot[0]][slot[1]]

    # ---- consumer side (to_device: the caller's thread and current stream) ----
    def upload(self, device, resolution: int, uploads):
        """Device cache: make the chunks the loader has planned so far, and copy the frames of ``uploads`` (``(chunk, frame, pinned
        tensor)``) that are still waiting into their slots.  A later gather on another stream is ordered behind the copies by an event."""
        R = resolution
        with self._lock:
            chunks = self._chunks.setdefault(R, [])
            for cap in self._caps.get(R, [])[len(chunks):]:
                chunks.append(torch.empty((cap, R, R, 3), dtype=torch.uint8, device=device))
            todo = [(c, i, self._pending.pop((R, c, i))) for c, i, _ in uploads if (R, c, i) in self._pending]
        stream = torch.cuda.current_stream(device)
        if self._ready is not None:
            stream.wait_event(self._ready)
        for c, i, t in todo:
            chunks[c][i].copy_(t, non_blocking=True)
        if todo:
            self._ready = torch.cuda.Event()
            self._ready.record(stream)

    def address(self, resolution: int, chunk: int, frame: int) -> int:
        return self._chunks[resolution][chunk].data_ptr() + frame * resolution * resolution * 3


class DataLoader:
    """``torch.utils.data.DataLoader(train_dataset, shuffle=True, collate_fn=collate_fn, batch_size=, num_workers=)``
    (train_controlnet_genima.py:1187-1193) for the uint8 path: seeded shuffle per epoch, last partial batch kept, and a background
    thread that decodes / resizes ``prefetch`` batches ahead so PNG decoding overlaps the device step (the reference's default
    ``num_workers=0`` decodes inline and can starve 8 GPUs).

    ``decode_workers`` > 1 (at most 16) fans the image decodes of a batch out over a thread pool, in order; captions are still tokenized
    on the one producer thread, in batch order, so python's ``random`` draws as before.  ``cache`` = "host" | "device" (or a
    ``FrameCache`` to share) keeps decoded frames for the following epochs within ``cache_bytes``: "host" yields the same batches as no
    cache, "device" yields batches that name cache slots (``frame_slots``) for ``to_device`` / ``train_step`` to gather on the device.  The
    producer thread launches no device work.  The cache assumes the files do not change during a run (``FrameCache``).

    ``render_targets`` (a ``render.TrajectorySource``; off by default): the target image of a sample is not read from its PNG but drawn on
    the device -- the trajectory's spheres over the sample's conditioning frame (``gn_render_spheres``, in ``to_device`` / ``train_step``) --
    so only the conditioning frames are decoded, and cached when ``cache`` is on.  For datasets whose targets are the rendering of their own
    conditioning frame (the tiled ``tiled_rgb`` / ``tiled_rgb_rendered`` pair without ``predict_future``).

    ``view_augment`` (a ``perturb.Perturbation``, a spec string or a preset name, read through ``perturb.parse``; off by default; needs
    ``render_targets``): the camera-pose and light perturbation the open-loop evaluator measures with (``OpenLoopEval(perturb=...)``), as a
    train-time augmentation with re-drawn targets.  With probability ``view_augment_prob`` a sample's four views are perturbed: the
    OBSERVATION is warped by the homography of its turned camera and tinted by the light's gain and offset (``gn_view_augment_tiled``,
    in ``to_device`` / ``train_step``), and the target's spheres are drawn UNTINTED over that frame from the turned camera's table -- the
    spheres are the signal, not scene, as DESIGN 3.19 argues for the evaluator.  The border the turned camera reveals is MIRRORED scene, not
    what it would have seen there; the batch's ``view_revealed`` (int32 [B, 4] on the device, read back by nothing here) counts it.  A
    sphere that leaves a view is simply not in that view's target.  The rotation and a change of intrinsics are exact, the light is an
    image-space stand-in, a camera translation is left out, and the ranges are the caller's choice (``perturb.py``).

    A sample's draw is a pure function of ``(view_augment_seed, epoch, dataset index)`` (``perturb.sample_tables``), ``epoch`` the value
    the epoch's shuffle used and ``view_augment_seed=None`` the loader's ``seed``: it does not depend on the batch size or composition, the
    rank, the world size, ``prefetch``, ``decode_workers`` or the cache, and a sample the data-parallel tail repeats gets the same draw.
    The producer thread computes the tables (``M``, ``colour`` and the perturbed ``cams`` in ``render_views``) and launches nothing.
    ``--augmentations`` of the trainer run afterwards, as before; the change mask of ``sphere_loss_weight`` / ``loss_parts`` is taken
    between the warped target and the warped frame.  A held-out loader (``eval_loss``) is unaffected as long as it sets no ``view_augment``."""

    MAX_DECODE_WORKERS = 16  # a fixed cap, never the machine's CPU count: a training host runs one loader per GPU

    def __init__(self, dataset, batch_size: int, tokenizer, resolution: int, shuffle: bool = True, seed: int = 0, prefetch: int = 2,
                 proportion_empty_prompts: float = 0.0, rank: int = 0, world: int = 1, cache=None, cache_bytes: int = 8 << 30,
                 decode_workers: int = 1, render_targets=None, view_augment=None, view_augment_prob: float = 1.0,
                 view_augment_seed: Optional[int] = None):
        self.ds, self.bs, self.tok, self.res = dataset, batch_size, tokenizer, resolution
        self.render_targets = render_targets
        if render_targets is not None and (resolution != 2 * render_targets.H or resolution != 2 * render_targets.W):
            raise ValueError(f"render_targets draws {2 * render_targets.H} x {2 * render_targets.W} tiled targets: resolution must be that, not {resolution}")
        self.view_augment = None
        if not 0.0 <= float(view_augment_prob) <= 1.0:  # (a NaN fails the comparison)
            raise ValueError(f"view_augment_prob = {view_augment_prob} must lie in [0, 1]")
        if view_augment is not None:
            from . import perturb

            if render_targets is None:
                raise ValueError("view_augment needs render_targets: without the trajectory there is no camera to turn and no target to re-draw")
            self.view_augment = perturb.parse(view_augment)
        self.view_augment_prob = float(view_augment_prob)
        self.view_augment_seed = int(seed if view_augment_seed is None else view_augment_seed)
        if self.view_augment is not None and self.view_augment_seed < 0:
            raise ValueError(f"view_augment_seed = {self.view_augment_seed} must not be negative (it is part of a numpy seed sequence)")
        self.shuffle, self.seed, self.prefetch, self.pep = shuffle, seed, max(0, prefetch), proportion_empty_prompts
        self.rank, self.world, self.epoch = rank, world, 0
        self.cache = FrameCache(cache, cache_bytes) if isinstance(cache, str) else cache
        self.decode_workers = max(1, min(int(decode_workers), self.MAX_DECODE_WORKERS))
        self._pool = ThreadPoolExecutor(self.decode_workers, thread_name_prefix="genima-decode") if self.decode_workers > 1 else None

    def __len__(self):
        n_batches = (len(self.ds) + self.bs - 1) // self.bs
        return (n_batches + self.world - 1) // self.world  # the same on every rank (a shorter rank would leave the others in a collective)

    def _batches(self) -> List[List[int]]:
        idx = list(range(len(self.ds)))
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(idx)
        if self.world > 1 and idx:
            # data parallel, as accelerate's prepared loader shards (BatchSamplerShard, even_batches=True): the epoch's permutation is
            # cut into batches, batch k goes to rank k % world, and the tail is completed by wrapping round to the start of the
            # permutation so that every rank runs the same number of full batches
            unit = self.bs * self.world
            total = (len(idx) + unit - 1) // unit * unit
            idx = (idx * (total // len(idx) + 1))[:total]
        batches = [idx[i:i + self.bs] for i in range(0, len(idx), self.bs)]
        return batches[self.rank::self.world]

    # ---- the cached / fanned-out batch (cache=None, decode_workers=1 stays collate_u8) ----
    def _sources(self, i: int):
        """-> (caption, [(path or None, payload or None)] for the target and the conditioning image).  A dataset that indexes paths
        (``RLBenchDataset.examples``) is not read here: a cache hit then touches no file, and a miss reads its file in the decode worker."""
        ex = getattr(self.ds, "examples", None)
        if ex is not None and isinstance(ex[i].get("image"), str):
            return ex[i]["text"], [(ex[i][k], None) for k in ("image", "conditioning_image")]
        e = self.ds[i]
        return e["text"], [(v.get("path") if isinstance(v, dict) else None, v) for v in (e["image"], e["conditioning_image"])]

    def _decode(self, job) -> np.ndarray:
        path, payload = job
        if payload is None:
            with open(path, "rb") as f:
                payload = f.read()
        return np.require(resize_center_crop_u8(payload, self.res), requirements="W")  # PIL's array is read-only; torch wants to own it

    def _decode_all(self, jobs) -> List[np.ndarray]:
        return list(self._pool.map(self._decode, jobs)) if self._pool is not None and len(jobs) > 1 else [self._decode(j) for j in jobs]

    def _make(self, ix: List[int], epoch: int = 0) -> Dict[str, object]:
        R, cache = self.res, self.cache
        meta = [self._sources(i) for i in ix]
        uses = [m[1][role] for role in (0, 1) for m in meta]  # the order collate_u8 decodes in: every target, then every conditioning image
        rendered = None
        if self.render_targets is not None:  # the targets are drawn on the device from the conditioning frames: those alone are decoded
            uses = uses[len(meta):]
            packed = [v for path, _ in uses for v in self.render_targets.views(path)]
            cams, tables = np.stack([v[0] for v in packed]), {}  # a stacked copy: TrajectorySource memoises its views and they stay clean
            if self.view_augment is not None:
                from . import perturb
                from .render import tile_cameras

                names = tile_cameras(self.render_targets.cfg.cameras)
                drawn = [perturb.sample_tables(self.view_augment, cams[4 * k:4 * k + 4], names, (self.view_augment_seed, epoch, i),
                                               self.view_augment_prob) for k, i in enumerate(ix)]
                cams = np.concatenate([d[0] for d in drawn])
                tables = {"M": torch.from_numpy(np.stack([d[1] for d in drawn])), "colour": torch.from_numpy(np.stack([d[2] for d in drawn]))}
            rendered = {**tables, "cams": torch.from_numpy(cams), "spheres": torch.from_numpy(np.stack([v[1] for v in packed])),
                        "tex_index": torch.from_numpy(np.stack([v[2] for v in packed]).astype(np.int32)),
                        "count": torch.tensor([v[3] for v in packed], dtype=torch.int32)}
            if torch.cuda.is_available():
                rendered = {k: v.pin_memory() for k, v in rendered.items()}
            rendered = {"render_views": rendered, "render_source": self.render_targets}
        # plan: per use a cached frame (hit) or a decode job; a frame admitted by this batch is decoded once however often the batch
        # names it (both roles, the data-parallel tail's wrap-around), one that is over the budget is decoded per use, as without a cache
        plan, jobs, keys, slots, fresh = [], [], [], [], {}
        for path, payload in uses:
            key = (path, R) if cache is not None and path is not None else None
            got = cache.lookup(key) if key is not None else None
            if got is None and key in fresh:
                got = ("job", fresh[key])
            elif got is None:
                slot = cache.reserve(R) if key is not None else None
                if slot is not None:
                    fresh[key] = len(jobs)
                got = ("job", len(jobs))
                jobs.append((path, payload)), keys.append(key if slot is not None else None), slots.append(slot)
            plan.append(got)
        try:
            frames = self._decode_all(jobs)
        except BaseException:
            for slot in slots:
                if slot is not None:
                    cache.release(R, slot)
            raise
        if cache is not None:
            cache.count_decodes(len(jobs))
        done = [cache.commit(k, s, f) if k is not None else None for k, s, f in zip(keys, slots, frames)]  # per job: (slot, pending) | None
        plan = [(done[g[1]] or ("frame", frames[g[1]])) if g[0] == "job" else g for g in plan]
        ids = tokenize_captions([m[0] for m in meta], self.tok, self.pep)
        pin = torch.cuda.is_available()
        if cache is not None and cache.where == "device":
            uploads, staging, where = {}, [], []
            for g in plan:
                if g[0] == "frame":  # over the budget: a staging slot of this batch
                    where.append((-1, len(staging)))
                    staging.append(torch.from_numpy(g[1]))
                else:
                    where.append(g[0])
                    if g[1] is not None:
                        uploads[g[0]] = g[1]
            stage = torch.stack(staging) if staging else None
            return {**(rendered or {}), "frame_cache": cache, "resolution": R, "frame_slots": torch.tensor(where, dtype=torch.int64).view(-1, 2),
                    "frame_uploads": [(c, i, t) for (c, i), t in uploads.items()],
                    "frame_staging_u8": stage.pin_memory() if pin and stage is not None else stage,
                    "input_ids": ids.pin_memory() if pin else ids}
        B = len(ix)
        out = torch.empty((len(plan), R, R, 3), dtype=torch.uint8, pin_memory=pin)
        for o, g in zip(out, plan):
            o.copy_(torch.from_numpy(g[1]) if g[0] == "frame" else cache.frame(R, g[0]))
        if rendered is not None:
            return {**rendered, "conditioning_pixel_values_u8": out, "input_ids": ids.pin_memory() if pin else ids}
        return {"pixel_values_u8": out[:B], "conditioning_pixel_values_u8": out[B:], "input_ids": ids.pin_memory() if pin else ids}

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        epoch = self.epoch  # the value the shuffle below uses: part of a view_augment draw's key
        batches = self._batches()
        self.epoch += 1

        def make(ix):
            if self.cache is None and self._pool is None and self.render_targets is None:
                return collate_u8([self.ds[i] for i in ix], self.tok, self.res, self.pep)
            return self._make(ix, epoch)

        if self.prefetch == 0:
            for ix in batches:
                yield make(ix)
            return
        q: Queue = Queue(maxsize=self.prefetch)

        def worker():
            try:
                for ix in batches:
                    q.put(make(ix))
                q.put(None)
            except BaseException as e:  # surface decoding errors in the consumer
                q.put(e)
        threading.Thread(target=worker, daemon=True).start()
        while True:
            item = q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item
