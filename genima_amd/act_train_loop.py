"""The epoch loop of the reference's controller training (``ControllerWorkspace._train`` / ``save_snapshot``, controller/train_act.py:195-279)
over a ``replay.DeviceReplay``: resume from ``latest.pt``, iterate the sampler once per epoch, rotate and prune checkpoints, write snapshots
with the reference's payload, and put the two statistics JSON files where the reference's evaluation wrappers look for them."""
from __future__ import annotations

import json
import os
import shutil
from typing import Callable, Dict, Optional

from . import harness
from .data import _natural_key
from .replay import ACTION_STATS_JSON, PROPRIO_STATS_JSON, save_stats


class ControllerTrainLoop:
    """``ControllerTrainLoop(agent, replay, work_dir).train()`` replaces ``ControllerWorkspace.train()``.

    ``agent``: a ``GenimaACT`` (``update_device``, ``state_dict``, ``load_state_dict``); ``replay``: a ``DeviceReplay`` (an iterable of device
    batches that restarts an epoch on ``iter()``, with ``action_stats`` / ``proprio_stats``).  Snapshots go to
    ``<work_dir>/snapshots/<experiment_name>/``: ``latest.pt``, the rotated ``<epoch>.pt`` files and the statistics JSON files.

    Host logic of the reference, kept: a snapshot is written at ``epoch % checkpoint_every == 0``; before that ``latest.pt`` is renamed to
    ``<max(0, epoch - checkpoint_every)>.pt`` and the numbered files are pruned, oldest first in natural order, to ``num_checkpoints``; the
    payload is ``{"cfg", "_epoch", "_num_iters", "agent"}`` with the ``clip_model`` keys filtered out (``harness.save_snapshot``) and nothing
    else -- so, as in the reference, it carries NO optimizer moments: a resumed run restarts AdamW's moments (and the loss scale) from
    scratch on the loaded weights.

    Two deliberate differences.  ``_epoch`` in the payload is the number of FINISHED epochs (``epoch + 1``), so a resumed run goes on with the
    next epoch; the reference stores ``epoch`` and trains the last finished epoch a second time after a resume.  And an exception inside an
    update is raised, not printed and skipped as the reference does: a failing kernel must not turn into a run that silently trains on fewer
    batches.

    ``validate``: an optional callable ``(agent, epochs_done) -> Dict[str, float]`` (``openloop.controller_validator`` makes one), called right
    after a snapshot is written.  Its dict goes, with ``_epoch`` and ``_num_iters``, as one line into ``<ckpt_dir>/validation.jsonl``; when it
    has the key ``select`` and that is the lowest seen so far -- over this run and, after a resume, over the lines already in the file --
    ``latest.pt`` is copied to ``best.pt``, which the rotation never prunes.  Without ``validate`` nothing changes: same files, same bytes."""

    def __init__(self, agent, replay, work_dir: str, experiment_name: str = "genima_controller", num_train_epochs: int = 1000,
                 checkpoint_every: int = 10, num_checkpoints: int = 3, log: Optional[Callable[[Dict[str, float], int], None]] = None, cfg=None,
                 validate: Optional[Callable[[object, int], Dict[str, float]]] = None):
        self.agent, self.replay, self.work_dir, self.experiment_name = agent, replay, str(work_dir), experiment_name
        self.num_train_epochs, self.checkpoint_every, self.num_checkpoints = int(num_train_epochs), int(checkpoint_every), int(num_checkpoints)
        if self.checkpoint_every < 1 or self.num_checkpoints < 0:
            raise ValueError("ControllerTrainLoop: checkpoint_every must be >= 1 and num_checkpoints >= 0")
        self.log, self.validate = log, validate
        self.cfg = cfg if cfg is not None else {"experiment_name": experiment_name, "num_train_epochs": self.num_train_epochs,
                                                 "checkpoint_every": self.checkpoint_every, "num_checkpoints": self.num_checkpoints,
                                                 "method": dict(getattr(agent, "config", None) or {})}
        self._epoch, self._num_iters = 0, 0
        self.ckpt_dir = os.path.join(self.work_dir, "snapshots", experiment_name)
        snapshot_path = os.path.join(self.ckpt_dir, "latest.pt")
        if not os.path.exists(self.ckpt_dir):
            os.makedirs(self.ckpt_dir)
        elif os.path.isfile(snapshot_path):
            self.load_snapshot(snapshot_path)
            if hasattr(self.replay, "draw"):  # a render-mode replay: go on with the next backgrounds, not the run's first ones again
                self.replay.draw = self._num_iters
        self.best_select = self._best_so_far() if validate is not None else None

    def load_snapshot(self, path: str):
        ckpt = harness.load_controller_ckpt(self.agent, path)
        self._epoch, self._num_iters = int(ckpt["_epoch"]), int(ckpt["_num_iters"])
        return ckpt

    def save_snapshot(self, ckpt_name: str, epochs_done: int):
        return harness.save_snapshot(self.agent, os.path.join(self.ckpt_dir, f"{ckpt_name}.pt"), cfg=self.cfg, epoch=epochs_done,
                                     num_iters=self._num_iters)

    def _rotate(self, epoch: int):
        latest = os.path.join(self.ckpt_dir, "latest.pt")
        if os.path.exists(latest):
            os.rename(latest, os.path.join(self.ckpt_dir, f"{max(0, epoch - self.checkpoint_every)}.pt"))
        ckpts = sorted((pt for pt in os.listdir(self.ckpt_dir) if pt.endswith(".pt") and pt not in ("latest.pt", "best.pt")), key=_natural_key)
        for pt in ckpts[: max(0, len(ckpts) - self.num_checkpoints)]:
            os.remove(os.path.join(self.ckpt_dir, pt))

    def _best_so_far(self) -> Optional[float]:
        """The lowest ``select`` among the lines of ``validation.jsonl`` (an earlier run's, on a resume), or None."""
        path, best = os.path.join(self.ckpt_dir, "validation.jsonl"), None
        if os.path.isfile(path) and os.path.isfile(os.path.join(self.ckpt_dir, "best.pt")):
            with open(path) as f:
                for line in f:
                    v = json.loads(line).get("select") if line.strip() else None
                    if v is not None and (best is None or float(v) < best):
                        best = float(v)
        return best

    def _validate(self, epochs_done: int):
        scores = dict(self.validate(self.agent, epochs_done))
        with open(os.path.join(self.ckpt_dir, "validation.jsonl"), "a") as f:
            f.write(json.dumps(dict(scores, _epoch=epochs_done, _num_iters=self._num_iters)) + "\n")
        select = scores.get("select")
        if select is not None and (self.best_select is None or float(select) < self.best_select):
            self.best_select = float(select)
            shutil.copyfile(os.path.join(self.ckpt_dir, "latest.pt"), os.path.join(self.ckpt_dir, "best.pt"))

    def train(self) -> Dict[str, float]:
        """Run epochs ``_epoch .. num_train_epochs - 1`` -> the last step's metrics."""
        if not (os.path.exists(os.path.join(self.ckpt_dir, ACTION_STATS_JSON)) and os.path.exists(os.path.join(self.ckpt_dir, PROPRIO_STATS_JSON))):
            save_stats(self.ckpt_dir, self.replay.action_stats, self.replay.proprio_stats)
        if hasattr(self.agent, "train"):
            self.agent.train(True)
        metrics: Dict[str, float] = {}
        for epoch in range(self._epoch, self.num_train_epochs):
            for batch in iter(self.replay):
                metrics = self.agent.update_device(batch, self._num_iters)
                if self.log is not None:
                    self.log(metrics, self._num_iters)
                self._num_iters += 1
            self._epoch = epoch + 1
            if epoch % self.checkpoint_every == 0:
                self._rotate(epoch)
                self.save_snapshot("latest", epoch + 1)
                if self.validate is not None:
                    self._validate(epoch + 1)
        if hasattr(self.agent, "train"):
            self.agent.train(False)
        return metrics
