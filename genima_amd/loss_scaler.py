"""The GradScaler bookkeeping of the trainers (ControlNetTrainer / InstructPix2PixTrainer / ACTTrainer): the loss scale, the clean-step count,
the optimizer and scheduler step counters, the last gradient norm -- and the deferred read-back of the clip kernel's three scalars.

The found-inf flag of step k is needed on the host only when step k + 1 scales its loss, so a trainer may leave an asynchronous copy + event
behind (``update_async``) instead of blocking on it; every read or write of the scale or a counter ``settle``s that first, so a host sees
exactly what ``scaler.update()`` would have left.  torch only: the bookkeeping runs without a device."""
from __future__ import annotations

from typing import Optional

import torch


class LossScaler:
    """GradScaler defaults: backoff x0.5 on a non-finite step, growth x2 every ``growth_interval`` clean steps (None: never grows)."""

    def __init__(self, scale: float, growth_interval: Optional[int] = None):
        self.growth_interval = growth_interval
        self._scale, self._clean, self._opt_step, self._sched_step = float(scale), 0, 0, 0
        self._grad_norm: Optional[float] = None
        self._host: Optional[torch.Tensor] = None  # the ONE pinned buffer every deferred read-back lands in
        self._pending = None                       # (host tensor, event) of the update still in flight

    def _settled(name):  # noqa: N805 -- evaluated in the class body
        def get(self):
            self.settle()
            return getattr(self, name)

        def put(self, value):
            self.settle()
            setattr(self, name, value)
        return property(get, put)

    scale = _settled("_scale")
    clean = _settled("_clean")
    opt_step = _settled("_opt_step")      # advanced by the trainer BEFORE AdamW runs (Adam's bias correction); taken back by a skipped step
    sched_step = _settled("_sched_step")  # APPLIED steps: what the learning-rate schedule is advanced by
    grad_norm = _settled("_grad_norm")    # the unscaled global gradient norm of the last optimizer step (None before the first)
    del _settled

    @property
    def pending(self) -> bool:
        """Is an update queued by ``update_async`` / ``defer`` still waiting to be applied?"""
        return self._pending is not None

    def settle(self):
        """Apply the update still in flight, if any (a host wait for that step's clip kernel)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            host, event = pend
            event.synchronize()
            self.apply(*host.tolist())

    def apply(self, coef, norm, bad) -> bool:
        """GradScaler.update() from the clip kernel's (clip coefficient, gradient norm, found-inf flag).  True: the step was applied."""
        self.settle()
        self._grad_norm = norm
        if bad:
            self._scale *= 0.5
            self._clean = 0
            self._opt_step -= 1  # the skipped step does not advance Adam's bias correction
            return False
        self._sched_step += 1
        self._clean += 1
        if self.growth_interval is not None and self._clean >= self.growth_interval:
            self._scale *= 2.0
            self._clean = 0
        return True

    def update(self, clip: torch.Tensor) -> bool:
        """One host read of the clip tensor's three scalars, now."""
        self.settle()
        return self.apply(*clip.tolist())

    def defer(self, host: torch.Tensor, event):
        """``host`` holds the three scalars once ``event.synchronize()`` returns: apply them the next time anyone looks."""
        self.settle()
        self._pending = (host, event)

    def update_async(self, clip: torch.Tensor, stream: "torch.cuda.Stream"):
        """The same as ``update``, without waiting: the scalars go to pinned host memory behind whatever ``stream`` holds (the optimizer's
        kernels -- the copy must sit on the ENGINE's stream, whatever the caller's is), followed by an event."""
        self.settle()
        if self._host is None:
            self._host = torch.empty(3, dtype=torch.float32, pin_memory=True)
        with torch.cuda.stream(stream):
            self._host.copy_(clip, non_blocking=True)
        event = torch.cuda.Event()
        event.record(stream)
        self.defer(self._host, event)

    # ---- checkpoints: the five-scalar vector of optimizer_flat.safetensors
    def state_vector(self, global_step: int) -> torch.Tensor:
        return torch.tensor([self.opt_step, self.scale, self.clean, global_step, self.sched_step], dtype=torch.float64)

    def load_state_vector(self, vec) -> int:
        """-> the global step the vector was written at.  Four entries: a file from before ``sched_step`` was saved."""
        sc = [float(v) for v in vec]
        gstep = int(sc[3])
        self.opt_step, self.scale, self.clean = int(sc[0]), sc[1], int(sc[2])
        self.sched_step = int(sc[4]) if len(sc) > 4 else gstep
        return gstep
