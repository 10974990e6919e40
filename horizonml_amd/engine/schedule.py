"""Learning-rate schedules for the fused optimizer step.

The flat engine captures the whole training step in a hipGraph, so anything
that changes per step has to live on the device.  A schedule is therefore
evaluated once, on the host, in float64, and shipped as a float32 table
``[total_steps]``; the fused Adam/SGD kernels index it with the device step
counter (``lr_table[min(step_t - 1, T - 1)]``).  A table instead of in-kernel
maths because the kernels are built with ``-ffast-math`` (an in-kernel
``cosf`` has no derivable bound against a host mirror), and because a table
admits any schedule; it costs one wave-uniform 4-byte load per thread.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

KINDS = ("constant", "cosine", "linear", "multistep")

# The device step counter is an f32 scalar: it counts exactly up to 2**24.
MAX_STEPS = 2 ** 24


class LRSchedule:
    """``lr_at(t)`` for the 0-based update index ``t``:

    * ``t < warmup_steps``: ``base_lr * (t + 1) / warmup_steps``;
    * otherwise, with ``p = min(1, (t - warmup_steps) /
      max(1, total_steps - warmup_steps))``:
      ``cosine``  ``min_lr + (base_lr - min_lr) * (1 + cos(pi * p)) / 2``,
      ``linear``  ``base_lr + (min_lr - base_lr) * p``,
      ``multistep``  ``base_lr * gamma ** #(milestones <= t)``,
      ``constant``  ``base_lr``;
    * ``t >= total_steps`` holds ``lr_at(total_steps - 1)``.
    """

    def __init__(self, kind: str, base_lr: float, total_steps: int,
                 warmup_steps: int = 0, min_lr: float = 0.0,
                 milestones: Sequence[int] = (), gamma: float = 0.1):
        if kind not in KINDS:
            raise ValueError(f"unknown schedule {kind!r}; one of {KINDS}")
        total_steps = int(total_steps)
        if total_steps < 1:
            raise ValueError("total_steps must be >= 1")
        if total_steps >= MAX_STEPS:
            raise ValueError(
                f"total_steps must be < 2**24 (the device step counter is "
                f"an f32 scalar and must stay exact), got {total_steps}")
        warmup_steps = int(warmup_steps)
        if warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        self.kind = kind
        self.base_lr = float(base_lr)
        self.total_steps = total_steps
        self.warmup_steps = warmup_steps
        self.min_lr = float(min_lr)
        self.milestones = tuple(sorted(int(m) for m in milestones))
        self.gamma = float(gamma)

    def lr_at(self, t: int) -> float:
        t = int(t)
        if t >= self.total_steps:
            t = self.total_steps - 1
        if t < self.warmup_steps:
            return self.base_lr * (t + 1) / self.warmup_steps
        p = min(1.0, (t - self.warmup_steps)
                / max(1, self.total_steps - self.warmup_steps))
        if self.kind == "cosine":
            return self.min_lr + (self.base_lr - self.min_lr) * 0.5 * (
                1.0 + math.cos(math.pi * p))
        if self.kind == "linear":
            return self.base_lr + (self.min_lr - self.base_lr) * p
        if self.kind == "multistep":
            k = sum(1 for m in self.milestones if m <= t)
            return self.base_lr * self.gamma ** k
        return self.base_lr

    def table(self) -> torch.Tensor:
        """float32 ``[total_steps]``: ``lr_at(0..T-1)``, each value rounded
        once from float64."""
        vals = [self.lr_at(t) for t in range(self.total_steps)]
        return torch.tensor(vals, dtype=torch.float64).to(torch.float32)

    def __repr__(self):
        return (f"LRSchedule({self.kind!r}, base_lr={self.base_lr}, "
                f"total_steps={self.total_steps}, "
                f"warmup_steps={self.warmup_steps}, min_lr={self.min_lr}, "
                f"milestones={self.milestones}, gamma={self.gamma})")


def schedule_from_epochs(kind: str, base_lr: float, epochs: int,
                         steps_per_epoch: int, warmup_epochs: float = 0.0,
                         min_lr: float = 0.0, milestones: Sequence[int] = (),
                         gamma: float = 0.1) -> LRSchedule:
    """The entry points speak epochs; the schedule speaks steps."""
    spe = max(1, int(steps_per_epoch))
    return LRSchedule(kind, base_lr, max(1, int(epochs) * spe),
                      warmup_steps=int(round(warmup_epochs * spe)),
                      min_lr=min_lr,
                      milestones=[int(m) * spe for m in milestones],
                      gamma=gamma)
