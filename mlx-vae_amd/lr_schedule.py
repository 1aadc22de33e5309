"""Learning-rate schedules for the trainer (an extension: the reference trains at one rate, trainer.py:75-76).

A schedule is a pure function lr(s) of the number s of updates already applied, evaluated in Python floats on the host; the
step receives the value as a device word (arcvae_hip: lr_device=True), so a rate that changes every
step replays the same captured step.  No torch needed.

    s < W      : base * (s + 1) / W                                  linear warmup, reaching base at s = W - 1
    otherwise  : q = min(1, (s - W) / max(1, N - W)), r = min_lr_ratio
                 constant : base
                 linear   : base * (r + (1 - r) * (1 - q))
                 cosine   : base * (r + (1 - r) * 0.5 * (1 + cos(pi * q)))
Beyond N the last value is held (q = 1).  The un-bias-corrected Adam of this project (Q7) takes first steps of about
(1 - b1) / sqrt(1 - b2) ~ 3 times the nominal step, which is what the warmup is for.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

KINDS = ("constant", "linear", "cosine")


class LRSchedule:
    def __init__(self, base_lr: float, kind: str, warmup_steps: int = 0, total_steps: Optional[int] = None,
                 min_lr_ratio: float = 0.0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        base = float(base_lr)
        if not (math.isfinite(base) and base >= 0.0):
            raise ValueError(f"base_lr must be finite and >= 0, got {base_lr!r}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError(f"warmup_steps must be an integer >= 0, got {warmup_steps!r}")
        r = float(min_lr_ratio)
        if not (0.0 <= r <= 1.0):        # (NaN fails both comparisons)
            raise ValueError(f"min_lr_ratio must be in [0, 1], got {min_lr_ratio!r}")
        self.base_lr, self.kind, self.warmup_steps, self.min_lr_ratio = base, kind, int(warmup_steps), r
        self.total_steps = None
        if total_steps is not None:
            self.set_total_steps(total_steps)

    def set_total_steps(self, total_steps: int) -> None:
        if int(total_steps) != total_steps or total_steps < 0:
            raise ValueError(f"total_steps must be an integer >= 0, got {total_steps!r}")
        self.total_steps = int(total_steps)

    def validate(self) -> "LRSchedule":
        """ValueError unless lr(s) is defined: linear and cosine decay towards total_steps (which the constructor may leave
        open for the trainer to fill in from the run's length; lr() refuses until then)."""
        if self.kind != "constant" and self.total_steps is None:
            raise ValueError(f"a {self.kind} schedule needs total_steps")
        return self

    def lr(self, s: int) -> float:
        """The rate of the update that follows s applied updates."""
        if s < 0:
            raise ValueError(f"the step count must be >= 0, got {s!r}")
        self.validate()
        base, W, r = self.base_lr, self.warmup_steps, self.min_lr_ratio
        if s < W:
            return base * (s + 1) / W
        if self.kind == "constant":
            return base
        q = min(1.0, (s - W) / max(1, self.total_steps - W))
        if self.kind == "linear":
            return base * (r + (1.0 - r) * (1.0 - q))
        return base * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q)))

    __call__ = lr

    # ---- checkpoints: the parameters as plain numbers / strings ----------------------------------------------
    def state(self) -> Dict[str, object]:
        return {"base_lr": self.base_lr, "kind": self.kind, "warmup_steps": self.warmup_steps,
                "total_steps": self.total_steps, "min_lr_ratio": self.min_lr_ratio}

    @classmethod
    def from_state(cls, st: Dict[str, object]) -> "LRSchedule":
        return cls(st["base_lr"], st["kind"], st["warmup_steps"], st["total_steps"], st["min_lr_ratio"])
