"""NumPy restatement of the weight EMA (csrc/ema.hip, arcvae_hip/ema.py): the update in the library's expression order, and
the decay warm-up.  The GPU tests hold the kernel to `update32` bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32


def omd32(one_minus_decay: float) -> np.float32:
    """The fp32 weight the library uses: the double 1 - decay rounded once."""
    return F(one_minus_decay)


def update32(e, p, omd) -> np.ndarray:
    """e + fl(omd * fl(p - e)): three fp32 roundings, no FMA (NumPy evaluates each operation on float32 arrays in float32)."""
    e = np.asarray(e, dtype=F)
    p = np.asarray(p, dtype=F)
    d = p - e
    s = F(omd) * d
    return e + s


def update64(e, p, omd) -> np.ndarray:
    """The same recursion in float64 (on the same fp32-rounded omd)."""
    e = np.asarray(e, dtype=np.float64)
    return e + np.float64(F(omd)) * (np.asarray(p, dtype=np.float64) - e)


def decay_at(decay: float, warmup: bool, t: int) -> float:
    """The decay of the update that follows t earlier ones."""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def replay(e0, weights, decay: float, warmup: bool, t0: int = 0) -> np.ndarray:
    """The shadow after one update per entry of `weights` (the weights read back after each step), starting from e0 with t0
    updates done."""
    e = np.asarray(e0, dtype=F).copy()
    for k, p in enumerate(weights):
        e = update32(e, p, omd32(1.0 - decay_at(decay, warmup, t0 + k)))
    return e
