"""Exponential moving average of the weights (an extension; csrc/ema.hip).

A WeightEMA owns one fp32 shadow buffer per ParamStore and keeps it as  e <- e + (1 - decay) * (p - e)  after every training
step: ONE launch over all stores, outside the captured step, on the stream the step was enqueued on.  The averaged weights are
read in two ways only: `applied()` exchanges `store.flat` with the shadow in place for the duration of a `with` block (every
consumer of the store follows, as after load_checkpoint), and the sampler's `load_from_decoder(decoder, ema=)` copies the
decoder's shadow.  The shadow is fp32 and so is the arithmetic: once (1 - decay) * |p - e| falls under half an ulp of e the
average stops moving (DESIGN.md section 10 states the band).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict

import torch

from . import _lib
from ._lib import call, ptr_array, stream_ptr
from .store import ParamStore

NO_GUARDS = (C.c_void_p(0), C.c_void_p(0))


def check_decay(decay) -> float:
    """decay as a float in (0, 1); ValueError otherwise (bool, str, NaN, 0, 1 included)."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 < float(decay) < 1.0):
        raise ValueError(f"ema decay must be a number with 0 < decay < 1, got {decay!r}")
    return float(decay)


class WeightEMA:
    def __init__(self, stores: Dict[str, ParamStore], decay: float, warmup: bool = False):
        self.decay = check_decay(decay)
        self.warmup = bool(warmup)
        if len(stores) > _lib.EMA_MAX_SEGMENTS:
            raise ValueError(f"at most {_lib.EMA_MAX_SEGMENTS} stores per WeightEMA, got {len(stores)}")
        self.stores = dict(stores)
        self._shadow = {}
        for name, st in self.stores.items():
            sh = torch.empty_like(st.flat)
            sh.copy_(st.flat)
            self._shadow[name] = sh
        self.num_updates = 0
        self._applied = False
        # the launch arguments never change: the flat buffers are overwritten in place, never re-allocated
        flats = [st.flat for st in self.stores.values()]
        shadows = [self._shadow[k] for k in self.stores]
        self._n = (C.c_long * max(1, len(flats)))(*[int(f.numel()) for f in flats])
        self._flat_ptrs, self._keep_f = ptr_array(flats) if flats else (None, None)
        self._shadow_ptrs, self._keep_s = ptr_array(shadows) if flats else (None, None)

    # ---- schedule -------------------------------------------------------------------------------------------------
    def decay_at(self, t: int) -> float:
        """The decay of the update that follows `t` earlier ones: min(decay, (1 + t) / (10 + t)) with the warm-up on (the first
        updates then do not average in the initialisation: decay_at(0) = 0.1), else `decay`."""
        if self.warmup:
            return min(self.decay, (1 + t) / (10 + t))
        return self.decay

    # ---- the two launches -----------------------------------------------------------------------------------------
    def update(self, guards=NO_GUARDS) -> None:
        """shadow <- shadow + (1 - decay_at(num_updates)) * (flat - shadow): one launch on the current stream.  guards: two
        device error words (StepEngine.guards); the kernel writes nothing when either is set, as the Adam updates do."""
        if self._applied:
            raise RuntimeError("WeightEMA.update() inside applied(): store.flat holds the averaged weights there")
        omd = 1.0 - self.decay_at(self.num_updates)      # Python floats: formed in double, rounded to fp32 once by the library
        if self.stores:
            call("arcvae_ema_update", self._shadow_ptrs, self._flat_ptrs, self._n, len(self.stores), omd, guards[0], guards[1],
                 stream_ptr())
        self.num_updates += 1

    def _swap(self) -> None:
        if self.stores:
            call("arcvae_ema_swap", self._flat_ptrs, self._shadow_ptrs, self._n, len(self.stores), stream_ptr())

    @contextlib.contextmanager
    def applied(self):
        """Inside the block `store.flat` holds the averaged weights and the shadow the raw ones (an exact in-place exchange, one
        launch on entry and one on exit, exception or not).  Not re-entrant."""
        if self._applied:
            raise RuntimeError("WeightEMA.applied() is not re-entrant")
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._swap()
            self._applied = False

    # ---- access / state -------------------------------------------------------------------------------------------
    def shadow(self, name: str) -> torch.Tensor:
        """The flat shadow buffer of store `name` (the layout of store.flat)."""
        return self._shadow[name]

    def shadow_view(self, name: str, param: str) -> torch.Tensor:
        st = self.stores[name]
        return st._view(self._shadow[name], param)

    def reset(self) -> None:
        """Shadows <- the stores' current weights, num_updates <- 0."""
        if self._applied:
            raise RuntimeError("WeightEMA.reset() inside applied()")
        for name, st in self.stores.items():
            self._shadow[name].copy_(st.flat)
        self.num_updates = 0

    def state(self) -> dict:
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates}

    def load_state(self, state: dict) -> None:
        self.decay, self.warmup, self.num_updates = check_decay(state["decay"]), bool(state["warmup"]), int(state["num_updates"])
