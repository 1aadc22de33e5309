"""Glue between the reference-named modules and the step engine: engine cache, loss forward,
value_and_grad (the mx.value_and_grad of trainer.py:292) and RNG conventions (Q5/Q18)."""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import SCALAR_KEYS, StepEngine

_ENGINES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def engine_for(encoder, decoder, predictor=None) -> StepEngine:
    """One StepEngine (workspaces, side stream, captured graphs) per (encoder, decoder, predictor): a step captured
    without a predictor is never replayed with one, nor the reverse.  The key of the plain pair is id(decoder).
    A predictor on a pair that runs data-parallel is refused (ValueError)."""
    per_enc = _ENGINES.setdefault(encoder, {})
    if predictor is not None and getattr(per_enc.get(id(decoder)), "dp", None) is not None:
        from .dp import PREDICTOR_DP_UNSUPPORTED
        raise ValueError(PREDICTOR_DP_UNSUPPORTED)
    key = id(decoder) if predictor is None else (id(decoder), id(predictor))
    if key not in per_enc:
        if encoder.dims != decoder.dims:
            raise ValueError("encoder and decoder were built with different dimensions")
        eng = StepEngine(encoder.store, decoder.store, encoder.dims,
                         prop=predictor.store if predictor is not None else None)
        eng.predictor = predictor      # held: its id stays this engine's key while the engine lives
        per_enc[key] = eng
    return per_enc[key]


def enable_data_parallel(encoder, decoder, group=None, predictor=None):
    """Route loss_forward / value_and_grad of this (encoder, decoder) pair through arcvae_hip.dp.EngineDataParallel: every
    call then takes the GLOBAL batch (identical on all ranks), works on this rank's rows and returns the global batch's
    loss scalars; mu / logvar / z in the result are the LOCAL rows'.  torch.distributed must be initialised (one process
    per GPU; backend nccl = RCCL).  Returns the driver (rank, world)."""
    from .dp import PREDICTOR_DP_UNSUPPORTED, EngineDataParallel
    if predictor is not None:
        raise ValueError(PREDICTOR_DP_UNSUPPORTED)
    eng = engine_for(encoder, decoder)
    if getattr(eng, "dp", None) is None:
        eng.dp = EngineDataParallel(eng, group)
    return eng.dp


def data_parallel_of(encoder, decoder):
    """The pair's data-parallel driver (enable_data_parallel), or None: single process."""
    return getattr(engine_for(encoder, decoder), "dp", None)


def attach_ema(encoder, decoder, ema) -> None:
    """Tell the pair's data-parallel driver (if any) about a WeightEMA, so that its state broadcast after a replicated step
    carries the shadows too.  Single process: nothing to do."""
    dp = data_parallel_of(encoder, decoder)
    if dp is not None:
        dp.ema = ema


def last_step_guards(encoder, decoder, predictor=None):
    """The two device error words of the pair's LAST training step (value_and_grad), for a launch that must be skipped
    together with that step's Adam updates -- the weight EMA (arcvae_hip.ema.WeightEMA.update(guards=)), enqueued on the
    current stream right behind the step.

    Also where that launch's order behind EVERY Adam update of the step is settled.  Single process: the decoder's update
    rides on the side stream at the end of the decoder segment; the step's finish on the current stream begins with the
    join of side -- `Gates.join` (side reports on R behind its decoder segment in stream order; a single-chunk sweep joins
    with `wait_stream(side)` in encoder_backward) or `wait_stream(side)` in enqueue_finish -- and the encoder's and the
    predictor's updates are launches of that finish, so whatever follows on the current stream follows all of them.  Data
    parallel: the decoder's update (`_dec_adam_gated`) runs on side behind the decoder bucket's reduce and main's join on R
    covers it in the gated form, but `train_step` itself ends with a collective, not with a join of side: the current
    stream is made to wait for side here, which costs nothing in the step and leaves the drivers untouched."""
    eng = engine_for(encoder, decoder, predictor)
    ws = getattr(eng, "last_train_ws", None)
    if ws is None:
        raise RuntimeError("last_step_guards: no training step has run for this pair")
    if getattr(eng, "dp", None) is not None:
        torch.cuda.current_stream().wait_stream(eng.side)
    return eng.guards(ws)


def draw_coins(T: int, ratio: float) -> np.ndarray:
    """models/decoder.py:180: one np.random.rand() per timestep from the GLOBAL legacy stream, drawn even
    when ratio == 0.0 (validation)."""
    return np.array([np.random.rand() < ratio for _ in range(T)], dtype=np.uint8)


def draw_eps(B: int, Z: int, device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The reference draws eps from MLX's unseeded global RNG (Q18): any N(0,1) draw is 'the same'."""
    return torch.randn(B, Z, device=device, dtype=torch.float32, generator=generator)


def _as_dict(eng: StepEngine, ws, clone: bool, status: bool = False, clip: bool = False,
             rate: bool = False) -> Dict[str, torch.Tensor]:
    sc = ws.scalars.clone()  # 16 floats: always detach from the static buffer the next call overwrites
    out = {k: sc[i] for i, k in enumerate(SCALAR_KEYS)}
    if status:   # [total_loss, step status]: ONE D2H read gives the trainer the loss and "stream order was lost"
        out["loss_and_status"] = sc[::15]     # elements 0 and 15 of the 16
    if clip:     # the global-norm clip: pre-clip norm and applied scale; [loss, status, norm] for the same single read
        out["grad_norm"], out["clip_scale"] = sc[11], sc[12]
        out["loss_status_norm"] = torch.stack((sc[0], sc[15], sc[11]))
    if rate:     # device-rate mode: the rate the encoder's update applied
        out["lr"] = sc[13]
    for k in ("mu", "logvar", "z"):
        t = getattr(ws, k)
        out[k] = t.clone() if clone else t
    return out


def loss_forward(encoder, decoder, x, conditions, eps=None, coins=None, teacher_forcing_ratio: float = 0.9,
                 predictor=None, **hyper) -> Dict[str, torch.Tensor]:
    """predictor (models.PropertyPredictor, optional): also prop_loss / weighted_prop_loss and "pred"; hyper must then
    include lambda_prop (ValueError otherwise)."""
    eng = engine_for(encoder, decoder, predictor)
    B, T = int(x.shape[0]), int(x.shape[1])
    if coins is None:
        coins = draw_coins(T, teacher_forcing_ratio)
    if eps is None:
        eps = draw_eps(B, encoder.latent_dim, encoder.store.device)
    dp = getattr(eng, "dp", None)
    if dp is not None:       # N ranks: this rank's rows, one all-reduce of the partial sums, the global batch's scalars
        x, conditions = _dev_batch(eng, x, conditions)
        return _as_dict(eng, dp.forward_loss(x, conditions, _local_eps(dp, eps, B), coins, **hyper), clone=True)
    eng.forward_loss(x, conditions, eps, coins, **hyper)
    out = _as_dict(eng, eng.workspace(B, T, train=False), clone=True)
    if predictor is not None:
        out["pred"] = eng.workspace(B, T, train=False).pred.clone()
    return out


def value_and_grad(encoder, decoder, x, conditions, eps=None, coins=None, teacher_forcing_ratio: float = 0.9,
                   lr: Optional[float] = None, predictor=None, grad_clip: Optional[float] = None, lr_device: bool = False,
                   **hyper):
    """(loss dict, (encoder grad tree, decoder grad tree)); with `lr` given the two Adam updates are applied
    in the same captured step (trainer.py:305-333).  With a predictor (hyper must include lambda_prop, ValueError
    otherwise): (loss dict, (encoder, decoder, predictor grad trees)) and three Adam updates.
    grad_clip (opt-in, needs lr): the updates apply the global-norm clip with max_norm = grad_clip --
    the reference's intended `_clip_gradients` rule over every gradient of the step.  The returned gradient trees stay the
    UNCLIPPED ones; the loss dict also holds "grad_norm" (pre-clip), "clip_scale" and "loss_status_norm".
    lr_device (opt-in, needs lr): lr (finite, >= 0) travels as a device word, so that a rate that changes
    from step to step -- a warmup or decay schedule -- replays the same captured step; the loss dict also holds "lr", the rate
    the update applied."""
    if grad_clip is not None and lr is None:
        raise ValueError("grad_clip needs lr: without an update there is nothing to clip")
    if lr_device and lr is None:
        raise ValueError("lr_device needs lr: without an update no rate is applied")
    from .engine import check_clip_norm
    clip = check_clip_norm(grad_clip)
    eng = engine_for(encoder, decoder, predictor)
    B, T = int(x.shape[0]), int(x.shape[1])
    if coins is None:
        coins = draw_coins(T, teacher_forcing_ratio)
    if eps is None:
        eps = draw_eps(B, encoder.latent_dim, encoder.store.device)
    dp = getattr(eng, "dp", None)
    if dp is not None:
        if lr is None:
            raise ValueError("the data-parallel step applies both Adam updates: pass lr")
        x, conditions = _dev_batch(eng, x, conditions)
        ws = dp.train_step(x, conditions, _local_eps(dp, eps, B), coins, lr, clip_norm=clip, lr_device=lr_device,
                           **hyper)
        eng.last_train_ws = ws
        return _as_dict(eng, ws, clone=False, status=True, clip=clip is not None, rate=lr_device), (encoder.gradients(), decoder.gradients())
    eng.train_step(x, conditions, eps, coins, lr=lr if lr is not None else 0.0, update=lr is not None, clip_norm=clip,
                   lr_device=lr_device, **hyper)
    ws = eng.workspace(B, T, train=True)
    eng.last_train_ws = ws       # (last_step_guards)
    out = _as_dict(eng, ws, clone=False, status=True, clip=clip is not None, rate=lr_device)
    if predictor is not None:
        return out, (encoder.gradients(), decoder.gradients(), predictor.gradients())
    return out, (encoder.gradients(), decoder.gradients())


def _dev_batch(eng: StepEngine, x, conditions):
    """Device-resident, contiguous global batch in the workspace's dtypes (what EngineDataParallel slices rows from)."""
    from .module import as_f32, as_tokens
    xt = as_tokens(x, eng.device)
    return xt, as_f32(conditions, eng.device).reshape(xt.shape[0], eng.d.C)


def _local_eps(dp, eps, B: int):
    """eps of the GLOBAL batch ([B, Z], sliced by the driver) -- an own draw per rank when none was injected."""
    if eps is None:
        return draw_eps(B, dp.eng.d.Z, dp.eng.device)
    from .module import as_f32
    return as_f32(eps, dp.eng.device)
