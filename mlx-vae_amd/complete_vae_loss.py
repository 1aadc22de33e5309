"""complete_vae_loss on MI355X: same signature, defaults and 12-key result as the reference
(complete_vae_loss.py:7-99); the values come from the fused HIP forward of arcvae_hip."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from arcvae_hip import api


def complete_vae_loss(encoder, decoder, property_predictor, x, conditions, beta: float = 0.4,
                      lambda_prop: float = 0.1, lambda_collapse: float = 0.01, teacher_forcing_ratio: float = 0.9,
                      free_bits: float = 0.5, lambda_mi: float = 0.0, target_mi: float = 4.85,
                      eps: Optional[torch.Tensor] = None, coins: Optional[Sequence[bool]] = None) -> dict:
    """total = recon + beta*kl + collapse + lambda_prop*prop + mi_penalty  (complete_vae_loss.py:76-82).

    `property_predictor`: None (prop_loss is then identically 0, as in the reference, whose predictor branch cannot
    run) or a models.PropertyPredictor -- an extension: prop_loss = mean over B*C
    of (predictor(z) - conditions)^2 on the sampled z.
    `eps` / `coins` are additive hooks to inject the reparameterisation noise and the per-step
    teacher-forcing decisions; by default they are drawn as the reference draws them."""
    hyper = dict(beta=beta, lambda_collapse=lambda_collapse, lambda_mi=lambda_mi, target_mi=target_mi, free_bits=free_bits)
    if property_predictor is not None:
        hyper["lambda_prop"] = lambda_prop
    out = api.loss_forward(encoder, decoder, x, conditions, eps=eps, coins=coins,
                           teacher_forcing_ratio=teacher_forcing_ratio, predictor=property_predictor, **hyper)
    out.pop("pred", None)
    # without a predictor, lambda_prop * 0 == 0: weighted_prop_loss stays the zero the kernel wrote
    return out
