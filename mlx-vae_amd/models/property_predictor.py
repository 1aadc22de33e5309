"""PropertyPredictor on MI355X: the head the reference's interface expects (complete_vae_loss(encoder, decoder,
property_predictor, ...), ARCVAETrainerWithLoss(property_predictor=...)) but never builds (its train.py passes None, and
its loss branch cannot run).  Defined here as an extension:

    pred = fc2(tanh(fc1(z)))      fc1: Linear(latent_dim -> hidden_dim), fc2: Linear(hidden_dim -> num_properties)

initialised like MLX nn.Linear (uniform +-1/sqrt(fan_in)), computed by the HIP kernels of csrc/prop.hip and trained with
its own un-bias-corrected Adam inside the captured step (arcvae_hip.engine)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import torch

from arcvae_hip import _lib
from arcvae_hip._lib import call, ptr, stream_ptr
from arcvae_hip.module import as_f32, resolve_device
from arcvae_hip.store import ParamStore

MAX_HIDDEN = 256
MAX_PROPERTIES = 8


def predictor_shapes(latent_dim: int, num_properties: int, hidden_dim: int) -> "OrderedDict[str, tuple]":
    s: "OrderedDict[str, tuple]" = OrderedDict()
    s["fc1.weight"] = (hidden_dim, latent_dim)
    s["fc1.bias"] = (hidden_dim,)
    s["fc2.weight"] = (num_properties, hidden_dim)
    s["fc2.bias"] = (num_properties,)
    return s


class PropertyPredictor:
    def __init__(self, latent_dim: int, num_properties: int, hidden_dim: int = 64, device=None,
                 generator: Optional[torch.Generator] = None):
        if not (1 <= int(hidden_dim) <= MAX_HIDDEN):
            raise ValueError(f"hidden_dim must be in [1, {MAX_HIDDEN}], got {hidden_dim}")
        if not (1 <= int(num_properties) <= MAX_PROPERTIES):
            raise ValueError(f"num_properties must be in [1, {MAX_PROPERTIES}], got {num_properties}")
        if not (1 <= int(latent_dim) <= 512):
            raise ValueError(f"latent_dim must be in [1, 512] for the predictor kernels, got {latent_dim}")
        self.latent_dim, self.num_properties, self.hidden_dim = int(latent_dim), int(num_properties), int(hidden_dim)
        self.store = ParamStore(predictor_shapes(self.latent_dim, self.num_properties, self.hidden_dim),
                                resolve_device(device))
        self.store.init_mlx_like(self.hidden_dim, generator or torch.Generator().manual_seed(torch.seed() % (2 ** 31)))
        self._ws: Dict[int, torch.Tensor] = {}

    def __call__(self, z) -> torch.Tensor:
        """z [B, latent_dim] -> predicted properties [B, num_properties] (one forward-only launch)."""
        dev = self.store.device
        zt = as_f32(z, dev)
        if zt.dim() != 2 or zt.shape[1] != self.latent_dim:
            raise ValueError(f"z must be [B, {self.latent_dim}], got {tuple(zt.shape)}")
        pred = torch.empty(zt.shape[0], self.num_properties, dtype=torch.float32, device=dev)
        st = self.store
        call("arcvae_prop_forward", ptr(zt), C.c_void_p(0), ptr(st.p("fc1.weight")), ptr(st.p("fc1.bias")),
             ptr(st.p("fc2.weight")), ptr(st.p("fc2.bias")), C.c_void_p(0), ptr(pred), C.c_void_p(0), C.c_void_p(0),
             C.c_long(0), int(zt.shape[0]), self.latent_dim, self.num_properties, self.hidden_dim, stream_ptr())
        return pred

    # MLX-style trees (as the encoder / decoder) ----------------------------------------------------------------------
    def parameters(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return self.store.tree("flat")

    def gradients(self) -> Dict[str, Dict[str, torch.Tensor]]:
        return self.store.tree("grad")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return self.store.state_dict()

    def load_state_dict(self, sd, prefix: str = "") -> None:
        self.store.load_state_dict(sd, prefix)

    @property
    def fc1(self):
        return _Linear(self.store, "fc1")

    @property
    def fc2(self):
        return _Linear(self.store, "fc2")


class _Linear:
    def __init__(self, store: ParamStore, name: str):
        self.weight, self.bias = store.p(f"{name}.weight"), store.p(f"{name}.bias")


def ws_floats(B: int, latent_dim: int, num_properties: int, hidden_dim: int) -> int:
    """Size of the partials workspace of the predictor kernels (arcvae_prop_ws_floats)."""
    n = C.c_long(0)
    _lib.check(_lib.load().arcvae_prop_ws_floats(B, latent_dim, num_properties, hidden_dim, C.byref(n)),
               "arcvae_prop_ws_floats")
    return n.value
