"""ARCVAE_LS_ROLES, the form of the layer-split forward sweep (csrc/lstm.hip: lstm_fwd_persist_split): 0 = every store of a tick
ahead of its flag, 1 (default; any non-zero value) = the gate and cell stores behind it.  Both forms run the same
arithmetic in the same order as the one-chain form (ARCVAE_LAYER_SPLIT=0) and must reproduce its h and c bit for bit -- at the
ring's start-up and first wrap (2 slots), with XCDs that hold fewer than 8 rows or none, and over a steady stretch."""
import os
import subprocess
import sys

import pytest
import torch

import arcvae_oracle as O
from helpers import HYPER, build_engine, make_case

pytestmark = pytest.mark.gpu

ROLES = ("0", "1", None)          # both forms, and the unset default
SHAPES = [(64, 1), (64, 2), (64, 3), (64, 5), (1, 5), (9, 7), (40, 9), (63, 33)]


def _cfg():
    return O.Config(vocab_size=60, embedding_dim=32, hidden_dim=256, latent_dim=16, num_conditions=1, num_layers=2)


def _env(split, roles):
    os.environ["ARCVAE_LAYER_SPLIT"] = "1" if split else "0"
    if roles is None:
        os.environ.pop("ARCVAE_LS_ROLES", None)
    else:
        os.environ["ARCVAE_LS_ROLES"] = roles


def _forward(split, roles, B, T, reps=1):
    """hseq / cseq of `reps` steps (the sweep's error word checked after each) in the given form."""
    _env(split, roles)
    params, x, cond, eps, coins = make_case(_cfg(), B, T, 0.6)
    eng, enc, dec = build_engine(_cfg(), params)
    outs = []
    for _ in range(reps):
        eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
        torch.cuda.synchronize()
        eng.check_gates()                                  # raises unless the sweeps' error word is 0
        ws = eng.workspace(B, T, True)
        outs.append((ws.hseq.clone(), ws.cseq.clone()))
    del eng, enc, dec
    torch.cuda.empty_cache()
    return outs


@pytest.fixture(autouse=True)
def _restore_env():
    saved = {k: os.environ.get(k) for k in ("ARCVAE_LAYER_SPLIT", "ARCVAE_LS_ROLES")}
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


_one_chain = {}


def _reference(B, T):
    """The one-chain form's h and c, computed once per shape and shared by the cases."""
    if (B, T) not in _one_chain:
        _one_chain[(B, T)] = _forward(False, None, B, T)[0]
    return _one_chain[(B, T)]


@pytest.mark.parametrize("roles", ROLES)
@pytest.mark.parametrize("B,T", SHAPES)
def test_every_form_matches_the_one_chain_form_bit_for_bit(B, T, roles):
    ref = _reference(B, T)
    new = _forward(True, roles, B, T)[0]
    for name, n, r in (("hseq", new[0], ref[0]), ("cseq", new[1], ref[1])):
        assert torch.isfinite(n).all(), name
        assert torch.equal(n, r), f"{name}: max |diff| {float((n - r).abs().max())}"


@pytest.mark.parametrize("roles", (None, "0"))
def test_forward_activations_are_repeatable(roles):
    outs = _forward(True, roles, 64, 33, reps=6)
    for h, c in outs[1:]:
        assert torch.equal(h, outs[0][0]) and torch.equal(c, outs[0][1])


def _child_priority_off():
    """Run in a fresh process with ARCVAE_STEP_PRIO=0 (read once per process): the default form against the one-chain form."""
    for B, T in ((64, 5), (63, 33)):
        ref = _forward(False, None, B, T)[0]
        new = _forward(True, None, B, T)[0]
        assert torch.equal(new[0], ref[0]) and torch.equal(new[1], ref[1]), (B, T)


def test_default_form_matches_with_priority_off():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, ARCVAE_STEP_PRIO="0")
    env.pop("ARCVAE_LS_ROLES", None)
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.join(root, "mlx-vae_amd"), os.path.join(root, "oracle"), env.get("PYTHONPATH", "")])
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", "import test_layer_split_roles_gpu as t; t._child_priority_off()"]
    subprocess.run(args, env=env, check=True, timeout=120)
