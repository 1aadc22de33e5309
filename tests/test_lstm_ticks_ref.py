"""The per-tick restatement of the encoder LSTM stack (tests/lstm_ticks.py) against torch autograd of the oracle's LSTM in
fp64, the power of its per-tick checker, and the premise of the long-memory setting the GPU tick tests run in.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import lstm_ticks as K
from helpers import DEFAULT, ELEM_ATOL_GRAD, assert_elem, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-vae_amd"))

from arcvae_hip.engine import EncoderBackwardPlan  # noqa: E402


def _autograd(params, cfg, x, dh_top):
    """Encoder stack through O.mlx_lstm in fp64.  The gate pre-activations get a zero offset per (row, tick) through the
    bias operand of the oracle's addmm, so its gradient is dG.  Returns h, c [L,T,B,H], dG [L,T,B,4H], parameter grads."""
    L, H = cfg.L, cfg.H
    B, T = x.shape
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items() if k.startswith("encoder.")}
    offs = [torch.zeros(B * T, 4 * H, dtype=torch.float64, requires_grad=True) for _ in range(L)]
    out = p["encoder.embedding.weight"][torch.as_tensor(x)]
    hs, cs = [], []
    for l in range(L):
        pre = f"encoder.lstm_layer_{l}."
        out, c = O.mlx_lstm(out, p[pre + "Wx"], p[pre + "Wh"], p[pre + "bias"] + offs[l])
        hs.append(out)
        cs.append(c)
    (out[:, -1, :] * torch.as_tensor(dh_top)).sum().backward()
    tb = lambda a: a.detach().numpy().transpose(1, 0, 2)       # [B,T,.] -> [T,B,.]
    dG = np.stack([tb(o.grad.reshape(B, T, 4 * H)) for o in offs])
    grads = {k: v.grad.numpy() if v.grad is not None else np.zeros(v.shape) for k, v in p.items()}   # (T = 1: Wh unused)
    return np.stack([tb(h) for h in hs]), np.stack([tb(c) for c in cs]), dG, grads


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("T", [1, 2, 17])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 5])
def test_restatement_matches_autograd_of_the_oracle_lstm(T, L, B):
    cfg = O.Config(vocab_size=11, embedding_dim=7, hidden_dim=12, latent_dim=4, num_conditions=1, num_layers=L)
    params = O.init_params(cfg, 1234)
    x, _ = O.synthetic_batch(cfg, B, T, 67)
    dh_top = np.random.RandomState(5).standard_normal((B, cfg.H))
    h, c, dG, grads = _autograd(params, cfg, x, dh_top)
    rows = np.arange(B)

    hs, cs, gs = K.run_forward(params, x, rows)
    assert _rel(hs, h) < 1e-12 and _rel(cs, c) < 1e-12
    h1, c1, g1 = K.forward_local(params, x, h, c, rows)
    assert _rel(h1, h) < 1e-12 and _rel(c1, c) < 1e-12 and _rel(g1, gs) < 1e-12
    mine = K.bptt(params, x, h, c, dh_top, rows)
    assert _rel(mine, dG) < 1e-12
    assert K.tick_check(mine, dG, rtol=1e-12, atol_frac=1e-12, floor=0.0).worst <= 1.0
    H = cfg.H
    assert _rel(K.dgo_local(params, x, h, c, dG, dh_top, rows), dG[..., 3 * H:]) < 1e-12
    wg = K.wgrad_from(params, x, h, dG)
    for name, g in wg.items():
        assert _rel(g.numpy(), grads[name]) < 1e-12, name
    # a row subset gives those rows of the whole-batch answer
    sub = np.array([B - 1, 0])
    assert _rel(K.bptt(params, x, h, c, dh_top, sub), dG[:, :, sub]) < 1e-12
    assert _rel(K.forward_local(params, x, h[:, :, sub], c[:, :, sub], sub)[0], h[:, :, sub]) < 1e-12


@pytest.fixture(scope="module")
def default_T128():
    """Default model, T 128, 8 rows of the default batch: fp32 and fp64 free-running forwards and a fixed dh_top."""
    cfg, B, T = DEFAULT, 8, 128
    params, x, _, _, _ = make_case(cfg, B, T, 0.9)
    rows = np.arange(B)
    dh_top = np.random.RandomState(7).standard_normal((B, cfg.H)) * 1e-3
    return cfg, params, x, rows, dh_top


def test_fp32_restatement_passes_the_tick_bar(default_T128):
    """A plain fp32 forward and BPTT (every tick from fp32 states) sits inside the per-tick bar the GPU is held to."""
    cfg, params, x, rows, dh_top = default_T128
    h32, c32, g32 = K.run_forward(params, x, rows, np.float32)
    h, c, g = K.forward_local(params, x, h32, c32, rows)
    for got, ref in ((h32, h), (c32, c), (g32, g)):
        rep = K.tick_check(got, ref)
        assert rep.worst < 0.5 and rep.skipped == 0, str(rep)
    ref = K.bptt(params, x, h32, c32, dh_top, rows, gates=g)
    got = K.bptt(params, x, h32, c32, dh_top, rows, gates=g32, dtype=np.float32)
    rep = K.tick_check(got, ref)
    assert rep.worst < 1.0, str(rep)
    rep = K.tick_check(K.dgo_local(params, x, h32, c32, got, dh_top, rows, gates=g), got[..., 3 * cfg.H:])
    assert rep.worst < 1.0, str(rep)


def test_one_wrong_early_element_fails_the_tick_check_but_not_the_gradient_sums(default_T128):
    """1e-3 relative on one element of dG at t = 3 fails tick_check.  At the default init that tick is far below the
    largest one, so the dWh it implies still passes the element-wise step bar: the gap the tick tests close."""
    cfg, params, x, rows, dh_top = default_T128
    h, c, g = K.run_forward(params, x, rows)
    dG = K.bptt(params, x, h, c, dh_top, rows, gates=g)
    assert K.tick_check(dG, dG).worst == 0.0
    bad = dG.copy()
    i = np.unravel_index(np.argmax(np.abs(bad[0, 3])), bad[0, 3].shape)
    bad[0, 3][i] *= 1.0 + 1e-3
    rep = K.tick_check(bad, dG)
    assert rep.worst > 5.0 and rep.where[:2] == (0, 3), str(rep)
    ok = K.wgrad_from(params, x, h, dG)["encoder.lstm_layer_0.Wh"].numpy()
    off = K.wgrad_from(params, x, h, bad)["encoder.lstm_layer_0.Wh"].numpy()
    assert np.abs(off - ok).max() <= 1e-12 * np.abs(ok).max()     # (below the fp64 rounding of the sum itself)
    assert_elem(off, ok, "dWh_0 from the perturbed dG", ELEM_ATOL_GRAD)


def _last_chunk_share(params, x, h, dG, L, T, fractions):
    """max|part of dWh_l from the last chunk's time range| / max|dWh_l| per layer, for the chunk schedule of `fractions`."""
    _, _, t_lo, t_hi, _, last = EncoderBackwardPlan.chunk_schedule(T, L, fractions)[-1]
    assert last and t_lo == 0
    full = K.wgrad_from(params, x, h, dG)
    part_dG = dG.copy()
    part_dG[:, t_hi:] = 0.0
    part = K.wgrad_from(params, x, h, part_dG)
    return [float(part[f"encoder.lstm_layer_{l}.Wh"].abs().max() / full[f"encoder.lstm_layer_{l}.Wh"].abs().max())
            for l in range(L)], t_hi


def test_long_memory_makes_every_tick_observable(default_T128):
    """Under long_memory every tick's gate-gradient scale is >= 1e-2 of the largest, and the time range of the last chunk of
    both default BPTT chunk schedules carries >= 1e-2 of max|dWh_l|: dropping or misplacing it fails the 1e-4 bar 100x.
    At the default init the same range carries almost nothing (the reason the tick tests run in both settings)."""
    cfg, params, x, rows, dh_top = default_T128
    L, T = cfg.L, x.shape[1]
    lm = K.long_memory(params, cfg)
    assert lm["encoder.lstm_layer_0.bias"].dtype == np.float32 and not np.shares_memory(lm["encoder.lstm_layer_0.Wh"],
                                                                                        params["encoder.lstm_layer_0.Wh"])
    for p, long_mem in ((lm, True), (params, False)):
        h, c, g = K.run_forward(p, x, rows)
        dG = K.bptt(p, x, h, c, dh_top, rows, gates=g)
        s = K.tick_scales(dG)
        if long_mem:
            assert s.min() >= 1e-2 * s.max(), (s.min() / s.max(), np.unravel_index(np.argmin(s), s.shape))
        else:
            assert s.min() < 1e-13 * s.max()
        for fr in (EncoderBackwardPlan.FRACTIONS_PERSISTENT, EncoderBackwardPlan.FRACTIONS_LAUNCHES):
            fractions = tuple(float(f) for f in fr.split(","))
            share, t_hi = _last_chunk_share(p, x, h, dG, L, T, fractions)
            if long_mem:
                assert min(share) >= 1e-2, (fr, t_hi, share)
            else:
                assert max(share) < 1e-6, (fr, t_hi, share)
