"""The layer-split form of the persistent forward sweep (csrc/lstm.hip: lstm_fwd_persist_split, lstm_fwd_persist_kernel with
LS = 1): fp32, H 256, L 2, at most 8 rows per XCD.  The two layers run as two chains with their own flag lines; the
cross-layer product Wx1 h0_t is handed to the layer-1 waves as unreduced accumulators, so the split form executes the same
instructions in the same order as the one-chain form and must reproduce it bit for bit (ARCVAE_LAYER_SPLIT=0 forces the
one-chain form, which the oracle tests of test_engine_gpu.py / test_golden_gpu.py pin)."""
import numpy as np
import pytest
import torch

import arcvae_oracle as O
from helpers import HYPER, build_engine, make_case

pytestmark = pytest.mark.gpu


def _step(monkeypatch, split, cfg, B, T, reps=1):
    monkeypatch.setenv("ARCVAE_LAYER_SPLIT", "1" if split else "0")
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.6)
    eng, enc, dec = build_engine(cfg, params)
    outs = []
    for _ in range(reps):
        out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
        torch.cuda.synchronize()
        eng.check_gates()
        ws = eng.workspace(B, T, True)
        outs.append(dict(hseq=ws.hseq.clone(), cseq=ws.cseq.clone(),   # (gseq: the BPTT overwrites it with gate gradients)
                         loss=float(out["total_loss"]), mu=out["mu"].cpu().numpy().copy(),
                         gWh0=enc.g("lstm_layer_0.Wh").clone(), gWx1=enc.g("lstm_layer_1.Wx").clone()))
    del eng, enc, dec
    torch.cuda.empty_cache()
    return outs


def _cfg():
    return O.Config(vocab_size=60, embedding_dim=32, hidden_dim=256, latent_dim=16, num_conditions=1, num_layers=2)


@pytest.mark.parametrize("B,T", [(64, 128), (64, 1), (64, 2), (64, 3), (1, 5), (9, 7), (40, 9), (63, 33)])
def test_layer_split_forward_matches_one_chain_form(B, T, monkeypatch):
    """Default shape, short T (ring and lead start-up), fewer than 8 rows per XCD: forward activations (h, c) bit-identical to the
    one-chain form, and so the whole step's loss, latent means and encoder gradients up to the split-K atomics' rounding."""
    cfg = _cfg()
    new = _step(monkeypatch, True, cfg, B, T)[0]
    old = _step(monkeypatch, False, cfg, B, T)[0]
    for k in ("hseq", "cseq"):
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(new[k], old[k]), f"{k}: max |diff| {float((new[k] - old[k]).abs().max())}"
    assert np.isfinite(new["loss"]) and abs(new["loss"] - old["loss"]) <= 1e-6 * max(1.0, abs(old["loss"]))
    assert np.allclose(new["mu"], old["mu"], rtol=1e-6, atol=1e-7)
    for k in ("gWh0", "gWx1"):
        dev = float((new[k] - old[k]).abs().max() / old[k].abs().max().clamp_min(1e-30))
        assert dev < 2e-5, (k, dev)


def test_layer_split_step_is_repeatable(monkeypatch):
    """The same default-shape step run repeatedly gives bit-identical forward activations (the sweep has no atomics)."""
    outs = _step(monkeypatch, True, _cfg(), 64, 128, reps=6)
    for o in outs[1:]:
        for k in ("hseq", "cseq"):
            assert torch.equal(o[k], outs[0][k]), k
