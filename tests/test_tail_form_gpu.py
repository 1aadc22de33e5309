"""The full step in both tail forms of the quiet regime (ARCVAE_TAIL_FORM, engine._encoder_backward_gated): 0 = every
BPTT chunk folds its own token table and main forms the last chunk's; 1 = side accumulates one table and folds it once
with arcvae_table_fold, main forms the last chunk's layer GEMMs behind its own sweep.

Shapes: the smallest that reach the persistent two-chunk gated path (H = 256) -- a full 64-row batch, 5 rows (XCDs without
rows, ragged groups), and a single layer.  Same two criteria and tolerances as test_engine_gpu.py::_check_step."""
import numpy as np
import pytest
import torch

import arcvae_oracle as O
from helpers import ELEM_ATOL_FWD, ELEM_ATOL_GRAD, HYPER, assert_elem, build_engine, make_case, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(2, 64, 20), (2, 5, 12), (1, 16, 9)]       # (L, B, T)
_cases = {}


def _cfg(L):
    return O.Config(vocab_size=60, embedding_dim=32, hidden_dim=256, latent_dim=16, num_conditions=1, num_layers=L)


def _case(L, B, T):
    """Inputs and the fp64 oracle of a shape: computed once, shared, never modified."""
    if (L, B, T) not in _cases:
        cfg = _cfg(L)
        params, x, cond, eps, coins = make_case(cfg, B, T, 0.6)
        vals, grads = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
        _cases[(L, B, T)] = (cfg, params, x, cond, eps, coins, vals, grads)
    return _cases[(L, B, T)]


def _step(L, B, T, form, monkeypatch, skip_f=None):
    import arcvae_hip.engine as E
    monkeypatch.setenv("ARCVAE_TAIL_FORM", form)
    if skip_f is not None:
        monkeypatch.setenv("ARCVAE_DEC_SKIP_F", skip_f)
    cfg, params, x, cond, eps, coins, vals, grads = _case(L, B, T)
    eng, enc, dec = build_engine(cfg, params)
    ws = eng.workspace(B, T)
    plan = E.EncoderBackwardPlan(enc, ws, eng.d)
    assert plan.quiet and len(plan.chunks) == 2 and E._tables_on_main(plan, ws)      # the path under test is the one that runs
    for rep in range(2):                                                              # eager + capture, then a replay
        out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
        torch.cuda.synchronize()
        eng.check_gates()
    return eng, enc, dec, out


def _check(L, B, T, eng, enc, dec, out):
    cfg, params, x, cond, eps, coins, vals, grads = _case(L, B, T)
    ws = eng.workspace(B, T)
    for k in ("total_loss", "recon_loss", "kl_loss", "weighted_kl", "collapse_penalty", "mutual_info", "mi_penalty"):
        assert abs(float(out[k]) - float(vals[k])) <= TOL * max(1.0, abs(float(vals[k]))), k
    for k in ("mu", "logvar", "z"):
        assert rel_err(out[k].cpu().numpy(), vals[k]) < TOL, k
        assert_elem(out[k].cpu().numpy(), vals[k], k, ELEM_ATOL_FWD)
    assert np.array_equal(ws.fed.cpu().numpy(), vals["fed_tokens"]), "fed-back tokens differ"
    logits = eng.gather_logits(ws)
    torch.cuda.synchronize()
    assert rel_err(logits.cpu().numpy(), vals["logits"]) < TOL
    assert_elem(logits.cpu().numpy(), vals["logits"], "logits", ELEM_ATOL_FWD)
    worst = {}
    for name, g in grads.items():
        mod, pname = name.split(".", 1)
        got = (enc if mod == "encoder" else dec).g(pname).cpu().numpy()
        if np.abs(g).max() == 0.0:
            assert np.abs(got).max() == 0.0, f"dead parameter {name} received gradient"
        else:
            worst[name] = rel_err(got, g)
            assert_elem(got, g, "grad " + name, ELEM_ATOL_GRAD)
    bad = {k: v for k, v in worst.items() if v >= TOL}
    assert not bad, bad


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("L,B,T", SHAPES)
def test_step_against_the_oracle_in_both_forms(L, B, T, form, monkeypatch):
    _check(L, B, T, *_step(L, B, T, form, monkeypatch))


def test_step_with_the_full_width_decoder_fold(monkeypatch):
    """ARCVAE_DEC_SKIP_F=0: the decoder's fold gets no dead range (and its layers their full-width products)."""
    L, B, T = SHAPES[0]
    _check(L, B, T, *_step(L, B, T, "1", monkeypatch, skip_f="0"))


@pytest.mark.parametrize("L,B,T", SHAPES)
def test_the_two_forms_agree(L, B, T, monkeypatch):
    g = {}
    for form in ("0", "1"):
        eng, enc, dec, out = _step(L, B, T, form, monkeypatch)
        g[form] = {n: enc.g(n).cpu().numpy().copy() for n in enc.names()}
        g[form].update({"dec." + n: dec.g(n).cpu().numpy().copy() for n in dec.names()})
        del eng, enc, dec
    for n, a in g["1"].items():
        b = g["0"][n]
        if np.abs(b).max() == 0.0:
            assert np.abs(a).max() == 0.0, n
        else:
            print(f"L={L} B={B} T={T} {n}: forms differ by {rel_err(a, b):.2e}")
            assert rel_err(a, b) < 1e-5, n


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("L,B,T", SHAPES)
def test_four_optimizer_steps_in_segments_mode(L, B, T, form, monkeypatch):
    """As test_engine_gpu.py::test_launch_modes_agree_over_several_steps: per-stream captured segments against plain launches."""
    monkeypatch.setenv("ARCVAE_TAIL_FORM", form)
    cfg, params, x, cond, eps, coins, vals, grads = _case(L, B, T)
    runs = {}
    for m in ("eager", "segments"):
        eng, enc, dec = build_engine(cfg, params)
        eng.mode = m
        losses = [float(eng.train_step(x, cond, eps, coins, lr=2e-4, **HYPER)["total_loss"]) for _ in range(4)]
        torch.cuda.synchronize()
        eng.check_gates()
        runs[m] = (losses, enc.flat.cpu().numpy(), dec.flat.cpu().numpy())
    assert np.allclose(runs["segments"][0], runs["eager"][0], rtol=1e-5)
    assert rel_err(runs["segments"][1], runs["eager"][1]) < 1e-5 and rel_err(runs["segments"][2], runs["eager"][2]) < 1e-5
