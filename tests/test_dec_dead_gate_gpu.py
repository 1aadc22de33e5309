"""The dense decoder's layers l >= 1 without their dead forget gate (csrc/decoder.hip dead_gate_skip, csrc/gemm.hip gaps).

Every decoder LSTM is called with zero state, so c = i * g and the forget gate reaches no result.  With H % 64 == 0 the
layer GEMMs step over the forget quarter [H, 2H) of their 4H-wide operands as a gap: it is neither computed, written nor
read; `gpre` and `ddG` keep their [R, 4H] layout.  The bias gradients ride in the weight-gradient launches.

Reference values: the fp64 oracle the other decoder tests use, at their bar -- norm-wise 1e-4 and the element-wise
criterion of tests/helpers.py; the bf16 throughput mode at the bar tests/test_bf16_mode_gpu.py states for it."""
import numpy as np
import pytest
import torch

import arcvae_oracle as O
from helpers import ELEM_ATOL_FWD, ELEM_ATOL_GRAD, HYPER, TINY, assert_elem, build_engine, make_case, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF16_LOSS_RTOL, BF16_ACT_TOL, BF16_GRAD_RTOL, BF16_GRAD_COS = 2e-2, 5e-2, 8e-2, 0.995   # tests/test_bf16_mode_gpu.py
NAN = float("nan")

_ORACLE = {}


def _cfg(H, L, V, E=16, Z=8, C=1):
    return O.Config(vocab_size=V, embedding_dim=E, hidden_dim=H, latent_dim=Z, num_conditions=C, num_layers=L)


def _case(cfg, B, T, tf):
    """Inputs and the fp64 oracle of a case, computed once per session and never written to."""
    key = (cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L, B, T, tf)
    if key not in _ORACLE:
        params, x, cond, eps, coins = make_case(cfg, B, T, tf)
        vals, grads = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
        _ORACLE[key] = (params, x, cond, eps, coins, vals, grads)
    return _ORACLE[key]


def _quarters(t, H):
    """[..., R, 4H] -> (forget quarter, the three live quarters)."""
    v = t.reshape(-1, 4, H)
    return v[:, 1], v[:, [0, 2, 3]]


def _check_grads_fp32(store_of, grads, only=None):
    bad = {}
    for name, g in grads.items():
        mod, pname = name.split(".", 1)
        if only is not None and mod != only:
            continue
        got = store_of(mod).g(pname).cpu().numpy()
        if np.abs(g).max() == 0.0:
            assert np.abs(got).max() == 0.0, f"dead parameter {name} received gradient"
        elif rel_err(got, g) >= TOL:
            bad[name] = rel_err(got, g)
        else:
            assert_elem(got, g, "grad " + name, ELEM_ATOL_GRAD)
    assert not bad, bad


def _check_grads_bf16(store_of, grads):
    for name, g in grads.items():
        mod, pname = name.split(".", 1)
        a = store_of(mod).g(pname).cpu().numpy().astype(np.float64)
        g = np.asarray(g, dtype=np.float64)
        if not np.any(g):
            assert not np.any(a), name
            continue
        cos = float((a * g).sum() / (np.linalg.norm(a) * np.linalg.norm(g)))
        assert rel_err(a, g) < BF16_GRAD_RTOL and cos > BF16_GRAD_COS, (name, rel_err(a, g), cos)


def _forget_rows(dec, L, H):
    """The forget-gate rows of every dWx_l and entries of every dbias_l, l >= 1, as one flat tensor."""
    parts = []
    for l in range(1, L):
        parts.append(dec.g(f"lstm_layer_{l}.Wx")[H:2 * H].reshape(-1))
        parts.append(dec.g(f"lstm_layer_{l}.bias")[H:2 * H].reshape(-1))
    return torch.cat(parts)


# ---- 1. nothing reads or writes the dead quarter: the whole step with NaN in gpre and ddG ---------------------------------------
STEP_SHAPES = [(64, 2, 3, 11), (128, 3, 5, 13)]     # (H, L, B, V): R = 33 ragged; R = 65, one row past a tile, two gapped layers


def _nan_step(cfg, B, T, mode, monkeypatch):
    from arcvae_hip.engine import StepEngine
    bf16 = mode == "bf16"
    if not bf16:
        monkeypatch.setenv("ARCVAE_DEC_SPLIT3", "1" if mode == "split3" else "0")
    params, x, cond, eps, coins, vals, grads = _case(cfg, B, T, 1.0 if bf16 else 0.6)
    eng, enc, dec = build_engine(cfg, params)
    if bf16:
        eng = StepEngine(enc, dec, eng.d, precision="bf16")
    ws = eng.workspace(B, T)
    assert getattr(ws, "dense_ws", None) is None            # the layers run in arcvae_dec_forward_dense / _backward_dense
    assert bf16 or ws.dec_split3 == (mode == "split3")
    ws.gpre.fill_(NAN)
    ws.ddG.fill_(NAN)
    out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
    torch.cuda.synchronize()
    assert eng.workspace(B, T) is ws
    H, store_of = cfg.H, (lambda mod: enc if mod == "encoder" else dec)
    for t in (ws.hact, ws.logits, ws.lse, dec.grad):
        assert bool(torch.isfinite(t).all())
    for name, t in (("gpre", ws.gpre[:cfg.L - 1]), ("ddG", ws.ddG)):
        dead, live = _quarters(t, H)
        assert bool(torch.isnan(dead).all()), f"{name}: the forget quarter was written"
        assert bool(torch.isfinite(live).all()), name
    scalars = ("total_loss", "recon_loss", "kl_loss", "weighted_kl", "collapse_penalty", "mutual_info", "mi_penalty")
    logits = eng.gather_logits(ws)
    torch.cuda.synchronize()
    if bf16:
        for k in scalars:
            assert abs(float(out[k]) - float(vals[k])) <= BF16_LOSS_RTOL * max(1.0, abs(float(vals[k]))), k
        # (the mode's activation bar: operands rounded to 8 significant bits through L layer products and fc_out)
        ref = np.asarray(vals["logits"], dtype=np.float64)
        assert np.abs(logits.cpu().numpy() - ref).max() <= BF16_ACT_TOL * np.abs(ref).max()
        _check_grads_bf16(store_of, grads)
    else:
        for k in scalars:
            assert abs(float(out[k]) - float(vals[k])) <= TOL * max(1.0, abs(float(vals[k]))), k
        assert np.array_equal(ws.fed.cpu().numpy(), vals["fed_tokens"])
        assert rel_err(logits.cpu().numpy(), vals["logits"]) < TOL
        assert_elem(logits.cpu().numpy(), vals["logits"], "logits", ELEM_ATOL_FWD)
        _check_grads_fp32(store_of, grads)
    # 2. (zeroed buffers) the forget-gate parameter gradients were never touched
    assert bool((_forget_rows(dec, cfg.L, H) == 0).all())


@pytest.mark.parametrize("mode", ["split3", "f32", "bf16"])
@pytest.mark.parametrize("H,L,B,V", STEP_SHAPES)
def test_step_leaves_the_forget_quarter_alone(H, L, B, V, mode, monkeypatch):
    _nan_step(_cfg(H, L, V), B, 7, mode, monkeypatch)


def test_default_shape_leaves_the_forget_quarter_alone(monkeypatch):
    _nan_step(O.Config(), 64, 128, "split3", monkeypatch)   # H 256, L 2, B 64, V 80: R = 5120, the three-piece kernels


# ---- the decoder alone, driven through the engine's own call sites ---------------------------------------------------------------
class _Dec:
    """Decoder parameters and a workspace without an engine (so H = 48, which the encoder's kernels do not take, can be run):
    forward, teacher-forcing walk, backward on the current stream."""

    def __init__(self, cfg, B, T, split3=False, bf16=False, tf=0.6):
        from arcvae_hip.engine import ModelDims, Workspace
        from arcvae_hip.store import ParamStore, decoder_shapes
        self.cfg, self.B, self.T = cfg, B, T
        self.params, x, cond, _eps, coins, self.vals, self.grads = _case(cfg, B, T, tf)
        self.d = ModelDims(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L)
        self.dec = ParamStore(decoder_shapes(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L), "cuda")
        self.dec.load_state_dict(self.params, prefix="decoder.")
        ws = self.ws = Workspace(self.d, B, T, "cuda", True)
        ws.x.copy_(torch.as_tensor(np.asarray(x), dtype=torch.int32))
        ws.cond.copy_(torch.as_tensor(np.asarray(cond), dtype=torch.float32).reshape(B, cfg.C))
        ws.coins.copy_(torch.as_tensor(np.asarray(coins).astype(np.uint8)))
        ws.dec_split3, ws.bf16_parts, ws.dense_ws = split3, (2 if bf16 else 0), None

    def run(self, fill=0.0, nan=True):
        import arcvae_hip.engine as E
        ws = self.ws
        self.dec.grad.fill_(fill)
        if nan:
            ws.gpre.fill_(NAN)
            ws.ddG.fill_(NAN)
        E.decoder_forward_dense(self.dec, ws, self.d, keep_gpre=True)
        E.decoder_chain(ws, self.d)
        E.decoder_backward(self.dec, ws, self.d, 1.0 / (self.B * self.T))
        torch.cuda.synchronize()
        return self

    def dh0(self):
        return self.ws.ddh[(self.cfg.L - 1) % 2]

    def check_oracle(self):
        ws, vals, V = self.ws, self.vals, self.cfg.V
        recon = float(ws.rowloss.sum()) / (self.B * self.T)
        assert abs(recon - float(vals["recon_loss"])) <= TOL * max(1.0, abs(float(vals["recon_loss"])))
        fed = ws.fed.cpu().numpy()
        assert np.array_equal(fed, vals["fed_tokens"])
        dense = ws.logits.cpu().numpy().reshape(self.B, V, V)
        logits = dense[np.arange(self.B)[:, None], fed]
        assert rel_err(logits, vals["logits"]) < TOL
        assert_elem(logits, vals["logits"], "logits", ELEM_ATOL_FWD)
        _check_grads_fp32(lambda mod: self.dec, self.grads, only="decoder")


# ---- 2. "+=": forget-gate parameter gradients keep what the buffers held ----------------------------------------------------------
@pytest.mark.parametrize("split3", [True, False])
@pytest.mark.parametrize("H,L,B,V", STEP_SHAPES + [(64, 2, 9, 40)])      # (R = 360: the tile kernels instead of the skinny one)
def test_forget_gate_parameter_gradients_are_not_touched(H, L, B, V, split3):
    run = _Dec(_cfg(H, L, V), B, 7, split3=split3)
    run.run(fill=0.0)
    assert bool((_forget_rows(run.dec, L, H) == 0).all())
    run.check_oracle()
    live = run.dec.grad.clone()
    run.run(fill=0.375)
    assert bool((_forget_rows(run.dec, L, H) == 0.375).all())
    # ... as does every entry the first backward left at zero; everything else is "constant + gradient": every add into an
    # entry below 2 rounds by at most 2^-24, and no entry receives more than 64 adds (K slices, table folds)
    touched = (live != 0)
    assert bool((run.dec.grad[~touched] == 0.375).all())
    assert float(live.abs().max()) < 1.5
    assert bool(((run.dec.grad - 0.375 - live).abs()[touched] <= 64 * 2.0 ** -24).all())


# ---- 3. same arithmetic where it must be the same ----------------------------------------------------------------------------------
@pytest.mark.parametrize("split3", [True, False])
@pytest.mark.parametrize("H,L,B,V", STEP_SHAPES + [(64, 2, 9, 40), (128, 2, 24, 20)])
def test_gapped_path_equals_the_full_width_path(H, L, B, V, split3, monkeypatch):
    run = _Dec(_cfg(H, L, V), B, 7, split3=split3)
    ws = run.ws
    monkeypatch.setenv("ARCVAE_DEC_SKIP_F", "0")
    run.run(nan=False)
    assert bool((_quarters(ws.ddG, H)[0] == 0).all())       # the full-width path writes its zeros
    run.check_oracle()
    full = {k: t.clone() for k, t in (("hact", ws.hact), ("logits", ws.logits), ("lse", ws.lse), ("nxt", ws.nxt), ("dh0", run.dh0()))}
    full_grad = run.dec.grad.clone()
    monkeypatch.delenv("ARCVAE_DEC_SKIP_F")
    run.run()
    assert bool(torch.isnan(_quarters(ws.ddG, H)[0]).all())
    run.check_oracle()
    for k, t in (("hact", ws.hact), ("logits", ws.logits), ("lse", ws.lse), ("nxt", ws.nxt), ("dh0", run.dh0())):
        assert bool((t == full[k]).all()), k                # element for element (== also accepts a signed zero)
    worst = {}
    for name in run.dec.names():
        a, b = run.dec.g(name), run.dec._view(full_grad, name)
        if bool((b != 0).any()):
            worst[name] = float((a - b).abs().max() / b.abs().max())
    print(f"H={H} L={L} R={B * V} split3={split3}: largest relative difference of a gradient between the two paths: "
          f"{max(worst.values()):.2e} ({max(worst, key=worst.get)})")


# ---- 4. fallback: H % 64 != 0 keeps the full-width path ---------------------------------------------------------------------------
@pytest.mark.parametrize("split3", [True, False])
def test_hidden_size_48_takes_the_full_width_path(split3):
    H, L = 48, 2
    run = _Dec(_cfg(H, L, 13), 5, 7, split3=split3).run()
    dead, live = _quarters(run.ws.ddG, H)
    assert bool((dead == 0).all()) and bool(torch.isfinite(live).all())
    assert bool(torch.isfinite(run.ws.gpre[:L - 1]).all())
    run.check_oracle()


# ---- 5. the fused forward kernel (sampler, loss-only forward) -----------------------------------------------------------------------
def _forward_only(cfg, B, keep_gpre):
    import arcvae_hip.engine as E
    from arcvae_hip.engine import ModelDims, Workspace
    from arcvae_hip.store import ParamStore, decoder_shapes
    d = ModelDims(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L)
    dec = ParamStore(decoder_shapes(cfg.V, cfg.E, cfg.H, cfg.Z, cfg.C, cfg.L), "cuda")
    dec.load_state_dict(O.init_params(cfg, 1234), prefix="decoder.")
    ws = Workspace(d, B, 4, "cuda", False)
    ws.cond.copy_(torch.as_tensor(np.random.RandomState(9).standard_normal((B, cfg.C)).astype(np.float32)))
    ws.dec_split3, ws.bf16_parts, ws.dense_ws = False, 0, None
    ws.hact.fill_(NAN)
    E.decoder_forward_dense(dec, ws, d, keep_gpre=keep_gpre)
    torch.cuda.synchronize()
    return ws.hact, ws.logits, ws.nxt


@pytest.mark.parametrize("H,L,B,V", [(64, 2, 64, 64), (64, 3, 66, 64), (256, 2, 1024, 80)])   # R = 4096, 4224 (the R >= 4096 switch); the sampler's batch
def test_fused_forward_kernel_equals_the_two_kernel_path(H, L, B, V, monkeypatch):
    cfg = _cfg(H, L, V, E=32)
    ref = [t.clone() for t in _forward_only(cfg, B, True)]
    assert bool(torch.isfinite(ref[0]).all())
    for skip_f in ("1", "0"):                                # three gates per unit / the four-gate kernel
        monkeypatch.setenv("ARCVAE_DEC_SKIP_F", skip_f)
        got = _forward_only(cfg, B, False)
        for name, a, b in zip(("hact", "logits", "nxt"), got, ref):
            assert bool((a == b).all()), (name, skip_f)


def test_greedy_tokens_do_not_depend_on_the_switch(monkeypatch):
    from models.vae import ARCVAE
    cfg, B = TINY, 52                                        # R = 52 * 80 = 4160: the fused kernel
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L, dropout=0.2)
    vae.decoder.load_state_dict(O.init_params(cfg, 1234), prefix="decoder.")
    vae.decoder_sampling.load_from_decoder(vae.decoder)
    cond = np.random.RandomState(9).standard_normal((B, cfg.C)).astype(np.float32)
    toks = {}
    for skip_f in ("1", "0"):
        monkeypatch.setenv("ARCVAE_DEC_SKIP_F", skip_f)
        toks[skip_f] = vae.decoder_sampling.generate_with_temperature(torch.zeros(B, cfg.Z), cond, max_length=30, temperature=0.7,
                                                                      early_stopping=False, use_graph=False).cpu().numpy()
    assert np.array_equal(toks["1"], toks["0"])


# ---- 6. the bias gradients as riders of the weight-gradient launches ---------------------------------------------------------------
# (3, 11): the ragged shape of test 1; (3, 173): R = 2 * 256 + 7, two K slices add into one column sum of dbias_l (V = 173 is no
# multiple of 4: dWout / dbout take the tile kernel and the column-sum launch); (13, 40): R = 520, two K slices for dbout's rider too
@pytest.mark.parametrize("B,V", [(3, 11), (3, 173), (13, 40)])
def test_bias_gradients_ride_in_the_weight_gradient_launches(B, V):
    _Dec(_cfg(64, 2, V), B, 7, split3=True).run().check_oracle()


def test_bias_gradients_by_column_sum_launch_where_no_rider_runs():
    """ARCVAE_GEMM_SPLIT=0 (read once per process, hence the child): the exact-f32 TN tile kernel with the gap in M, and every
    bias gradient by column-sum launches over the columns outside the gap."""
    import os
    import subprocess
    import sys
    code = ("import torch, test_dec_dead_gate_gpu as t; r = t._Dec(t._cfg(64, 2, 173), 3, 7, split3=True).run(); r.check_oracle(); "
            "assert bool(torch.isnan(t._quarters(r.ws.ddG, 64)[0]).all()); assert bool((t._forget_rows(r.dec, 2, 64) == 0).all())")
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, ARCVAE_GEMM_SPLIT="0")
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.join(root, "mlx-vae_amd"), os.path.join(root, "oracle"), env.get("PYTHONPATH", "")])
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    subprocess.run(args, env=env, check=True, timeout=120)
