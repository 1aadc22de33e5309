"""Property predictor head on z (csrc/prop.hip, models/property_predictor.py; DESIGN.md section 10, an extension).

The fp64 reference is the unchanged oracle's complete_vae_loss (its z keeps its graph) plus
lambda_prop * mean((fc2(tanh(fc1(z))) - cond)^2), back-propagated."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import arcvae_oracle as O
from helpers import (DEFAULT, ELEM_ATOL_FWD, ELEM_ATOL_GRAD, HYPER, SMALL, TINY, assert_elem, build_engine, make_case,
                     rel_err)

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAM = 0.7


def _pred_params(Z, Cn, Hp, seed=99):
    rs = np.random.RandomState(seed)
    k1, k2 = 1.0 / np.sqrt(Z), 1.0 / np.sqrt(Hp)
    return {"fc1.weight": rs.uniform(-k1, k1, (Hp, Z)).astype(np.float32),
            "fc1.bias": rs.uniform(-k1, k1, (Hp,)).astype(np.float32),
            "fc2.weight": rs.uniform(-k2, k2, (Cn, Hp)).astype(np.float32),
            "fc2.bias": rs.uniform(-k2, k2, (Cn,)).astype(np.float32)}


def _predictor(cfg, pp):
    from models import PropertyPredictor
    p = PropertyPredictor(cfg.Z, cfg.C, pp["fc1.weight"].shape[0], device="cuda")
    p.load_state_dict(pp)
    return p


def _ref(cfg, params, pp, x, cond, eps, coins, lam, dtype=torch.float64, hyper=HYPER):
    """(values, gradients) of the full step with the predictor; gradient keys 'encoder.*', 'decoder.*', 'predictor.*'."""
    p = O.to_torch(params, dtype, requires_grad=True)
    q = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in pp.items()}
    c = torch.tensor(cond, dtype=dtype)
    out = O.complete_vae_loss(p, cfg, torch.as_tensor(x, dtype=torch.int64), c, torch.tensor(eps, dtype=dtype), coins,
                              lambda_prop=lam, **hyper)
    pred = torch.tanh(out["z"] @ q["fc1.weight"].T + q["fc1.bias"]) @ q["fc2.weight"].T + q["fc2.bias"]
    prop = ((pred - c) ** 2).mean()
    total = out["total_loss"] + lam * prop
    total.backward()
    vals = {k: v.detach().numpy().copy() for k, v in out.items()}
    vals.update(prop_loss=prop.detach().numpy().copy(), weighted_prop_loss=(lam * prop).detach().numpy().copy(),
                total_loss=total.detach().numpy().copy(), pred=pred.detach().numpy().copy())
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    grads.update({"predictor." + k: v.grad.numpy().copy() for k, v in q.items()})
    return vals, grads


def _engines(cfg, params, pred, precision=None):
    from arcvae_hip.engine import StepEngine
    eng0, enc, dec = build_engine(cfg, params)
    if precision is not None:
        eng0 = StepEngine(enc, dec, eng0.d, precision=precision)
    eng = StepEngine(enc, dec, eng0.d, precision=precision, prop=pred.store)
    return eng0, eng, enc, dec


def _grads(store, prefix):
    return {prefix + n: store.g(n).detach().cpu().numpy().copy() for n in store.names()}


@pytest.mark.parametrize("cfg,B,T", [(TINY, 6, 12), (SMALL, 9, 10), (DEFAULT, 64, 128)], ids=["tiny", "small", "default"])
def test_step_matches_fp64_reference(cfg, B, T):
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 64)
    vals, grads = _ref(cfg, params, pp, x, cond, eps, coins, LAM)
    pred = _predictor(cfg, pp)
    eng0, eng, enc, dec = _engines(cfg, params, pred)
    eng0.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
    torch.cuda.synchronize()
    dec_plain = _grads(dec, "decoder.")
    out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, lambda_prop=LAM, **HYPER)
    torch.cuda.synchronize()
    for k in ("prop_loss", "weighted_prop_loss", "total_loss", "recon_loss", "kl_loss", "mutual_info"):
        assert abs(float(out[k]) - float(vals[k])) <= TOL * max(1.0, abs(float(vals[k]))), (k, float(out[k]), float(vals[k]))
    assert float(out["prop_loss"]) > 0.0
    assert_elem(eng.workspace(B, T).pred.cpu().numpy(), vals["pred"], "pred", ELEM_ATOL_FWD)
    got = {**_grads(enc, "encoder."), **_grads(pred.store, "predictor.")}
    for name, g in got.items():
        ref = grads[name]
        if np.abs(ref).max() == 0.0:
            assert np.abs(g).max() == 0.0, name
            continue
        assert rel_err(g, ref) < TOL, name
        assert_elem(g, ref, "grad " + name, ELEM_ATOL_GRAD)
    # the predictor reaches the encoder: its share of an encoder gradient is far above fp32 noise
    _, g_noprop = _ref(cfg, params, pp, x, cond, eps, coins, 0.0)
    assert rel_err(g_noprop["encoder.fc_mu.weight"], grads["encoder.fc_mu.weight"]) > 1e-3
    # the decoder's gradients do not depend on the predictor
    for name, g in _grads(dec, "decoder.").items():
        assert rel_err(g, dec_plain[name]) <= 1e-6, name


def test_forward_only_paths_match_reference():
    from complete_vae_loss import complete_vae_loss
    from models.vae import ARCVAE
    cfg, B, T = SMALL, 11, 9
    params, x, cond, eps, _ = make_case(cfg, B, T, 0.0)
    coins = np.zeros(T, dtype=bool)                                     # TF = 0: validation
    pp = _pred_params(cfg.Z, cfg.C, 48)
    vals, _ = _ref(cfg, params, pp, x, cond, eps, coins, 0.3)
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    vae.encoder.load_state_dict(params, prefix="encoder.")
    vae.decoder.load_state_dict(params, prefix="decoder.")
    pred = _predictor(cfg, pp)
    # PropertyPredictor.__call__ on the reference's z
    got = pred(torch.tensor(vals["z"], dtype=torch.float32)).cpu().numpy()
    p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in pp.items()}
    z64 = torch.tensor(vals["z"].astype(np.float32), dtype=torch.float64)
    ref = (torch.tanh(z64 @ p64["fc1.weight"].T + p64["fc1.bias"]) @ p64["fc2.weight"].T + p64["fc2.bias"]).numpy()
    assert got.shape == (B, cfg.C)
    assert_elem(got, ref, "pred", ELEM_ATOL_FWD)
    # the loss forward (validation path)
    out = complete_vae_loss(vae.encoder, vae.decoder, pred, x, cond, beta=HYPER["beta"], lambda_prop=0.3,
                            lambda_collapse=HYPER["lambda_collapse"], teacher_forcing_ratio=0.0,
                            free_bits=HYPER["free_bits"], lambda_mi=HYPER["lambda_mi"], target_mi=HYPER["target_mi"],
                            eps=torch.tensor(eps), coins=coins)
    assert len(out) == 12
    for k in ("prop_loss", "weighted_prop_loss", "total_loss", "recon_loss"):
        assert abs(float(out[k]) - float(vals[k])) <= TOL * max(1.0, abs(float(vals[k]))), k
    assert_elem(out["z"].cpu().numpy(), vals["z"], "z", ELEM_ATOL_FWD)


@pytest.mark.parametrize("mode", ["segments", "eager"])
def test_training_trajectory_matches_oracle_adam(mode):
    """Five steps with lr: encoder, decoder and predictor parameters follow the oracle's adam_update (fp32 oracle)."""
    cfg, B, T = TINY, 8, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 32)
    ref = {**{k: v.copy() for k, v in params.items()}, **{"predictor." + k: v.copy() for k, v in pp.items()}}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    v = {k: np.zeros_like(vv) for k, vv in ref.items()}
    pred = _predictor(cfg, pp)
    _, eng, enc, dec = _engines(cfg, params, pred)
    eng.mode = mode
    losses, losses_ref = [], []
    for _ in range(5):
        cur = {k: ref[k] for k in params}
        cur_pp = {k[len("predictor."):]: ref[k] for k in ref if k.startswith("predictor.")}
        vals, grads = _ref(cfg, cur, cur_pp, x, cond, eps, coins, LAM, dtype=torch.float32)
        O.adam_update(ref, grads, m, v, 2e-4)
        losses_ref.append(float(vals["total_loss"]))
        out = eng.train_step(x, cond, eps, coins, lr=2e-4, lambda_prop=LAM, **HYPER)
        losses.append(float(out["total_loss"]))
    torch.cuda.synchronize()
    eng.check_gates()
    assert np.allclose(losses, losses_ref, rtol=1e-4, atol=1e-5)
    for name, r in ref.items():
        mod, pname = name.split(".", 1)
        st = {"encoder": enc, "decoder": dec, "predictor": pred.store}[mod]
        assert rel_err(st.p(pname).cpu().numpy(), r) < 1e-4, name
    assert not np.array_equal(pred.store.p("fc1.weight").cpu().numpy(), pp["fc1.weight"])   # the predictor was trained


@pytest.mark.parametrize("path", ["gated", "gates_off", "graph"])
def test_step_with_the_fused_seam_enabled_uses_the_five_launch_seam(path, monkeypatch):
    """ARCVAE_SEAM_FUSED=1 (opt-in) on a shape the fused seam takes: with a predictor attached every single-process path of
    the step -- gated segments, event waits (ARCVAE_GATES=0), one forked graph (mode "graph") -- still runs the predictor
    between the latent loss and the heads' dcomb chain."""
    import arcvae_hip.engine as E
    monkeypatch.setenv("ARCVAE_SEAM_FUSED", "1")
    if path == "gates_off":
        monkeypatch.setenv("ARCVAE_GATES", "0")
    cfg = O.Config(vocab_size=60, embedding_dim=32, hidden_dim=256, latent_dim=128, num_conditions=2, num_layers=2)
    B, T = 37, 9
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.6)
    pp = _pred_params(cfg.Z, cfg.C, 64)
    vals, grads = _ref(cfg, params, pp, x, cond, eps, coins, LAM)
    pred = _predictor(cfg, pp)
    _, eng, enc, _ = _engines(cfg, params, pred)
    if path == "graph":
        eng.mode = "graph"
    for _ in range(3):                                  # eager + capture, then replays
        out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, lambda_prop=LAM, **HYPER)
    torch.cuda.synchronize()
    assert E.seam_fused_ok(eng.workspace(B, T), eng.d)
    assert (eng.gates is None) == (path == "gates_off")
    for k in ("prop_loss", "weighted_prop_loss", "total_loss", "kl_loss"):
        assert abs(float(out[k]) - float(vals[k])) <= TOL * max(1.0, abs(float(vals[k]))), (k, float(out[k]), float(vals[k]))
    for name, g in {**_grads(enc, "encoder."), **_grads(pred.store, "predictor.")}.items():
        ref = grads[name]
        if np.abs(ref).max() == 0.0:
            assert np.abs(g).max() == 0.0, name
            continue
        assert_elem(g, ref, "grad " + name, ELEM_ATOL_GRAD)


def test_a_predictor_step_needs_lambda_prop():
    from arcvae_hip import api
    from models.vae import ARCVAE
    cfg, B, T = TINY, 6, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pred = _predictor(cfg, _pred_params(cfg.Z, cfg.C, 16))
    _, eng, _, _ = _engines(cfg, params, pred)
    with pytest.raises(ValueError, match="lambda_prop"):
        eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
    eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, lambda_prop=0.2, **HYPER)
    with pytest.raises(ValueError, match="lambda_prop"):    # not the value of the call before
        eng.forward_loss(x, cond, eps, coins, **HYPER)
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    with pytest.raises(ValueError, match="lambda_prop"):
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=2e-4, predictor=pred, **HYPER)


def test_captured_and_eager_training_agree():
    cfg, B, T = TINY, 8, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 32)
    finals = []
    for mode in ("segments", "eager"):
        pred = _predictor(cfg, pp)
        _, eng, enc, _ = _engines(cfg, params, pred)
        eng.mode = mode
        for _ in range(5):
            eng.train_step(x, cond, eps, coins, lr=2e-4, lambda_prop=LAM, **HYPER)
        torch.cuda.synchronize()
        finals.append((enc.flat.cpu().numpy().copy(), pred.store.flat.cpu().numpy().copy()))
    assert rel_err(finals[0][0], finals[1][0]) < 1e-5
    assert rel_err(finals[0][1], finals[1][1]) < 1e-5


# ---- the kernels alone: batch sizes, multi-block reduction, determinism ------------------------------------------------
def _kernel_inputs(B, Z, Cn, Hp, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)   # noqa: E731
    return dict(z=f(B, Z), cond=f(B, Cn), eps=f(B, Z), mu_raw=f(B, Z), lv_raw=f(B, Z), dmu=f(B, Z) * 1e-3,
                dlv=f(B, Z) * 1e-3, **_pred_params(Z, Cn, Hp, seed + 1))


def _run_kernels(a, lam):
    from arcvae_hip._lib import call, ptr, stream_ptr
    from models.property_predictor import ws_floats
    B, Z = a["z"].shape
    Cn, Hp = a["fc2.weight"].shape
    d = {k: torch.tensor(v, device="cuda") for k, v in a.items()}
    hyper = torch.zeros(8, device="cuda")
    hyper[5] = lam
    ws = torch.empty(ws_floats(B, Z, Cn, Hp), device="cuda")
    pred = torch.empty(B, Cn, device="cuda")
    sc = torch.zeros(16, device="cuda")
    gr = {k: torch.full(v.shape, 7.0, device="cuda") for k, v in a.items() if k.startswith("fc")}   # overwritten, not added to
    call("arcvae_prop_backward", ptr(d["z"]), ptr(d["cond"]), ptr(d["eps"]), ptr(d["mu_raw"]), ptr(d["lv_raw"]),
         ptr(d["fc1.weight"]), ptr(d["fc1.bias"]), ptr(d["fc2.weight"]), ptr(d["fc2.bias"]), ptr(hyper), ptr(d["dmu"]),
         ptr(d["dlv"]), ptr(pred), ptr(ws), C.c_long(ws.numel()), B, Z, Cn, Hp, stream_ptr())
    call("arcvae_prop_wgrad", ptr(d["z"]), ptr(ws), C.c_long(ws.numel()), ptr(hyper), ptr(gr["fc1.weight"]),
         ptr(gr["fc1.bias"]), ptr(gr["fc2.weight"]), ptr(gr["fc2.bias"]), ptr(sc), B, Z, Cn, Hp, stream_ptr())
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in gr.items()}
    out.update(pred=pred.cpu().numpy(), dmu=d["dmu"].cpu().numpy(), dlv=d["dlv"].cpu().numpy(),
               prop=float(sc[5]), wprop=float(sc[6]))
    return out


def _kernel_ref(a, lam):
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in a.items()}
    for k in ("z", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        t[k].requires_grad_(True)
    pred = torch.tanh(t["z"] @ t["fc1.weight"].T + t["fc1.bias"]) @ t["fc2.weight"].T + t["fc2.bias"]
    prop = ((pred - t["cond"]) ** 2).mean()
    (lam * prop).backward()
    dz = t["z"].grad
    tm, tl = torch.tanh(t["mu_raw"] / 2), torch.tanh(t["lv_raw"] / 2)
    out = {k: t[k].grad.numpy() for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")}
    out.update(pred=pred.detach().numpy(), prop=float(prop.detach()), wprop=float(lam * prop.detach()),
               dmu=(t["dmu"] + dz * (1 - tm * tm)).numpy(),
               dlv=(t["dlv"] + dz * t["eps"] * 0.5 * torch.exp(0.5 * (tl - 1)) * 0.5 * (1 - tl * tl)).numpy())
    return out


@pytest.mark.parametrize("B", [1, 33, 256, 1000, 2048])     # (the reduction's row slices per output: 1, 1, 4, 8 ragged, 16)
def test_kernels_at_batch_sizes(B):
    Z, Cn, Hp = 128, 3, 64
    a = _kernel_inputs(B, Z, Cn, Hp, B)
    got, ref = _run_kernels(a, 0.4), _kernel_ref(a, 0.4)
    assert abs(got["prop"] - ref["prop"]) <= TOL * abs(ref["prop"]) and abs(got["wprop"] - ref["wprop"]) <= TOL * abs(ref["wprop"])
    for k in ("pred", "dmu", "dlv", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        assert_elem(got[k], ref[k], k, ELEM_ATOL_GRAD)
    again = _run_kernels(a, 0.4)                              # fixed-order reduction: bitwise repeatable
    for k, v in got.items():
        assert np.array_equal(np.asarray(v), np.asarray(again[k])), k
    perm = np.random.RandomState(5).permutation(B)            # row order: the same loss up to fp32 reordering
    ap = {k: (v[perm] if k in ("z", "cond", "eps", "mu_raw", "lv_raw", "dmu", "dlv") else v) for k, v in a.items()}
    gp = _run_kernels(ap, 0.4)
    assert abs(gp["prop"] - got["prop"]) <= 1e-5 * abs(got["prop"])
    assert np.array_equal(gp["pred"], got["pred"][perm]) and np.array_equal(gp["dmu"], got["dmu"][perm])
    for k in ("fc1.weight", "fc2.weight", "fc1.bias", "fc2.bias"):
        assert rel_err(gp[k], got[k]) < 1e-5, k


def test_kernels_at_the_size_limits():
    a = _kernel_inputs(40, 512, 8, 256, 3)
    got, ref = _run_kernels(a, 1.0), _kernel_ref(a, 1.0)
    assert abs(got["prop"] - ref["prop"]) <= TOL * abs(ref["prop"])
    for k in ("pred", "dmu", "dlv", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        assert_elem(got[k], ref[k], k, ELEM_ATOL_GRAD)


# ---- edge cases ---------------------------------------------------------------------------------------------------------
def test_lambda_zero_gives_zero_predictor_gradients_and_the_plain_encoder_gradients():
    cfg, B, T = TINY, 6, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pred = _predictor(cfg, _pred_params(cfg.Z, cfg.C, 32))
    eng0, eng, enc, dec = _engines(cfg, params, pred)
    eng0.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
    torch.cuda.synchronize()
    plain = {**_grads(enc, "encoder."), **_grads(dec, "decoder.")}
    out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, lambda_prop=0.0, **HYPER)
    torch.cuda.synchronize()
    assert float(out["prop_loss"]) > 0.0 and float(out["weighted_prop_loss"]) == 0.0
    for name, g in _grads(pred.store, "predictor.").items():
        assert np.all(g == 0.0), name
    for name, g in {**_grads(enc, "encoder."), **_grads(dec, "decoder.")}.items():
        assert rel_err(g, plain[name]) <= 1e-6, name


def test_no_predictor_call_after_a_predictor_call_is_the_plain_loss():
    """A predictor engine must not leak into the pair's plain engine (or its captured graphs)."""
    from complete_vae_loss import complete_vae_loss
    from models.vae import ARCVAE
    cfg, B, T = TINY, 6, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)

    def vae():
        m = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                   num_layers=cfg.L)
        m.encoder.load_state_dict(params, prefix="encoder.")
        m.decoder.load_state_dict(params, prefix="decoder.")
        return m

    kw = dict(beta=HYPER["beta"], lambda_prop=0.5, lambda_collapse=HYPER["lambda_collapse"], teacher_forcing_ratio=0.7,
              free_bits=HYPER["free_bits"], lambda_mi=HYPER["lambda_mi"], target_mi=HYPER["target_mi"],
              eps=torch.tensor(eps), coins=coins)
    used, fresh = vae(), vae()
    pred = _predictor(cfg, _pred_params(cfg.Z, cfg.C, 16))
    for _ in range(2):
        with_p = complete_vae_loss(used.encoder, used.decoder, pred, x, cond, **kw)
    assert float(with_p["prop_loss"]) > 0.0
    a = complete_vae_loss(used.encoder, used.decoder, None, x, cond, **kw)
    b = complete_vae_loss(fresh.encoder, fresh.decoder, None, x, cond, **kw)
    assert float(a["prop_loss"]) == 0.0 and float(a["weighted_prop_loss"]) == 0.0
    for k in ("total_loss", "recon_loss", "kl_loss", "collapse_penalty", "mutual_info", "mi_penalty"):
        assert abs(float(a[k]) - float(b[k])) <= 1e-6 * max(1.0, abs(float(b[k]))), k
    assert abs(float(with_p["total_loss"]) - float(a["total_loss"]) - float(with_p["weighted_prop_loss"])) <= 1e-5


def test_predictor_with_data_parallelism_is_refused():
    from arcvae_hip import api
    from models.vae import ARCVAE
    vae = ARCVAE(vocab_size=TINY.V, embedding_dim=TINY.E, hidden_dim=TINY.H, latent_dim=TINY.Z, num_conditions=TINY.C,
                 num_layers=TINY.L)
    pred = _predictor(TINY, _pred_params(TINY.Z, TINY.C, 8))
    with pytest.raises(ValueError, match="data parallelism"):
        api.enable_data_parallel(vae.encoder, vae.decoder, predictor=pred)
    from arcvae_hip.dp import EngineDataParallel
    with pytest.raises(ValueError, match="data parallelism"):
        EngineDataParallel(api.engine_for(vae.encoder, vae.decoder, pred))


def test_predictor_shape_must_match_the_model():
    from arcvae_hip import api
    from models import PropertyPredictor
    from models.vae import ARCVAE
    vae = ARCVAE(vocab_size=TINY.V, embedding_dim=TINY.E, hidden_dim=TINY.H, latent_dim=TINY.Z, num_conditions=TINY.C,
                 num_layers=TINY.L)
    with pytest.raises(ValueError):
        api.engine_for(vae.encoder, vae.decoder, PropertyPredictor(TINY.Z, TINY.C + 1, 8, device="cuda"))
    for hp in (0, 257):
        with pytest.raises(ValueError):
            PropertyPredictor(TINY.Z, TINY.C, hp, device="cuda")


# ---- trainer and CLI ----------------------------------------------------------------------------------------------------
def _datasets(n, T, vocab):
    import train
    from mlx_data.dataloader import MoleculeDataset
    data = train.synthetic_dataset(n, vocab, max_length=T)
    props = np.array([[m["tpsa"]] for m in data["molecules"]], dtype=np.float32)
    seqs = data["tokenized_sequences"]
    k = int(0.8 * n)
    tr = MoleculeDataset(seqs[:k], props[:k], max_length=T)
    va = MoleculeDataset(seqs[k:], props[k:], max_length=T, properties_mean=tr.properties_mean,
                         properties_std=tr.properties_std)
    return tr, va


def test_trainer_trains_the_predictor_and_round_trips_checkpoints(tmp_path):
    from models import PropertyPredictor
    from models.vae import ARCVAE
    from trainer import ARCVAETrainerWithLoss
    cfg = TINY
    tr, va = _datasets(60, 24, cfg.V)
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    pred = PropertyPredictor(cfg.Z, cfg.C, 16, device="cuda", generator=torch.Generator().manual_seed(3))
    w0 = pred.store.flat.clone()
    trainer = ARCVAETrainerWithLoss(vae.encoder, vae.decoder, pred, tr, learning_rate=2e-4, batch_size=8,
                                    lambda_prop=0.5, checkpoint_dir=str(tmp_path / "ck"), progress=False)
    np.random.seed(0)
    m = trainer.train_epoch(0, 2, val_dataset=va)
    torch.cuda.synchronize()
    for k in ("train_prop", "val_prop"):
        assert np.isfinite(m[k]) and m[k] > 0.0, (k, m[k])
    assert not torch.equal(pred.store.flat, w0)
    trainer.save_checkpoint(0, is_best=True)
    ck = np.load(tmp_path / "ck" / "checkpoint_best.npz")
    assert {f"predictor_weights/{n}" for n in pred.store.names()} <= set(ck.files)
    assert {f"predictor_optimizer_state/{s}/{n}" for s in ("m", "v") for n in pred.store.names()} <= set(ck.files)
    saved = {b: getattr(pred.store, b).clone() for b in ("flat", "adam_m", "adam_v")}
    pred2 = PropertyPredictor(cfg.Z, cfg.C, 16, device="cuda", generator=torch.Generator().manual_seed(4))
    t2 = ARCVAETrainerWithLoss(vae.encoder, vae.decoder, pred2, tr, batch_size=8, checkpoint_dir=str(tmp_path / "ck2"),
                               progress=False)
    t2.load_checkpoint(str(tmp_path / "ck" / "checkpoint_best.npz"))
    for b, v in saved.items():
        assert torch.equal(getattr(pred2.store, b), v), b
    # a checkpoint without predictor keys leaves the predictor as initialised
    plain = ARCVAETrainerWithLoss(vae.encoder, vae.decoder, None, tr, batch_size=8, checkpoint_dir=str(tmp_path / "ck3"),
                                  progress=False)
    plain.save_checkpoint(0)
    pred3 = PropertyPredictor(cfg.Z, cfg.C, 16, device="cuda", generator=torch.Generator().manual_seed(5))
    init3 = pred3.store.flat.clone()
    ARCVAETrainerWithLoss(vae.encoder, vae.decoder, pred3, tr, batch_size=8, checkpoint_dir=str(tmp_path / "ck4"),
                          progress=False).load_checkpoint(str(tmp_path / "ck3" / "checkpoint_epoch_000.npz"))
    assert torch.equal(pred3.store.flat, init3)


def test_train_cli_with_and_without_predictor(tmp_path):
    import train
    base = ["--synthetic", "200", "--epochs", "1", "--hidden_dim", "64", "--embedding_dim", "16", "--latent_dim", "16",
            "--no_progress"]
    tr = train.main(base + ["--checkpoint_dir", str(tmp_path / "p"), "--property_predictor_hidden", "32"])
    assert tr.property_predictor is not None and np.isfinite(tr.history["val_prop"][0]) and tr.history["val_prop"][0] > 0
    files = glob.glob(str(tmp_path / "p" / "*.npz"))
    assert files and all(any(k.startswith("predictor_weights/") for k in np.load(f).files) for f in files)
    tr0 = train.main(base + ["--checkpoint_dir", str(tmp_path / "n")])
    assert tr0.property_predictor is None and tr0.history["val_prop"][0] == 0.0
    files = glob.glob(str(tmp_path / "n" / "*.npz"))
    assert files and not any(k.startswith("predictor") for f in files for k in np.load(f).files)


# ---- throughput mode ----------------------------------------------------------------------------------------------------
def test_bf16_mode_step_with_predictor_within_its_tolerance():
    """tests/test_bf16_mode_gpu.py's stated tolerance: loss scalars 2e-2 relative, gradients 8e-2 relative L2 and > 0.995
    cosine; the predictor itself stays fp32."""
    cfg, B, T = O.Config(vocab_size=30, embedding_dim=32, hidden_dim=256, latent_dim=32, num_conditions=1, num_layers=2), 64, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 1.0)
    pp = _pred_params(cfg.Z, cfg.C, 64)
    vals, grads = _ref(cfg, params, pp, x, cond, eps, coins, LAM)
    pred = _predictor(cfg, pp)
    _, eng, enc, dec = _engines(cfg, params, pred, precision="bf16")
    out = eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, lambda_prop=LAM, **HYPER)
    torch.cuda.synchronize()
    for k in ("prop_loss", "weighted_prop_loss", "total_loss"):
        assert abs(float(out[k]) - float(vals[k])) <= 2e-2 * abs(float(vals[k])), k
    for name, g in {**_grads(enc, "encoder."), **_grads(pred.store, "predictor.")}.items():
        ref = grads[name].astype(np.float64)
        if np.abs(ref).max() == 0.0:
            continue
        g = g.astype(np.float64)
        assert np.linalg.norm(g - ref) <= 8e-2 * np.linalg.norm(ref), name
        assert float(g.ravel() @ ref.ravel()) / (np.linalg.norm(g) * np.linalg.norm(ref)) > 0.995, name
