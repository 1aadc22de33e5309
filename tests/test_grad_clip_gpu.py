"""Opt-in global-norm gradient clipping (csrc/clip.hip; DESIGN.md section 10, an extension: the reference's _clip_gradients
sums nothing, Q6).

The rule under test (not torch.nn.utils.clip_grad_norm_): norm = sqrt(sum g^2) over every gradient the step applies; when
norm > max_norm, g * fp32(max_norm / (norm + 1e-8)) goes into the un-bias-corrected Adam.  The fp64 reference is the
oracle's gradients plus that rule plus O.adam_update.

The step's gradients are formed with float atomics in places (latent statistics, split-K GEMMs), so two steps are not
bitwise equal as a whole; what the clip adds is: given a step's (unclipped) gradients in store.grad, its update is bitwise
the clip kernels replayed on them from the pre-step state -- which also shows that every sum of squares saw complete
gradients -- and with the clip inactive bitwise the plain arcvae_adam_update."""
import ctypes as C
import glob
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import arcvae_oracle as O
from helpers import DEFAULT, HYPER, TINY, build_engine, make_case, rel_err

pytestmark = pytest.mark.gpu
LR = 2e-4
LAM = 0.7


def _call(name, *args):
    from arcvae_hip._lib import call
    call(name, *args)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _s():
    from arcvae_hip._lib import stream_ptr
    return stream_ptr()


def _nparts(n):
    from arcvae_hip import _lib
    c = C.c_long(0)
    _lib.check(_lib.load().arcvae_grad_sumsq_partials(C.c_long(n), C.byref(c)), "size query")
    return c.value


# ---- the reference rule ------------------------------------------------------------------------------------------------
def _norm64(grads):
    return math.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))


def _scale(norm, max_norm):
    """fp32(max_norm / (norm + 1e-8)) when norm > max_norm (NaN: False), else None (no scaling)."""
    return np.float32(max_norm / (norm + 1e-8)) if norm > max_norm else None


def _clipped_adam(params, grads, m, v, lr, max_norm, norm=None):
    """The rule + O.adam_update on fp32 arrays (dicts updated in place); returns the norm used."""
    norm = _norm64(grads.values()) if norm is None else norm
    s = _scale(norm, max_norm)
    gs = {k: (np.asarray(g, dtype=np.float32) * s if s is not None else np.asarray(g, dtype=np.float32))
          for k, g in grads.items()}
    O.adam_update(params, gs, m, v, lr)
    return norm


# ---- kernels alone --------------------------------------------------------------------------------------------------------
def _sumsq(g_dev, n, off=0):
    P = _nparts(n)
    part = torch.full((P,), float("nan"), device="cuda")
    _call("arcvae_grad_sumsq", _p(g_dev, off), C.c_long(n), _p(part), C.c_long(P), _s())
    torch.cuda.synchronize()
    return part.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 1023, 1025, 4099, 262147, 1324288, 10_000_001])
def test_sumsq_matches_numpy_any_alignment_and_is_repeatable(n):
    rs = np.random.RandomState(n % 1000)
    g = rs.standard_normal(n + 1).astype(np.float32) * np.float32(1e-3)
    gd = torch.tensor(g, device="cuda")
    aligned = _sumsq(gd, n)
    assert aligned.shape == (min(256, -(-(-(-n // 4)) // 256)),)
    ref = float(np.sum(g[:n].astype(np.float64) ** 2))
    assert abs(float(np.sum(aligned.astype(np.float64))) - ref) <= 1e-5 * ref
    assert np.array_equal(aligned, _sumsq(gd, n))                        # bitwise repeatable
    ref1 = float(np.sum(g[1:].astype(np.float64) ** 2))
    unaligned = _sumsq(gd, n, off=1)                                     # 4-byte offset: the scalar-load path
    assert abs(float(np.sum(unaligned.astype(np.float64))) - ref1) <= 1e-5 * ref1
    # the element-to-partial assignment depends on n alone: the same values at another alignment give the same partials
    g2 = torch.zeros(n + 1, device="cuda")
    g2[1:] = gd[:n]
    assert np.array_equal(_sumsq(g2, n, off=1), aligned)


def _adam_buffers(n, seed, off):
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n + off).astype(np.float32)
    g = (rs.standard_normal(n + off) * 0.05).astype(np.float32)
    m = (rs.standard_normal(n + off) * 1e-3).astype(np.float32)
    v = (rs.random_sample(n + off) * 1e-5).astype(np.float32)
    return p, g, m, v


def _np_adam(p, g, m, v, lr, scale=None):
    f = np.float32
    gs = g * scale if scale is not None else g
    m2 = f(0.9) * m + f(1.0 - 0.9) * gs
    v2 = f(0.999) * v + f(1.0 - 0.999) * (gs * gs)
    return p - (f(lr) * m2) / (np.sqrt(v2) + f(1e-8)), m2, v2


def _run_clipped(bufs, n, off, max_norm, guard=None, plain=False):
    d = [torch.tensor(b, device="cuda") for b in bufs]
    p, g, m, v = d
    sc = torch.zeros(16, device="cuda")
    P = _nparts(n)
    part = torch.empty(P, device="cuda")
    _call("arcvae_grad_sumsq", _p(g, off), C.c_long(n), _p(part), C.c_long(P), _s())
    ga = C.c_void_p(guard.data_ptr()) if guard is not None else C.c_void_p(0)
    if plain:
        _call("arcvae_adam_update", _p(p, off), _p(g, off), _p(m, off), _p(v, off), C.c_long(n), LR, 0.9, 0.999, 1e-8, ga,
              C.c_void_p(0), _s())
    else:
        _call("arcvae_adam_update_clipped", _p(p, off), _p(g, off), _p(m, off), _p(v, off), C.c_long(n), LR, 0.9, 0.999,
              1e-8, ga, C.c_void_p(0), _p(part), C.c_long(P), float(max_norm), _p(sc), _s())
    torch.cuda.synchronize()
    return [t.cpu().numpy()[off:] for t in (p, m, v)], sc.cpu().numpy()


@pytest.mark.parametrize("n", [1, 5, 1024, 100_003, 10_000_001])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_clipped_update_matches_numpy(n, off):
    bufs = _adam_buffers(n, n % 977, off)
    p, g, m, v = (b[off:] for b in bufs)
    norm = _norm64([g])
    for max_norm in (0.25 * norm, 4.0 * norm):                         # active, inactive
        (gp, gm, gv), sc = _run_clipped(bufs, n, off, max_norm)
        assert abs(float(sc[11]) - norm) <= 1e-5 * norm
        s = _scale(float(sc[11]), max_norm)
        if s is None:
            assert sc[12] == 1.0
            (pp, pm, pv), _ = _run_clipped(bufs, n, off, max_norm, plain=True)
            assert np.array_equal(gp, pp) and np.array_equal(gm, pm) and np.array_equal(gv, pv)   # the unclipped arithmetic
        else:
            assert sc[12] == s and 0.2 < s < 0.3
        ep, em, ev = _np_adam(p, g, m, v, LR, s)
        assert np.allclose(gm, em, rtol=1e-6, atol=0) and np.allclose(gv, ev, rtol=1e-6, atol=0)
        assert rel_err(gp - p, ep - p) < 1e-5
        again, sc2 = _run_clipped(bufs, n, off, max_norm)
        assert all(np.array_equal(a, b) for a, b in zip(again, (gp, gm, gv))) and np.array_equal(sc, sc2)


def test_clipped_update_reduces_the_partials_of_all_stores():
    """Two stores, one partial buffer [a | b]: both updates use the norm over both."""
    na, nb = 70_001, 3_333
    a, b = _adam_buffers(na, 1, 0), _adam_buffers(nb, 2, 0)
    da, db = [torch.tensor(x, device="cuda") for x in a], [torch.tensor(x, device="cuda") for x in b]
    Pa, Pb = _nparts(na), _nparts(nb)
    part = torch.empty(Pa + Pb, device="cuda")
    sc = torch.zeros(16, device="cuda")
    _call("arcvae_grad_sumsq", _p(da[1]), C.c_long(na), _p(part), C.c_long(Pa), _s())
    _call("arcvae_grad_sumsq", _p(db[1]), C.c_long(nb), _p(part, Pa), C.c_long(Pb), _s())
    norm = _norm64([a[1], b[1]])
    max_norm = 0.1 * norm
    for d, n, out in ((da, na, None), (db, nb, sc)):
        _call("arcvae_adam_update_clipped", _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), C.c_long(n), LR, 0.9, 0.999, 1e-8,
              C.c_void_p(0), C.c_void_p(0), _p(part), C.c_long(Pa + Pb), max_norm, _p(out) if out is not None else C.c_void_p(0),
              _s())
    torch.cuda.synchronize()
    assert abs(float(sc[11]) - norm) <= 1e-5 * norm
    s = _scale(float(sc[11]), max_norm)
    for d, bufs in ((da, a), (db, b)):
        _, em, ev = _np_adam(*bufs, LR, s)
        assert np.allclose(d[2].cpu().numpy(), em, rtol=1e-6, atol=0) and np.allclose(d[3].cpu().numpy(), ev, rtol=1e-6, atol=0)


def test_tripped_guard_and_nan_norm():
    n = 4099
    bufs = _adam_buffers(n, 7, 0)
    guard = torch.ones(1, dtype=torch.int32, device="cuda")
    (gp, gm, gv), sc = _run_clipped(bufs, n, 0, 1e-3, guard=guard)
    assert np.array_equal(gp, bufs[0]) and np.array_equal(gm, bufs[2]) and np.array_equal(gv, bufs[3])   # nothing applied
    assert np.isnan(sc[11]) and np.isnan(sc[12])
    bufs[1][17] = np.nan                                   # NaN norm: `norm > max_norm` is False -> no scaling
    (gp, gm, gv), sc = _run_clipped(bufs, n, 0, 1e-3)
    (pp, pm, pv), _ = _run_clipped(bufs, n, 0, 1e-3, plain=True)
    assert np.isnan(sc[11]) and sc[12] == 1.0
    assert np.array_equal(gp, pp, equal_nan=True) and np.array_equal(gm, pm, equal_nan=True)


# ---- the step: every path, the update against the clip kernels replayed on the step's own gradients ----------------------
def _stores(eng):
    out = [("enc", eng.enc), ("dec", eng.dec)]
    if eng.prop is not None:
        out.append(("prop", eng.prop))
    return out


def _snapshot(eng):
    return {k: tuple(t.detach().clone() for t in (st.flat, st.adam_m, st.adam_v)) for k, st in _stores(eng)}


def _replay(eng, ws, snap, clip, plain=False):
    """The step's update recomputed from the pre-step state and the step's (unclipped) gradients in store.grad."""
    part = torch.empty_like(ws.clip_part)
    for k, st in _stores(eng):
        off, cnt = ws.clip_off[k]
        _call("arcvae_grad_sumsq", _p(st.grad), C.c_long(st.numel_padded), _p(part, off), C.c_long(cnt), _s())
    out, sc = {}, torch.zeros(16, device="cuda")
    for k, st in _stores(eng):
        p, m, v = (t.clone() for t in snap[k])
        if plain:
            _call("arcvae_adam_update", _p(p), _p(st.grad), _p(m), _p(v), C.c_long(st.numel_padded), LR, 0.9, 0.999, 1e-8,
                  C.c_void_p(0), C.c_void_p(0), _s())
        else:
            _call("arcvae_adam_update_clipped", _p(p), _p(st.grad), _p(m), _p(v), C.c_long(st.numel_padded), LR, 0.9, 0.999,
                  1e-8, C.c_void_p(0), C.c_void_p(0), _p(part), C.c_long(part.numel()), float(clip), _p(sc), _s())
        out[k] = (p, m, v)
    torch.cuda.synchronize()
    return out, sc


def _padding_mask(st):
    mask = np.ones(st.numel_padded, dtype=bool)
    for name, shp in st.shapes.items():
        mask[st.offsets[name]:st.offsets[name] + int(np.prod(shp))] = False
    return mask


def _engine(cfg, params, pred_params=None):
    from arcvae_hip.engine import StepEngine
    eng, enc, dec = build_engine(cfg, params)
    if pred_params is not None:
        from models import PropertyPredictor
        pred = PropertyPredictor(cfg.Z, cfg.C, pred_params["fc1.weight"].shape[0], device="cuda")
        pred.load_state_dict(pred_params)
        eng = StepEngine(enc, dec, eng.d, prop=pred.store)
    return eng


def _pred_params(Z, Cn, Hp, seed=99):
    rs = np.random.RandomState(seed)
    k1, k2 = 1.0 / np.sqrt(Z), 1.0 / np.sqrt(Hp)
    return {"fc1.weight": rs.uniform(-k1, k1, (Hp, Z)).astype(np.float32),
            "fc1.bias": rs.uniform(-k1, k1, (Hp,)).astype(np.float32),
            "fc2.weight": rs.uniform(-k2, k2, (Cn, Hp)).astype(np.float32),
            "fc2.bias": rs.uniform(-k2, k2, (Cn,)).astype(np.float32)}


H256 = O.Config(vocab_size=60, embedding_dim=32, hidden_dim=256, latent_dim=32, num_conditions=1, num_layers=2)
PATHS = {   # name: (cfg, B, T, env, mode, predictor)
    "gated": (TINY, 8, 12, {}, "segments", False),                 # merged main+finish from the second step on
    "unmerged": (TINY, 8, 12, {"ARCVAE_MERGE_FINISH": "0"}, "segments", False),
    "single_chunk": (TINY, 8, 12, {"ARCVAE_BPTT_CHUNKS": "1.0"}, "segments", False),
    "gates_off": (TINY, 8, 12, {"ARCVAE_GATES": "0"}, "segments", False),
    "graph": (TINY, 8, 12, {}, "graph", False),
    "eager": (TINY, 8, 12, {}, "eager", False),
    "persistent": (H256, 64, 16, {}, "segments", False),           # the default recurrence: persistent sweeps, tables on main
    "fused_wgrad": (H256, 64, 16, {"ARCVAE_FUSED_WGRAD": "1"}, "segments", False),
    "predictor": (TINY, 8, 12, {}, "segments", True),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_every_step_path_applies_the_clip_to_complete_gradients(path, monkeypatch):
    import arcvae_hip.engine as E
    cfg, B, T, env, mode, with_pred = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 32) if with_pred else None
    hyper = dict(HYPER, **({"lambda_prop": LAM} if with_pred else {}))
    # the norm of this case's gradients, from a plain gradient-only step
    probe = _engine(cfg, params, pp)
    probe.train_step(x, cond, eps, coins, lr=LR, update=False, **hyper)
    torch.cuda.synchronize()
    norm0 = _norm64([st.grad.cpu().numpy() for _, st in _stores(probe)])
    for clip, active in ((0.1 * norm0, True), (100.0 * norm0, False)):
        eng = _engine(cfg, params, pp)
        eng.mode = mode
        for step in range(3):                              # eager first use + capture, replays (merged finish from step 2)
            snap = _snapshot(eng)
            out = eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, **hyper)
            torch.cuda.synchronize()
            ws = eng.workspace(B, T)
            got_norm, got_scale = float(out["grad_norm"]), float(out["clip_scale"])
            norm = _norm64([st.grad.cpu().numpy() for _, st in _stores(eng)])
            assert abs(got_norm - norm) <= 1e-5 * norm, (step, got_norm, norm)
            assert (got_scale < 0.2) if active else (got_scale == 1.0), (step, got_scale)
            assert float(out["step_status"]) == 0.0
            exp, sc = _replay(eng, ws, snap, clip)
            assert float(sc[11]) == got_norm and float(sc[12]) == got_scale
            for k, st in _stores(eng):
                for a, b, what in zip((st.flat, st.adam_m, st.adam_v), exp[k], ("p", "m", "v")):
                    assert torch.equal(a, b), (path, step, k, what, float((a - b).abs().max()))
            if not active:                                 # inactive: bitwise the unclipped update of the same gradients
                plain, _ = _replay(eng, ws, snap, clip, plain=True)
                for k, st in _stores(eng):
                    for a, b in zip((st.flat, st.adam_m, st.adam_v), plain[k]):
                        assert torch.equal(a, b), (path, step, k)
        eng.check_gates()
    if path == "fused_wgrad":
        assert E.fused_wgrad_ok(eng.workspace(B, T), eng.d)
    if path == "persistent":
        assert E.bptt_reduce_scatter_ok(eng.workspace(B, T), eng.d)
    if path == "single_chunk":
        assert len(E.EncoderBackwardPlan(eng.enc, eng.workspace(B, T), eng.d).chunks) == 1
    for _, st in _stores(eng):                             # the padded tails carry zero gradients: they add nothing to the norm
        assert np.all(st.grad.cpu().numpy()[_padding_mask(st)] == 0.0)


# ---- against the oracle -----------------------------------------------------------------------------------------------------
SHAPES = [(TINY, 6, 12), (DEFAULT, 64, 128), (DEFAULT, 256, 16), (DEFAULT, 2048, 8)]


@pytest.mark.parametrize("cfg,B,T", SHAPES, ids=["tiny", "default_bs64", "rows256", "rows2048"])
def test_clip_active_matches_oracle_one_step_and_trajectory(cfg, B, T):
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    vals64, g64 = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
    norm64 = _norm64(g64.values())
    clip = 0.1 * norm64                                     # well below the norm: the clip is active
    eng = _engine(cfg, params)
    enc, dec = eng.enc, eng.dec
    # one step against the fp64 gradients + the rule + O.adam_update
    ref = {k: v.copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    v = {k: np.zeros_like(vv) for k, vv in ref.items()}
    _clipped_adam(ref, {k: g64[k] for k in ref}, m, v, LR, clip)
    out = eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, **HYPER)
    torch.cuda.synchronize()
    assert abs(float(out["grad_norm"]) - norm64) <= 1e-5 * norm64
    assert abs(float(out["clip_scale"]) - clip / norm64) <= 1e-5 * clip / norm64
    assert abs(float(out["total_loss"]) - float(vals64["total_loss"])) <= 1e-4 * max(1.0, abs(float(vals64["total_loss"])))

    def check(tag):
        for name in ref:
            mod, pn = name.split(".", 1)
            st = enc if mod == "encoder" else dec
            for buf, r, what in ((st.flat, ref, "p"), (st.adam_m, m, "m"), (st.adam_v, v, "v")):
                got = st._view(buf, pn).cpu().numpy()
                if np.abs(r[name]).max() == 0.0:
                    assert np.abs(got).max() == 0.0, (tag, name, what)
                    continue
                assert rel_err(got, r[name]) < 1e-4, (tag, name, what, rel_err(got, r[name]))

    check("step 1")
    # store.grad keeps the UNCLIPPED gradients (the reference's `grads`)
    for name in ("encoder.lstm_layer_0.Wh", "encoder.fc_mu.weight", "decoder.fc_out.weight"):
        mod, pn = name.split(".", 1)
        assert rel_err((enc if mod == "encoder" else dec).g(pn).cpu().numpy(), g64[name]) < 1e-4, name
    # four more steps against the fp32 oracle's trajectory
    for _ in range(4):
        _, g32 = O.loss_and_grads(ref, cfg, x, cond, eps, coins, dtype=torch.float32, **HYPER)
        _clipped_adam(ref, {k: g32[k] for k in ref}, m, v, LR, clip)
        eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, **HYPER)
    torch.cuda.synchronize()
    eng.check_gates()
    check("step 5")


def test_the_norm_includes_the_predictor():
    cfg, B, T = TINY, 8, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 32)
    p = O.to_torch(params, torch.float64, requires_grad=True)
    q = {k: torch.tensor(vv, dtype=torch.float64, requires_grad=True) for k, vv in pp.items()}
    c = torch.tensor(cond, dtype=torch.float64)
    o = O.complete_vae_loss(p, cfg, torch.as_tensor(x, dtype=torch.int64), c, torch.tensor(eps, dtype=torch.float64), coins,
                            lambda_prop=LAM, **HYPER)
    pred = torch.tanh(o["z"] @ q["fc1.weight"].T + q["fc1.bias"]) @ q["fc2.weight"].T + q["fc2.bias"]
    (o["total_loss"] + LAM * ((pred - c) ** 2).mean()).backward()
    g_model = [t.grad.numpy() for t in p.values() if t.grad is not None]
    g_pred = [t.grad.numpy() for t in q.values()]
    norm64 = _norm64(g_model + g_pred)
    assert norm64 - _norm64(g_model) > 1e-4 * norm64       # the predictor's share is visible in the norm
    clip = 0.1 * norm64
    eng = _engine(cfg, params, pp)
    out = eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, lambda_prop=LAM, **HYPER)
    torch.cuda.synchronize()
    assert abs(float(out["grad_norm"]) - norm64) <= 1e-5 * norm64
    # the predictor's update uses the same scale: m = 0.1 * g * scale from a zero state
    s = np.float32(clip / (float(out["grad_norm"]) + 1e-8))
    for k, t in q.items():
        want = np.float32(0.1) * (t.grad.numpy().astype(np.float32) * s)
        assert rel_err(eng.prop._view(eng.prop.adam_m, k).cpu().numpy(), want) < 1e-4, k


def test_api_surface():
    from arcvae_hip import api
    from models.vae import ARCVAE
    cfg, B, T = TINY, 6, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    vae.encoder.load_state_dict(params, prefix="encoder.")
    vae.decoder.load_state_dict(params, prefix="decoder.")
    with pytest.raises(ValueError, match="lr"):
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, grad_clip=1.0, **HYPER)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=LR, grad_clip=bad, **HYPER)
    eng = api.engine_for(vae.encoder, vae.decoder)
    with pytest.raises(ValueError):
        eng.train_step(x, cond, eps, coins, lr=LR, update=False, clip_norm=1.0, **HYPER)
    w0 = vae.encoder.store.flat.clone()
    out, (ge, gd) = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=LR, grad_clip=1e-3,
                                       **HYPER)
    vals = out["loss_status_norm"].tolist()
    assert vals[0] == float(out["total_loss"]) and vals[1] == 0.0 and vals[2] == float(out["grad_norm"]) > 1e-3
    assert float(out["clip_scale"]) < 1.0 and not torch.equal(vae.encoder.store.flat, w0)
    _, g64 = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
    assert rel_err(ge["fc_mu"]["weight"].cpu().numpy(), g64["encoder.fc_mu.weight"]) < 1e-4   # unclipped
    plain, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=LR, **HYPER)
    assert "grad_norm" not in plain and "loss_status_norm" not in plain


def test_bf16_mode_within_its_tolerance():
    """tests/test_bf16_mode_gpu.py's stated tolerance on gradients (8e-2 relative L2, > 0.995 cosine) for the norm and for
    the first step's m = 0.1 * g * scale."""
    from arcvae_hip.engine import StepEngine
    cfg, B, T = O.Config(vocab_size=30, embedding_dim=32, hidden_dim=256, latent_dim=32, num_conditions=1, num_layers=2), 64, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 1.0)
    _, g64 = O.loss_and_grads(params, cfg, x, cond, eps, coins, dtype=torch.float64, **HYPER)
    norm64 = _norm64(g64.values())
    clip = 0.1 * norm64
    eng32, enc, dec = build_engine(cfg, params)
    eng = StepEngine(enc, dec, eng32.d, precision="bf16")
    out = eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, **HYPER)
    torch.cuda.synchronize()
    assert abs(float(out["grad_norm"]) - norm64) <= 8e-2 * norm64
    s = clip / norm64
    for name in ("encoder.lstm_layer_1.Wh", "encoder.fc_mu.weight", "decoder.lstm_layer_0.Wx", "decoder.fc_out.weight"):
        mod, pn = name.split(".", 1)
        st = enc if mod == "encoder" else dec
        got = st._view(st.adam_m, pn).cpu().numpy().astype(np.float64).ravel()
        want = 0.1 * s * g64[name].ravel()
        assert np.linalg.norm(got - want) <= 8e-2 * np.linalg.norm(want), name
        assert float(got @ want) / (np.linalg.norm(got) * np.linalg.norm(want)) > 0.995, name


# ---- data parallelism: two ranks on one MI355X (tests/test_dp_gpu.py's pattern) ------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, B, T, clip, ret):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "mlx-vae_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from arcvae_hip.dp import DataParallelStep, EngineOps
    params, x, cond, eps, coins = make_case(TINY, B, T, 0.6)
    eng, enc, dec = build_engine(TINY, params)
    lo, hi = rank * B // world, (rank + 1) * B // world
    ws = eng.workspace(hi - lo, T)
    eng.set_hyper(ws, **HYPER)
    ops = EngineOps(eng, ws, LR, B, use_graph=True, clip=clip)
    step = DataParallelStep(ops)
    norms = []
    for _ in range(3):
        eng.load_inputs(ws, x[lo:hi], cond[lo:hi], eps[lo:hi], coins)
        step.step()
        torch.cuda.synchronize()
        norms.append(ws.scalars[11:13].cpu().numpy().copy())
    ret[f"r{rank}"] = dict(norms=np.stack(norms), **{f"{tag}_{b}": getattr(st, b).cpu().numpy()
                                                     for tag, st in (("enc", enc), ("dec", dec))
                                                     for b in ("flat", "adam_m", "adam_v")})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("early", ["1", "0"], ids=["early_reduce", "late_reduce"])
def test_two_ranks_clip_equal_single_process(early, monkeypatch):
    monkeypatch.setenv("ARCVAE_DP_EARLY_REDUCE", early)
    B, T, world = 8, 12, 2
    params, x, cond, eps, coins = make_case(TINY, B, T, 0.6)
    eng, enc, dec = build_engine(TINY, params)
    eng.train_step(x, cond, eps, coins, lr=LR, update=False, **HYPER)
    torch.cuda.synchronize()
    clip = 0.1 * _norm64([enc.grad.cpu().numpy(), dec.grad.cpu().numpy()])
    norms = []
    for _ in range(3):
        eng.train_step(x, cond, eps, coins, lr=LR, clip_norm=clip, **HYPER)
        torch.cuda.synchronize()
        norms.append(eng.workspace(B, T).scalars[11:13].cpu().numpy().copy())
    norms = np.stack(norms)
    assert np.all(norms[:, 1] < 0.2)
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), B, T, clip, ret), nprocs=world, join=True)
    r0, r1 = ret["r0"], ret["r1"]
    for k in r0:                                   # same reduced gradients -> same norm, scale and update on every rank
        assert np.array_equal(r0[k], r1[k]), k
    assert np.allclose(r0["norms"], norms, rtol=1e-5, atol=0), (r0["norms"], norms)
    for tag, st in (("enc", enc), ("dec", dec)):
        for b in ("flat", "adam_m", "adam_v"):
            assert rel_err(r0[f"{tag}_{b}"], getattr(st, b).cpu().numpy()) < 1e-5, (tag, b)


# ---- trainer and CLI ------------------------------------------------------------------------------------------------------
def test_train_cli_global_norm_writes_grad_norm_and_round_trips(tmp_path):
    import json
    import train
    from trainer import ARCVAETrainerWithLoss
    base = ["--synthetic", "200", "--epochs", "2", "--hidden_dim", "64", "--embedding_dim", "16", "--latent_dim", "16",
            "--no_progress", "--checkpoint_freq", "1"]
    tr = train.main(base + ["--checkpoint_dir", str(tmp_path / "g"), "--grad_clip_mode", "global_norm", "--grad_clip", "0.5"])
    assert tr.clip_norm == 0.5
    gn = tr.history["grad_norm"]
    assert len(gn) == 2 and all(np.isfinite(gn)) and all(g > 0.0 for g in gn)
    hist = json.load(open(tmp_path / "g" / "training_history.json"))
    assert hist["grad_norm"] == gn
    ck = sorted(glob.glob(str(tmp_path / "g" / "checkpoint_epoch_*.npz")))[-1]
    saved = {(tag, b): getattr(mod.store, b).clone() for tag, mod in tr._modules() for b in ("flat", "adam_m", "adam_v")}
    from models.vae import ARCVAE
    vae = ARCVAE(vocab_size=tr.encoder.dims.V, embedding_dim=16, hidden_dim=64, latent_dim=16,
                 num_conditions=tr.encoder.dims.C, num_layers=tr.encoder.dims.L)
    t2 = ARCVAETrainerWithLoss(vae.encoder, vae.decoder, None, tr.dataset, batch_size=8, checkpoint_dir=str(tmp_path / "r"),
                               progress=False, grad_clip=0.5, grad_clip_mode="global_norm")
    assert t2.load_checkpoint(ck) == 1
    assert t2.history["grad_norm"] == gn
    for (tag, b), val in saved.items():
        assert torch.equal(getattr(dict(t2._modules())[tag].store, b), val), (tag, b)
    tr0 = train.main(base + ["--checkpoint_dir", str(tmp_path / "n")])             # default: the reference's no-op, no key
    assert tr0.clip_norm is None and "grad_norm" not in tr0.history
