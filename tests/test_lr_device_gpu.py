"""The learning rate as a device word (arcvae_adam_step, csrc/misc.hip + csrc/clip.hip) and the
schedules on top of it (lr_schedule.py, trainer.py, train.py).

What device-rate mode promises: with the word holding fp32(lr), every update form is BITWISE its by-value entry point; the
word is written between two steps, so each step applies exactly its own rate on every stream -- shown by alternating rates
with zeros (a zero step moves no parameter, its neighbours do: a late or early write would show in the step beside it) --;
and one captured set of segments serves every rate."""
import ctypes as C
import glob
import math
import os
import shutil
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
NULL = C.c_void_p(0)


def _call(name, *args):
    from arcvae_hip._lib import call
    call(name, *args)


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else NULL


def _s():
    from arcvae_hip._lib import stream_ptr
    return stream_ptr()


def _nparts(n):
    from arcvae_hip import _lib
    c = C.c_long(0)
    _lib.check(_lib.load().arcvae_grad_sumsq_partials(C.c_long(n), C.byref(c)), "size query")
    return c.value


# ---- the kernel alone: every form against its by-value entry point ------------------------------------------------------
FORMS = ("plain", "finalize", "clipped", "finalize_clipped")
FB, FZ, FT = 37, 8, 12           # rows, latent width, sequence length of the finalize part's inputs


def _adam_buffers(n, seed, off):
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n + off).astype(np.float32)
    g = (rs.standard_normal(n + off) * 0.05).astype(np.float32)
    m = (rs.standard_normal(n + off) * 1e-3).astype(np.float32)
    v = (rs.random_sample(n + off) * 1e-5).astype(np.float32)
    return p, g, m, v


def _finalize_inputs(seed):
    rs = np.random.RandomState(seed + 5)
    rowloss = (rs.random_sample(FB) * 40.0).astype(np.float32)
    stats = rs.standard_normal(2 * FZ + 4).astype(np.float32)
    stats[2 * FZ + 2] = FB                                  # the row count the recon term divides by
    scalars = rs.random_sample(16).astype(np.float32)       # [3], [4], [6], [8]: the terms of the total; the rest: bystanders
    return rowloss, stats, scalars


def _run(form, bufs, n, off, lr=LR, word=None, guard=None, max_norm=None):
    """One update launch on copies of `bufs`.  word None: the by-value entry point of `form` at rate lr; else arcvae_adam_step
    with the rate word holding `word`.  Returns (p, m, v), scalars, stats -- device tensors."""
    p, g, m, v = (torch.tensor(b, device="cuda") for b in bufs)
    rowloss, stats, scalars = (torch.tensor(a, device="cuda") for a in _finalize_inputs(n))
    fin, clip = "finalize" in form, "clipped" in form
    P = _nparts(n)
    part = torch.empty(P, device="cuda")
    _call("arcvae_grad_sumsq", _p(g, off), C.c_long(n), _p(part), C.c_long(P), _s())
    if max_norm is None:
        max_norm = 0.25 * float(np.sqrt(np.sum(bufs[1][off:].astype(np.float64) ** 2)))      # active
    ga = C.c_void_p(guard.data_ptr()) if guard is not None else NULL
    head = (_p(p, off), _p(g, off), _p(m, off), _p(v, off), C.c_long(n))
    fargs = (_p(rowloss), FB, _p(stats), _p(scalars), FZ, FT)
    cargs = (_p(part), C.c_long(P), float(max_norm))
    if word is not None:
        w = torch.tensor([word], dtype=torch.float32, device="cuda")
        _call("arcvae_adam_step", *head, _p(w), 0.9, 0.999, 1e-8, ga, NULL,
              *(fargs if fin else (NULL, 0, NULL, _p(scalars), 0, 0)), *(cargs if clip else (NULL, C.c_long(0), 0.0)), _s())
    elif form == "plain":
        _call("arcvae_adam_update", *head, lr, 0.9, 0.999, 1e-8, ga, NULL, _s())
    elif form == "finalize":
        _call("arcvae_adam_update_finalize", *head, lr, 0.9, 0.999, 1e-8, ga, NULL, *fargs, _s())
    elif form == "clipped":
        _call("arcvae_adam_update_clipped", *head, lr, 0.9, 0.999, 1e-8, ga, NULL, *cargs, _p(scalars), _s())
    else:
        _call("arcvae_adam_update_finalize_clipped", *head, lr, 0.9, 0.999, 1e-8, ga, NULL, *fargs, *cargs, _s())
    torch.cuda.synchronize()
    return (p, m, v), scalars, stats


KEPT = list(range(13)) + [15]        # the scalars the by-value forms own or leave alone; [13] is the rate, [14] unused


@pytest.mark.parametrize("n", [1, 5, 1024, 100_003])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
def test_device_rate_is_bitwise_the_by_value_update(n, off):
    bufs = _adam_buffers(n, n % 977, off)
    for form in FORMS:
        want, wsc, wst = _run(form, bufs, n, off)
        got, gsc, gst = _run(form, bufs, n, off, word=np.float32(LR))
        for a, b, what in zip(got, want, "pmv"):
            assert torch.equal(a, b), (form, what, float((a - b).abs().max()))
        assert not torch.equal(got[0], torch.tensor(bufs[0], device="cuda"))     # ... and it is an update
        assert torch.equal(gsc[KEPT], wsc[KEPT]) and torch.equal(gst, wst), form
        assert gsc[13].item() == np.float32(LR), form
        assert wsc[13].item() == _finalize_inputs(n)[2][13]                      # the by-value forms never write slot 13


def test_device_rate_edge_words():
    n = 4099
    bufs = _adam_buffers(n, 7, 0)
    p0, m0, v0 = (torch.tensor(bufs[i], device="cuda") for i in (0, 2, 3))
    for form in FORMS:
        want, wsc, wst = _run(form, bufs, n, 0)
        # a zero word is a rate: m and v advance as in the by-value form, p does not move
        got, sc, _ = _run(form, bufs, n, 0, word=0.0)
        assert torch.equal(got[0], p0) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), form
        assert not torch.equal(got[1], m0) and sc[13].item() == 0.0
        # negative, infinite, NaN: nothing is updated; the word is reported; the loss / clip scalars are written as ever
        for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
            got, sc, st = _run(form, bufs, n, 0, word=bad)
            assert torch.equal(got[0], p0) and torch.equal(got[1], m0) and torch.equal(got[2], v0), (form, bad)
            assert (math.isnan(sc[13].item()) if math.isnan(bad) else sc[13].item() == bad), (form, bad)
            assert torch.equal(sc[KEPT], wsc[KEPT]) and torch.equal(st, wst), (form, bad)
        # a tripped guard: nothing is updated, the scalars are those of the by-value form on the same guard
        guard = torch.ones(1, dtype=torch.int32, device="cuda")
        gwant, gwsc, _ = _run(form, bufs, n, 0, guard=guard)
        got, sc, _ = _run(form, bufs, n, 0, word=np.float32(LR), guard=guard)
        assert torch.equal(got[0], p0) and torch.equal(got[1], m0) and torch.equal(got[2], v0), form
        assert all(torch.equal(a, b) for a, b in zip(got, gwant))
        assert torch.equal(torch.isnan(sc[KEPT]), torch.isnan(gwsc[KEPT])), form
        keep = ~torch.isnan(gwsc[KEPT])
        assert torch.equal(sc[KEPT][keep], gwsc[KEPT][keep]) and sc[13].item() == np.float32(LR), form
        if "finalize" in form:
            assert sc[15].item() == 1.0 and math.isnan(sc[0].item())


def test_scalars_are_optional_without_parts():
    """The plain form reports nothing when it is given no scalars (the decoder's and the predictor's updates)."""
    n = 1025
    bufs = _adam_buffers(n, 3, 0)
    want, _, _ = _run("plain", bufs, n, 0)
    p, g, m, v = (torch.tensor(b, device="cuda") for b in bufs)
    w = torch.tensor([LR], dtype=torch.float32, device="cuda")
    _call("arcvae_adam_step", _p(p), _p(g), _p(m), _p(v), C.c_long(n), _p(w), 0.9, 0.999, 1e-8, NULL, NULL,
          NULL, 0, NULL, NULL, 0, 0, NULL, C.c_long(0), 0.0, _s())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), want))


# ---- the step: every path applies each step's own rate ------------------------------------------------------------------
def _stores(eng):
    out = [("enc", eng.enc), ("dec", eng.dec)]
    if eng.prop is not None:
        out.append(("prop", eng.prop))
    return out


def _snapshot(eng):
    return {k: tuple(t.detach().clone() for t in (st.flat, st.adam_m, st.adam_v)) for k, st in _stores(eng)}


def _norm64(grads):
    return math.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))


def _replay(eng, ws, snap, lr, clip):
    """The step's update recomputed BY VALUE (rate lr) from the pre-step state and the step's gradients in store.grad."""
    if clip is not None:
        part = torch.empty_like(ws.clip_part)
        for k, st in _stores(eng):
            off, cnt = ws.clip_off[k]
            _call("arcvae_grad_sumsq", _p(st.grad), C.c_long(st.numel_padded), _p(part, off), C.c_long(cnt), _s())
    out, sc = {}, torch.zeros(16, device="cuda")
    for k, st in _stores(eng):
        p, m, v = (t.clone() for t in snap[k])
        if clip is None:
            _call("arcvae_adam_update", _p(p), _p(st.grad), _p(m), _p(v), C.c_long(st.numel_padded), lr, 0.9, 0.999, 1e-8,
                  NULL, NULL, _s())
        else:
            _call("arcvae_adam_update_clipped", _p(p), _p(st.grad), _p(m), _p(v), C.c_long(st.numel_padded), lr, 0.9, 0.999,
                  1e-8, NULL, NULL, _p(part), C.c_long(part.numel()), float(clip), _p(sc), _s())
        out[k] = (p, m, v)
    torch.cuda.synchronize()
    return out


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
PATHS = {   # name: (cfg, B, T, env, mode, predictor) -- the table of tests/test_grad_clip_gpu.py, restated
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
RATES = [1e-3, 0.0, 5e-4, 0.0, 2e-4, 1e-3]


@pytest.mark.parametrize("path", list(PATHS))
def test_every_step_path_applies_its_own_rate(path, monkeypatch):
    import arcvae_hip.engine as E
    cfg, B, T, env, mode, with_pred = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    pp = _pred_params(cfg.Z, cfg.C, 32) if with_pred else None
    hyper = dict(HYPER, **({"lambda_prop": LAM} if with_pred else {}))
    probe = _engine(cfg, params, pp)                       # the norm of this case's gradients: a clip well below it is active
    probe.train_step(x, cond, eps, coins, lr=LR, update=False, **hyper)
    torch.cuda.synchronize()
    norm0 = _norm64([st.grad.cpu().numpy() for _, st in _stores(probe)])
    # (a clip far below the first norm: the norm falls over six steps at these rates, the clip has to stay active)
    for clip in (None, 0.01 * norm0):
        eng = _engine(cfg, params, pp)
        eng.mode = mode
        sets = []
        for step, lr in enumerate(RATES):
            snap = _snapshot(eng)
            out = eng.train_step(x, cond, eps, coins, lr=lr, clip_norm=clip, lr_device=True, **hyper)
            torch.cuda.synchronize()
            ws = eng.workspace(B, T)
            assert float(out["lr"]) == np.float32(lr), (path, step, float(out["lr"]))
            assert float(out["step_status"]) == 0.0
            if clip is not None:
                assert float(out["clip_scale"]) < 1.0                    # active: the clipped form's arithmetic ran
            exp = _replay(eng, ws, snap, lr, clip)
            for k, st in _stores(eng):
                for a, b, what in zip((st.flat, st.adam_m, st.adam_v), exp[k], ("p", "m", "v")):
                    assert torch.equal(a, b), (path, clip is not None, step, k, what, float((a - b).abs().max()))
                moved = not torch.equal(st.flat, snap[k][0])
                assert moved == (lr != 0.0), (path, step, k)       # a zero step moves nothing, its neighbours do
            sets.append((len(eng._runners), len(eng._graphs)))
        eng.check_gates()
        assert sets[5] == sets[1], (path, sets)                    # one captured set serves every rate
        assert sets[5][1 if mode == "graph" else 0] >= 1
    if path == "fused_wgrad":
        assert E.fused_wgrad_ok(eng.workspace(B, T), eng.d)
    if path == "persistent":
        assert E.bptt_reduce_scatter_ok(eng.workspace(B, T), eng.d)
    if path == "single_chunk":
        assert len(E.EncoderBackwardPlan(eng.enc, eng.workspace(B, T), eng.d).chunks) == 1


def test_by_value_mode_is_untouched_and_rate_is_validated():
    """lr_device=False: the keys carry the value (a new rate is a new set, as before) and no "lr" is reported; the rate
    word's value is checked on the host; an unchanged rate is not written again."""
    from arcvae_hip.engine import LR_DEVICE
    cfg, B, T = TINY, 8, 12
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    eng = _engine(cfg, params)
    for lr in (1e-3, 5e-4):
        out = eng.train_step(x, cond, eps, coins, lr=lr, **HYPER)
    torch.cuda.synchronize()
    assert "lr" not in out and len(eng._runners) == 2 and all(LR_DEVICE not in k for k in eng._runners)
    for bad in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="learning rate"):
            eng.train_step(x, cond, eps, coins, lr=bad, lr_device=True, **HYPER)
    ws = eng.workspace(B, T)
    for lr in (1e-3, 1e-3, 3e-4):
        out = eng.train_step(x, cond, eps, coins, lr=lr, lr_device=True, **HYPER)
        assert ws._rate_val == float(np.float32(lr))
    torch.cuda.synchronize()
    assert float(out["lr"]) == np.float32(3e-4) == ws.rate.word.item()
    assert len(eng._runners) == 3 and sum(LR_DEVICE in k for k in eng._runners) == 1
    g = eng.train_step(x, cond, eps, coins, lr=0.0, update=False, lr_device=True, **HYPER)     # gradient-only: no rate applied
    assert "lr" not in g


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
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr_device=True, **HYPER)
    with pytest.raises(ValueError, match="learning rate"):
        api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=-1.0, lr_device=True, **HYPER)
    w0 = vae.encoder.store.flat.clone()
    out, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=0.0, lr_device=True, **HYPER)
    assert float(out["lr"]) == 0.0 and torch.equal(vae.encoder.store.flat, w0)
    out, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=3e-4, lr_device=True,
                                grad_clip=1e-3, **HYPER)
    assert float(out["lr"]) == np.float32(3e-4) and float(out["clip_scale"]) < 1.0
    assert not torch.equal(vae.encoder.store.flat, w0) and out["loss_status_norm"].tolist()[1] == 0.0
    plain, _ = api.value_and_grad(vae.encoder, vae.decoder, x, cond, eps=eps, coins=coins, lr=LR, **HYPER)
    assert "lr" not in plain


# ---- against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B,T", [(TINY, 6, 12), (DEFAULT, 64, 128)], ids=["tiny", "default_bs64"])
def test_scheduled_trajectory_matches_fp64_oracle(cfg, B, T):
    """Four steps under cosine, W = 2, N = 4, r = 0.1 against the fp64 oracle stepping its own un-bias-corrected Adam with the
    same rates, at the project's 1e-4 parity tolerance."""
    from lr_schedule import LRSchedule
    sch = LRSchedule(LR, "cosine", warmup_steps=2, total_steps=4, min_lr_ratio=0.1)
    rates = [sch.lr(s) for s in range(4)]
    assert rates[0] == LR / 2 and rates[1] == LR and abs(rates[3] - LR * 0.55) < 1e-12 * LR
    params, x, cond, eps, coins = make_case(cfg, B, T, 0.7)
    ref = {k: v.astype(np.float64) for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    v = {k: np.zeros_like(vv) for k, vv in ref.items()}
    eng = _engine(cfg, params)
    enc, dec = eng.enc, eng.dec
    for s, lr in enumerate(rates):
        vals64, _ = O.train_step(ref, m, v, cfg, x, cond, eps, coins, lr, dtype=torch.float64, **HYPER)
        out = eng.train_step(x, cond, eps, coins, lr=lr, lr_device=True, **HYPER)
        torch.cuda.synchronize()
        want = float(vals64["total_loss"])
        assert abs(float(out["total_loss"]) - want) <= 1e-4 * max(1.0, abs(want)), (s, float(out["total_loss"]), want)
        assert float(out["lr"]) == np.float32(lr)
    eng.check_gates()
    for name in ref:
        mod, pn = name.split(".", 1)
        st = enc if mod == "encoder" else dec
        for buf, r, what in ((st.flat, ref, "p"), (st.adam_m, m, "m"), (st.adam_v, v, "v")):
            got = st._view(buf, pn).cpu().numpy()
            if np.abs(r[name]).max() == 0.0:
                assert np.abs(got).max() == 0.0, (name, what)
                continue
            assert rel_err(got, r[name]) < 1e-4, (name, what, rel_err(got, r[name]))


# ---- data parallelism: two ranks on one MI355X (tests/test_grad_clip_gpu.py's pattern) ----------------------------------
DP_RATES = [1e-3, 2e-4, 5e-4]


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
    from arcvae_hip.dp import EngineDataParallel
    params, x, cond, eps, coins = make_case(TINY, B, T, 0.6)
    eng, enc, dec = build_engine(TINY, params)
    dpx = EngineDataParallel(eng)
    applied = []
    for lr in DP_RATES:
        ws = dpx.train_step(x, cond, eps, coins, lr, clip_norm=clip, lr_device=True, **HYPER)
        torch.cuda.synchronize()
        applied.append(ws.scalars[[13, 15]].cpu().numpy().copy())
    ret[f"r{rank}"] = dict(applied=np.stack(applied), drivers=np.array(len(dpx._drivers)),
                           **{f"{tag}_{b}": getattr(st, b).cpu().numpy()
                              for tag, st in (("enc", enc), ("dec", dec)) for b in ("flat", "adam_m", "adam_v")})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("with_clip", [False, True], ids=["no_clip", "clip"])
def test_two_ranks_device_rate_equal_single_process(with_clip):
    B, T, world = 8, 12, 2
    params, x, cond, eps, coins = make_case(TINY, B, T, 0.6)
    eng, enc, dec = build_engine(TINY, params)
    eng.train_step(x, cond, eps, coins, lr=LR, update=False, **HYPER)
    torch.cuda.synchronize()
    clip = 0.1 * _norm64([enc.grad.cpu().numpy(), dec.grad.cpu().numpy()]) if with_clip else None
    for lr in DP_RATES:
        eng.train_step(x, cond, eps, coins, lr=lr, clip_norm=clip, lr_device=True, **HYPER)
    torch.cuda.synchronize()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_dp_worker, args=(world, _free_port(), B, T, clip, ret), nprocs=world, join=True)
    r0, r1 = ret["r0"], ret["r1"]
    for k in r0:                                   # same reduced gradients, same word -> the same update on every rank
        assert np.array_equal(r0[k], r1[k]), k
    assert int(r0["drivers"]) == 1                 # one driver for the three rates
    assert np.array_equal(r0["applied"][:, 0], np.array(DP_RATES, dtype=np.float32)) and np.all(r0["applied"][:, 1] == 0.0)
    for tag, st in (("enc", enc), ("dec", dec)):
        for b in ("flat", "adam_m", "adam_v"):
            assert rel_err(r0[f"{tag}_{b}"], getattr(st, b).cpu().numpy()) < 1e-5, (tag, b)


# ---- trainer and CLI ------------------------------------------------------------------------------------------------------
def test_train_cli_schedule_history_checkpoint_and_resume(tmp_path):
    import train
    from lr_schedule import LRSchedule
    base = ["--synthetic", "256", "--epochs", "2", "--batch_size", "64", "--lr_schedule", "cosine", "--warmup_steps", "2",
            "--no_progress", "--checkpoint_freq", "1"]
    tr = train.main(base + ["--checkpoint_dir", str(tmp_path / "a")])
    # 204 training rows: four steps per epoch (the last one ragged), N = 2 * (204 // 64) = 6
    sch = LRSchedule(2e-4, "cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.0)
    assert tr.lr_schedule.state() == sch.state() and tr.global_step == 8
    assert tr.history["learning_rate"] == [sch.lr(3), sch.lr(7)]
    ck = np.load(sorted(glob.glob(str(tmp_path / "a" / "checkpoint_epoch_*.npz")))[-1], allow_pickle=False)
    assert int(ck["global_step"]) == 8 and int(ck["epoch"]) == 1
    # one epoch, then --resume for the second: the curve continues where it stopped
    first = tmp_path / "a" / "checkpoint_epoch_000.npz"
    assert int(np.load(first, allow_pickle=False)["global_step"]) == 4
    os.makedirs(tmp_path / "b")
    shutil.copy(first, tmp_path / "b" / "checkpoint_best.npz")
    tr2 = train.main(base + ["--checkpoint_dir", str(tmp_path / "b"), "--resume"])
    assert tr2.global_step == 8 and tr2.history["learning_rate"] == tr.history["learning_rate"]
    assert tr2.history["epoch"] == [0, 1]
