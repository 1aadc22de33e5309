"""Every tick of the encoder LSTM sweeps against the fp64 per-tick restatement (tests/lstm_ticks.py), form by form.

The step-level tests see the sweeps through mu / logvar / z and the parameter gradients, which are sums over t: at the default
init most ticks' gate gradients are far too small to move those sums, so a wrong ring slot, a bad hand-off across a chunk
relaunch or a misplaced time range would pass them.  Here each case runs one training step (update=False) through the engine,
with the knobs set before it is built, reads hseq, cseq, the gate gradients dG and dh_top = dcomb[:, :H], and checks

  (a) h and c of every tick from the GPU's own previous states (forward_local);
  (b) with ARCVAE_INPLACE_DG=0, the saved gates gseq (the BPTT's input) the same way;
  (c) the o-gate quarter of dG[l, t] from the GPU's own dG^l[t+1], dG^{l+1}[t] (dgo_local);
  (d) all of dG, chained in fp64 from the GPU's forward states (bptt);
  (e) the stack's parameter gradients against fp64 sums over the GPU's own dG and h, at the element-wise step bar.

(a)-(d) are judged per tick: |got - ref| <= 1e-4*|ref| + 4e-6*max|ref[l, t]| (lstm_ticks.tick_check).  Every case runs at the
default init and under lstm_ticks.long_memory, where every tick's gate gradient stays within a few percent of the largest
one and no tick may fall below the checker's floor.  Every case also asserts that the form it names is the one that ran."""
import os

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import lstm_ticks as K
from helpers import DEFAULT, ELEM_ATOL_GRAD, HYPER, assert_elem, build_engine, make_case

pytestmark = pytest.mark.gpu


def _lib():
    from arcvae_hip import _lib
    return _lib.load()


def _E():
    from arcvae_hip import engine
    return engine


def _cfg(H, L):
    return O.Config(vocab_size=60, embedding_dim=32, hidden_dim=H, latent_dim=16, num_conditions=1, num_layers=L)


def _edge_rows(B: int) -> np.ndarray:
    """First and last row of every XCD slice (ceil(B/8) rows), of every 64-row tile and of the 16-row groups in the first and
    last XCD slice, plus the ragged tail."""
    rows = {B - 1}
    xs = -(-B // 8)
    for size, lo, hi in ((xs, 0, B), (64, 0, B), (16, 0, min(B, xs)), (16, max(0, B - xs), B)):
        for s in range(lo - lo % size, hi, size):
            rows.update((max(s, lo), min(s + size, hi) - 1))
    return np.array(sorted(rows))


def _check(tag, eng, enc, cfg, params, x, ws, rows, inplace_dg=True):
    """(a)-(e) for the step that just ran; returns the worst per-tick ratio of each check."""
    L, H = cfg.L, cfg.H
    full = len(rows) == ws.B
    ri = torch.as_tensor(rows, device=ws.hseq.device)
    take = (lambda a: a.cpu().numpy()) if full else (lambda a: a.index_select(2, ri).cpu().numpy())
    hs, cs = take(ws.hseq), take(ws.cseq)
    dG = take(ws.dG)
    dh_top = ws.dcomb[:, :H].index_select(0, ri).cpu().numpy()
    long_mem = tag == "long_memory"
    out = {}

    h, c, gates = K.forward_local(params, x, hs, cs, rows)
    for name, got, ref in (("h", hs, h), ("c", cs, c)):
        out[name] = K.tick_check(got, ref)
    if not inplace_dg:
        out["gates"] = K.tick_check(take(ws.gseq), gates)
    out["dGo_local"] = K.tick_check(dG[..., 3 * H:], K.dgo_local(params, x, hs, cs, dG, dh_top, rows, gates=gates))
    out["dG"] = K.tick_check(dG, K.bptt(params, x, hs, cs, dh_top, rows, gates=gates))
    for name, rep in out.items():
        assert rep.worst <= 1.0, f"{tag}: {name}: {rep}"
        if long_mem:
            assert rep.skipped == 0, f"{tag}: {name}: {rep}"

    # (e): fp64 sums over the GPU's own dG and h of every row, formed on the device
    ref = K.wgrad_from(params, x, ws.hseq, ws.dG)
    worst = 0.0
    for name, r in ref.items():
        got = enc.g(name.split(".", 1)[1]).cpu().numpy()
        worst = max(worst, assert_elem(got, r.cpu().numpy(), f"{tag}: grad {name}", ELEM_ATOL_GRAD))
    del ref
    ratios = {k: round(v.worst, 4) for k, v in out.items()}
    ratios["dG_ticks_skipped"] = out["dG"].skipped
    ratios["wgrad_elem"] = round(worst, 4)
    return ratios


def _run(cfg, B, T, rows=None, expect=None, inplace_dg=True, tf=0.6):
    """One step at the default init and one under long_memory on the same engine (knobs already set); `expect(eng, enc, ws)`
    asserts the form under test."""
    params, x, cond, eps, coins = make_case(cfg, B, T, tf)
    eng, enc, dec = build_engine(cfg, params)
    ws = eng.workspace(B, T)
    if expect is not None:
        expect(eng, enc, ws)
    assert (ws.dG is ws.gseq) == inplace_dg
    rows = np.arange(B) if rows is None else rows
    res = {}
    for tag, p in (("default", params), ("long_memory", K.long_memory(params, cfg))):
        enc.load_state_dict(p, prefix="encoder.")
        eng.train_step(x, cond, eps, coins, lr=2e-4, update=False, **HYPER)
        torch.cuda.synchronize()
        eng.check_gates()
        assert eng.workspace(B, T) is ws
        res[tag] = _check(tag, eng, enc, cfg, p, x, ws, rows, inplace_dg)
    print(f"\n[ticks] {os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]}: {res}")
    del eng, enc, dec, ws
    torch.cuda.empty_cache()
    return res


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---- the default step (H 256, L 2, B 64, T 128, all rows) in each of its forms -------------------------------------------
def _persistent(eng, enc, ws, bwd="rs", n_chunks=None, fused=False):
    E, lib, d = _E(), _lib(), eng.d
    assert E.persistent_forward_ok(ws, d) and lib.arcvae_enc_lstm_persist_groups(ws.B, d.H, d.L) == 1
    plan = E.EncoderBackwardPlan(enc, ws, d)
    assert plan.persistent == (bwd == "rs") and E.bptt_reduce_scatter_ok(ws, d) == (bwd == "rs")
    assert (lib.arcvae_enc_lstm_bwd_persistent_ok(ws.B, ws.T, d.H, d.L) == 1) == (bwd == "persistent")
    assert plan.fused == fused
    if n_chunks is not None:
        assert len(plan.chunks) == n_chunks
    return plan


DEFAULT_FORMS = {
    "layer_split": ({}, dict(n_chunks=2)),
    "one_chain": ({"ARCVAE_LAYER_SPLIT": "0"}, dict(n_chunks=2)),
    "persistent_bwd_output_split": ({"ARCVAE_PERSIST_BWD": "1"}, dict(bwd="persistent", n_chunks=4)),
    "bwd_launches": ({"ARCVAE_PERSIST_BWD": "0"}, dict(bwd="launches", n_chunks=4)),
    "fused_wgrad": ({"ARCVAE_FUSED_WGRAD": "1"}, dict(fused=True, n_chunks=1)),
    "eight_chunks": ({"ARCVAE_BPTT_CHUNKS": "0.1,0.2,0.3,0.4,0.5,0.6,0.7,1.0"}, dict(n_chunks=8)),
}


@pytest.mark.parametrize("form", list(DEFAULT_FORMS) + ["no_persistent"])
def test_default_step_every_tick(form, monkeypatch):
    cfg, B, T = DEFAULT, 64, 128
    if form == "no_persistent":
        monkeypatch.setenv("ARCVAE_PERSIST", "0")

        def expect(eng, enc, ws):
            E, lib, d = _E(), _lib(), eng.d
            assert not E.persistent_forward_ok(ws, d) and not E.bptt_reduce_scatter_ok(ws, d)
            assert lib.arcvae_enc_lstm_bwd_persistent_ok(B, T, d.H, d.L) == 0
            assert len(E.EncoderBackwardPlan(enc, ws, d).chunks) == 4
    else:
        env, kw = DEFAULT_FORMS[form]
        _set(monkeypatch, env)

        def expect(eng, enc, ws):
            _persistent(eng, enc, ws, **kw)
    _run(cfg, B, T, expect=expect, tf=0.9)


def test_saved_gates_every_tick(monkeypatch):
    """ARCVAE_INPLACE_DG=0: the gate gradients get their own buffer, so the saved gates the BPTT reads are checked too."""
    monkeypatch.setenv("ARCVAE_INPLACE_DG", "0")
    _run(DEFAULT, 64, 128, expect=lambda eng, enc, ws: _persistent(eng, enc, ws, n_chunks=2), inplace_dg=False, tf=0.9)


# ---- ring wraps: the dc / dX / operand rings hold min(T, 16) slots (ARCVAE_RING) ------------------------------------------
@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("T,ring", [(16, None), (17, None), (33, None), (13, "4")])
def test_ring_wraps_every_tick(T, ring, persist, monkeypatch):
    monkeypatch.setenv("ARCVAE_PERSIST", persist)
    if ring is not None:
        monkeypatch.setenv("ARCVAE_RING", ring)
    slots = min(T, int(ring or 16))

    def expect(eng, enc, ws):
        E = _E()
        assert E.persistent_forward_ok(ws, eng.d) == (persist == "1")
        assert ws.dcs.shape[1] == slots and ws.dxs.shape[1] == slots
    _run(_cfg(256, 2), 64, T, expect=expect)


# ---- row partitions of the persistent sweeps over the XCDs ----------------------------------------------------------------
ROW_CASES = [
    # (knobs, H, B, two-group forward, BPTT form)
    ({}, 256, 1, False, "rs"), ({}, 256, 3, False, "rs"), ({}, 256, 9, False, "rs"), ({}, 256, 63, False, "rs"),
    ({}, 256, 65, False, "rs"), ({}, 256, 130, True, "launches"), ({}, 256, 200, True, "launches"),
    ({}, 256, 256, True, "launches"),
    ({}, 128, 3, False, "launches"), ({}, 128, 65, False, "launches"), ({}, 128, 200, False, "launches"),
    ({}, 384, 9, False, "launches"), ({}, 384, 63, False, "launches"),
    ({"ARCVAE_PERSIST2": "3"}, 256, 130, True, "rs"), ({"ARCVAE_PERSIST2": "3"}, 256, 200, True, "rs"),
    ({"ARCVAE_PERSIST2": "3"}, 256, 256, True, "rs"),
    ({"ARCVAE_PERSIST2": "0", "ARCVAE_RS_MAX_B": "256"}, 256, 130, False, "rs"),
    ({"ARCVAE_PERSIST2": "0", "ARCVAE_RS_MAX_B": "256"}, 256, 256, False, "rs"),
    ({"ARCVAE_PERSIST2": "0", "ARCVAE_RS_MAX_B": "256", "ARCVAE_RS_R16": "0"}, 256, 200, False, "rs"),
    ({"ARCVAE_RS_HALVES": "1"}, 256, 130, True, "halves"), ({"ARCVAE_RS_HALVES": "1"}, 256, 256, True, "halves"),
    ({"ARCVAE_RS_HALVES": "1", "ARCVAE_PERSIST2": "0"}, 256, 200, False, "halves"),
]


@pytest.mark.parametrize("env,H,B,two,bwd", ROW_CASES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else None)
def test_row_partitions_every_tick(env, H, B, two, bwd, monkeypatch):
    _set(monkeypatch, env)
    L, T = 2 if H < 384 else 1, 21

    def expect(eng, enc, ws):
        E, lib, d = _E(), _lib(), eng.d
        assert E.persistent_forward_ok(ws, d)
        assert (lib.arcvae_enc_lstm_persist_groups(B, H, L) == 2) == two
        assert E.bptt_reduce_scatter_ok(ws, d) == (bwd in ("rs", "halves"))
        assert (lib.arcvae_enc_lstm_bwd_rs_halves(B, T, H, L) == 1) == (bwd == "halves")
    _run(_cfg(H, L), B, T, expect=expect)


# ---- the register-tiled step kernels (tile regime), forced on at small shapes ----------------------------------------------
TILE_CASES = [
    # (knobs, H, L, B, T)
    ({"ARCVAE_STEP_TILE": "1", "ARCVAE_LSTM_SPLIT3": "1"}, 64, 3, 37, 20),
    ({"ARCVAE_STEP_TILE": "1", "ARCVAE_LSTM_SPLIT3": "0"}, 192, 1, 130, 40),
    ({"ARCVAE_STEP_TILE": "2", "ARCVAE_LSTM_SPLIT3": "1"}, 192, 4, 130, 20),
    ({"ARCVAE_STEP_TILE": "2", "ARCVAE_LSTM_SPLIT3": "0"}, 64, 1, 288, 40),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_LSTM_SPLIT3": "1"}, 256, 3, 288, 20),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_LSTM_SPLIT3": "0"}, 64, 4, 37, 40),
    ({"ARCVAE_STEP_TILE": "44", "ARCVAE_LSTM_SPLIT3": "1"}, 192, 3, 288, 40),
    ({"ARCVAE_STEP_TILE": "44", "ARCVAE_LSTM_SPLIT3": "0"}, 256, 1, 37, 20),
    ({"ARCVAE_STEP_TILE": "22", "ARCVAE_LSTM_SPLIT3": "1"}, 256, 4, 130, 20),
    ({"ARCVAE_STEP_TILE": "22", "ARCVAE_LSTM_SPLIT3": "0"}, 256, 3, 288, 40),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_BWD_KSPLIT3": "2"}, 192, 3, 130, 20),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_BWD_KSPLIT3": "2"}, 256, 1, 288, 40),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_BWD_KSPLIT3": "0"}, 64, 4, 288, 20),
    ({"ARCVAE_STEP_TILE": "4", "ARCVAE_BWD_KSPLIT3": "0"}, 256, 3, 37, 40),
]


@pytest.mark.parametrize("env,H,L,B,T", TILE_CASES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else None)
def test_tile_regime_every_tick(env, H, L, B, T, monkeypatch):
    monkeypatch.setenv("ARCVAE_PERSIST", "0")      # (else the persistent sweeps take the shapes they cover)
    _set(monkeypatch, env)

    def expect(eng, enc, ws):
        E, lib, d = _E(), _lib(), eng.d
        assert not E.persistent_forward_ok(ws, d) and not E.bptt_reduce_scatter_ok(ws, d)
        assert E._lstm_flags(ws) == (0 if env.get("ARCVAE_LSTM_SPLIT3") == "0" else _lib_mod().LSTM_SPLIT3)
        assert lib.arcvae_enc_lstm_tiled_for(B, H, L, E._lstm_flags(ws)) == (0 if env["ARCVAE_STEP_TILE"] == "22" else 3)
    _run(_cfg(H, L), B, T, expect=expect)


def _lib_mod():
    from arcvae_hip import _lib
    return _lib


# ---- full size: a row subset at the edges of every XCD slice and row tile ----------------------------------------------------
@pytest.mark.parametrize("cfg,B", [(DEFAULT, 256), (DEFAULT, 2048),
                                   (O.Config(vocab_size=80, embedding_dim=128, hidden_dim=512, latent_dim=256,
                                             num_conditions=1, num_layers=4), 512)],
                         ids=["default_b256", "default_b2048", "configs2"])
def test_full_size_every_tick(cfg, B):
    T = 128

    def expect(eng, enc, ws):
        E, lib, d = _E(), _lib(), eng.d
        tiled = lib.arcvae_enc_lstm_tiled_for(B, d.H, d.L, E._lstm_flags(ws))
        if B == 256:
            assert E.persistent_forward_ok(ws, d) and lib.arcvae_enc_lstm_persist_groups(B, d.H, d.L) == 2 and tiled == 0
        else:
            assert not E.persistent_forward_ok(ws, d) and tiled == 3
    _run(cfg, B, T, rows=_edge_rows(B), expect=expect, tf=0.9)
