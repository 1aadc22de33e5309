"""N independent draws per batch row on the GPU (csrc/sample.hip arcvae_dec_sample_draws; an extension with no reference behaviour
to match): draw 0 against the existing list walk bit for bit, every draw against a NumPy replay of the kernels' own rows
(tests/draws_ref.py), prefix stability in N, the pad mode, the distribution of the draws and their independence, the model-level
surface and the argument errors."""
import numpy as np
import pytest
import torch

import arcvae_oracle as O
import draws_ref as D
import trunc_ref as R
from helpers import TINY, dev as _dev, lib as _lib, ws_bytes
from test_trunc_gpu import _rows, _seed, _tables, _vae, _walk, _walk_table

pytestmark = pytest.mark.gpu
END = 2
DENSE, DRAWS = "arcvae_dec_forward_dense", "arcvae_dec_sample_draws"


def _table(B, V, rs):
    """[B*V, V] logits: the row kinds of test_trunc_gpu._tables (random, flat, dominant, duplicated, underflowing), shuffled so
    that every batch row's chain meets each kind."""
    rows, _ = _tables(V, (B * V + 3) // 4, rs)
    return _dev(rows[rs.permutation(len(rows))[:B * V]], torch.float32)


def _draws(table_d, B, N, V, Tn, min_len=0, temp=1.0, k=0, p=1.0, mp=0.0, tp=1.0, seed=0, end=END, pad=-1):
    L = _lib()
    tok = torch.full((B, N, Tn), -7, dtype=torch.int32, device="cuda")
    fe = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    sd = _seed(seed)
    ws = torch.empty(ws_bytes("sample_draws", B, V, int(k), int(min_len)), dtype=torch.uint8, device="cuda")
    L.call(DRAWS, L.ptr(table_d), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws.numel(), B, N, V, Tn, int(min_len), int(end), int(pad),
           float(temp), int(k), float(p), float(mp), float(tp), L.ptr(sd), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), fe.cpu().numpy()


@pytest.mark.parametrize("V,Tn,kw,min_len", [(80, 128, dict(k=20, p=0.9), 0), (80, 64, dict(k=20, p=0.9, mp=0.1), 10),
                                             (80, 64, dict(tp=0.9), 0), (256, 40, dict(), 0),      # V 256: lists read through L2
                                             (3, 16, dict(), 0)])
def test_draw_zero_is_the_existing_walk(V, Tn, kw, min_len):
    B = 5                                                            # not a multiple of the 4 rows a workgroup of the old walk takes
    table_d = _table(B, V, np.random.RandomState(V + Tn))
    for seed in (0, 2 ** 64 - 5):
        want_t, want_f = _walk(table_d, B, V, Tn, min_len, 1.0, seed=seed, **kw)
        for N in (1, 67):                                            # 67 crosses a wave
            tok, fe = _draws(table_d, B, N, V, Tn, min_len, seed=seed, **kw)
            assert tok.min() >= 0 and tok.max() < V
            np.testing.assert_array_equal(tok[:, 0, :], want_t)
            np.testing.assert_array_equal(fe[:, 0], want_f)


@pytest.mark.parametrize("V,Tn,N,B,kw,min_len", [(80, 40, 300, 2, dict(k=20, p=0.9), 0), (256, 16, 70, 2, dict(), 0),
                                                 (80, 32, 130, 3, dict(), 8)])
def test_every_draw_is_the_replay_of_the_kernels_rows(V, Tn, N, B, kw, min_len):
    table_d = _walk_table(B, V, np.random.RandomState(V + N), END)
    pc, pt, pm, _, _ = _rows(table_d, V, 1.0, ban=-1, **kw)
    bc, bt, bm, _, _ = _rows(table_d, V, 1.0, ban=END, **kw)
    tok, fe = _draws(table_d, B, N, V, Tn, min_len, seed=11, **kw)
    rtok, rfe = D.walk(lambda r: (pc[r], pt[r], pm[r]), lambda r: (bc[r], bt[r], bm[r]), B, N, V, Tn, min_len, 11, END)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(fe, rfe)
    assert (tok[:, :, :min_len] != END).all()
    assert len({tok[b, d].tobytes() for b in range(B) for d in range(N)}) > B * N // 2      # draws are not copies


def test_prefix_stability_and_repeatability():
    B, V, Tn = 3, 80, 32
    table_d = _table(B, V, np.random.RandomState(5))
    kw = dict(k=20, p=0.9, seed=3, min_len=4)
    t67, f67 = _draws(table_d, B, 67, V, Tn, **kw)
    t300, f300 = _draws(table_d, B, 300, V, Tn, **kw)               # other workgroups, other lanes: the same draws
    np.testing.assert_array_equal(t67, t300[:, :67])
    np.testing.assert_array_equal(f67, f300[:, :67])
    again_t, again_f = _draws(table_d, B, 300, V, Tn, **kw)
    assert again_t.tobytes() == t300.tobytes() and again_f.tobytes() == f300.tobytes()


@pytest.mark.parametrize("V,min_len,kw", [(80, 0, dict(p=0.9)), (80, 5, dict()), (256, 0, dict())])
def test_pad_mode(V, min_len, kw):
    B, N, Tn = 2, 200, 48
    table = (np.random.RandomState(V).standard_normal((B * V, V)) * 1.5).astype(np.float32)
    table[:, END] += 2.5 + np.log(V / 80.0)                         # the end token carries real mass: most draws end early
    table_d = _dev(table, torch.float32)
    t0, f0 = _draws(table_d, B, N, V, Tn, min_len, seed=9, **kw)
    t7, f7 = _draws(table_d, B, N, V, Tn, min_len, seed=9, pad=7, **kw)
    np.testing.assert_array_equal(f0, f7)
    assert (f0 < Tn // 2).mean() > 0.5 and ((f0 == Tn).any() or f0.max() > 2 * np.median(f0))     # most end early, some late
    after = np.arange(Tn)[None, None, :] > f0[:, :, None]
    np.testing.assert_array_equal(t7[~after], t0[~after])
    assert (t7[after] == 7).all()
    assert ((t0 == END).argmax(2)[f0 < Tn] == f0[f0 < Tn]).all()


def _bound(p, n):
    return 5.0 * np.sqrt(p * (1.0 - p) / n) + 1e-3


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(min_p=0.1), dict()])
def test_first_token_distribution_is_the_truncated_softmax(kw):
    V, N = 80, 20000
    table = (np.random.RandomState(80).standard_normal((V, V)) * 1.5).astype(np.float32)
    tok, _ = _draws(_dev(table, torch.float32), 1, N, V, 2, p=kw.get("top_p", 1.0), mp=kw.get("min_p", 0.0), seed=21)
    want = R.truncated_probs(table[0], 1.0, 0, kw.get("top_p", 1.0), kw.get("min_p", 0.0))
    f = np.bincount(tok[0, :, 0], minlength=V) / N
    print("worst |f - p| / bound:", float((np.abs(f - want) / _bound(want, N)).max()), "kept", int((want > 0).sum()))
    assert not f[want == 0].any()                                    # no token outside the kept set is ever drawn
    assert (np.abs(f - want) <= _bound(want, N)).all()


def test_consecutive_draws_are_independent():
    V, N = 3, 20000
    table = np.array([[0.3, -0.2, 0.1]] * V, np.float32)
    tok, _ = _draws(_dev(table, torch.float32), 1, N, V, 2, seed=22, end=-1)
    first = tok[0, :, 0]
    p = R.truncated_probs(table[0], 1.0)
    f = np.bincount(first, minlength=V) / N
    assert (np.abs(f - p) <= _bound(p, N)).all()
    pairs = N // 2                                                   # (draw 2i, draw 2i + 1): disjoint pairs
    joint = np.bincount(first[0::2] * V + first[1::2], minlength=V * V).reshape(V, V) / pairs
    q = np.outer(p, p)
    print("worst joint |f - p p| / bound:", float((np.abs(joint - q) / _bound(q, pairs)).max()))
    assert (np.abs(joint - q) <= _bound(q, pairs)).all()


def test_model_path(monkeypatch):
    cfg, B, N, Tn = TINY, 3, 50, 24
    params = O.init_params(cfg, 1234)
    params["decoder.fc_out.bias"][END] += 2.0                        # molecules that end, and ones that do not
    vae = _vae(cfg, params)
    samp = vae.decoder_sampling
    cond = np.random.RandomState(2).standard_normal((B, cfg.C)).astype(np.float32)
    L = _lib()
    real, names = L.check, []

    def recorder(rc, what):
        if not what.endswith("_ws_bytes"):
            names.append(what)
        real(rc, what)

    monkeypatch.setattr(L, "check", recorder)
    kw = dict(max_length=Tn, top_p=0.9, early_stopping=False)
    tok, lengths = samp.generate_many(cond, N, seed=1, **kw)
    assert names == [DENSE, DRAWS, DENSE, DRAWS]                     # eagerly, then under capture
    assert tuple(tok.shape) == (B, N, Tn) and tok.dtype == torch.int32
    assert tuple(lengths.shape) == (B, N) and lengths.dtype == torch.int32
    tok, lengths = tok.cpu().numpy(), lengths.cpu().numpy()
    assert lengths.min() >= 1 and lengths.max() <= Tn and (lengths < Tn).any()
    for b in range(B):
        for d in range(N):
            n = lengths[b, d]
            assert (tok[b, d, :n - 1] != END).all() and (tok[b, d, n:] == samp.pad_token).all()
            assert tok[b, d, n - 1] == END or n == Tn
    names.clear()
    outs = {seed: samp.generate_many(cond, N, seed=seed, **kw)[0].cpu().numpy() for seed in (2, 2 ** 63 + 9)}
    assert names == []                                               # replays: nothing launched from Python
    assert (outs[2] != tok).any() and (outs[2] != outs[2 ** 63 + 9]).any()
    for seed, got in outs.items():
        eager = samp.generate_many(cond, N, seed=seed, use_graph=False, **kw)[0].cpu().numpy()
        np.testing.assert_array_equal(got, eager)
    assert names == [DENSE, DRAWS] * 2
    cut, cut_len = samp.generate_many(cond, N, seed=1, max_length=Tn, top_p=0.9)
    assert cut.shape[2] == int(cut_len.max()) and cut.is_contiguous()
    np.testing.assert_array_equal(cut.cpu().numpy(), tok[:, :, :cut.shape[2]])
    # one draw per row is the existing sampler's molecule for the same seed, up to each row's end
    one, one_len = samp.generate_many(cond, 1, seed=5, **kw)
    old = samp.generate_with_temperature(None, cond, max_length=Tn, sample=True, seed=5, top_p=0.9, early_stopping=False)
    one, one_len, old = one.cpu().numpy(), one_len.cpu().numpy(), old.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(one[b, 0, :one_len[b, 0]], old[b, :one_len[b, 0]])
    via = vae.generate(B, cond, max_length=Tn, sample=True, num_draws=3, top_k=5)
    assert via.dim() == 3 and tuple(via.shape[:2]) == (B, 3) and 1 <= via.shape[2] <= Tn
    for bad in (dict(num_draws=3), dict(sample=True, num_draws=3, beam_width=4), dict(sample=True, num_draws=3, exact=True),
                dict(sample=True, num_draws=3, num_best=2), dict(sample=True, num_draws=3, num_samples=2),
                dict(sample=True, num_draws=3, length_penalty=1.0), dict(sample=True, num_draws=0)):
        with pytest.raises(ValueError):
            vae.generate(B, cond, max_length=Tn, **bad)
    for bad in (dict(num_draws=0), dict(num_draws=2, min_p=1.0), dict(num_draws=2, typical_p=0.9, top_p=0.9),
                dict(num_draws=2, min_length=Tn + 1), dict(num_draws=2, top_k=0), dict(num_draws=2, temperature=0.0)):
        with pytest.raises(ValueError):
            samp.generate_many(cond, max_length=Tn, **bad)


def test_argument_errors():
    L = _lib()
    lib = L.load()
    B, N, V, Tn = 4, 3, 12, 8
    table = torch.zeros(B * V, V, device="cuda")
    tok = torch.full((B, N, Tn), -7, dtype=torch.int32, device="cuda")
    fe = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    sd = torch.zeros(1, dtype=torch.int64, device="cuda")
    one = ws_bytes("sample_draws", B, V, 3, 0)
    assert one == B * V * (4 + 3 * 5) and ws_bytes("sample_draws", B, V, 3, 2) == 2 * one
    ws = torch.empty(2 * one, dtype=torch.uint8, device="cuda")

    def draws(table=table, tok=tok, fe=fe, ws=ws, ws_bytes=2 * one, B_=B, N_=N, V_=V, Tn_=Tn, min_len=2, end=END, pad=-1, temp=1.0,
              seed=sd):
        return lib.arcvae_dec_sample_draws(L.ptr(table), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws_bytes, B_, N_, V_, Tn_, min_len, end,
                                           pad, temp, 3, 1.0, 0.0, 1.0, L.ptr(seed), L.stream_ptr())

    for bad in (dict(N_=0), dict(ws_bytes=2 * one - 1), dict(min_len=0, ws_bytes=one - 1), dict(table=None), dict(tok=None),
                dict(fe=None), dict(ws=None), dict(seed=None), dict(pad=256), dict(pad=-2), dict(min_len=Tn + 1),
                dict(min_len=1, end=-1), dict(min_len=1, end=V), dict(N_=2 ** 30), dict(temp=float("nan"))):
        assert draws(**bad) == -1, bad
    torch.cuda.synchronize()
    assert (tok == -7).all() and (fe == -7).all()                    # nothing was launched
    assert draws() == 0 and draws(min_len=0, ws_bytes=one, end=-5, pad=255) == 0
    torch.cuda.synchronize()
    assert int(tok.min()) >= 0 and int(tok.max()) < V and (fe == Tn).all()
