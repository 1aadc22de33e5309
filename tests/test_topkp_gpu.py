"""Top-k / nucleus (top-p) truncated sampling on the GPU (csrc/sample.hip; an extension with no reference behaviour to match):
the materialised rows against the fp64 restatement (tests/topkp_ref.py), the walk bit for bit against a NumPy replay of the
kernels' own rows and the splitmix64 generator, the model-level surface against the oracle's truncated softmax."""
import ctypes as C

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import topkp_ref as R
from helpers import DEFAULT, TINY, dev as _dev, lib as _lib, ws_bytes

pytestmark = pytest.mark.gpu
END = 2


def _vae(cfg, params):          # (not helpers.sampling_vae: the sampler's own decoder loaded directly, the rest left as drawn)
    from models.vae import ARCVAE
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    vae.decoder_sampling.decoder.load_state_dict(params, prefix="decoder.")
    return vae


def _rows(table_d, V, temp, k, p, rows=None):
    """arcvae_dec_topkp_rows -> (count [R], tokens [R, V], cum [R, V]) as NumPy."""
    L = _lib()
    Rn = table_d.shape[0] if rows is None else len(rows)
    rows_d = None if rows is None else _dev(rows, torch.int32)
    cnt = torch.full((Rn,), -7, dtype=torch.int32, device="cuda")
    tok = torch.full((Rn, V), -7, dtype=torch.int32, device="cuda")
    cum = torch.full((Rn, V), -7.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_topkp_rows", L.ptr(table_d), table_d.shape[0], L.ptr(rows_d), Rn, V, float(temp), int(k), float(p),
           L.ptr(cnt), L.ptr(tok), L.ptr(cum), L.stream_ptr())
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), tok.cpu().numpy(), cum.cpu().numpy()


def _ws(B, V, k):
    return torch.empty(ws_bytes("topkp", B, V, int(k)), dtype=torch.uint8, device="cuda")


def _walk(table_d, B, V, T, temp, k, p, seed):
    L = _lib()
    tok = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    fe = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    sd = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device="cuda")
    ws = _ws(B, V, k)
    L.call("arcvae_dec_sample_chain_topkp", L.ptr(table_d), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws.numel(), B, V, T, END, float(temp),
           int(k), float(p), L.ptr(sd), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), fe.cpu().numpy()


def _tables(V, n, rs):
    """n rows of each kind: random, flat, one dominant token, duplicated logits at the k = 5 and k = V - 1 boundaries"""
    rnd = rs.standard_normal((n, V)).astype(np.float32) * 2
    flat = np.full((n, V), 0.25, np.float32)
    dom = rs.standard_normal((n, V)).astype(np.float32)
    dom[np.arange(n), rs.randint(V, size=n)] += 25
    dup = rs.standard_normal((n, V)).astype(np.float32) * 2
    for r in dup:
        o = R.order(r)
        for a, b in ((4, 5), (V - 2, V - 1)):
            if 0 <= a < b < V:
                r[o[b]] = r[o[a]]
    return np.concatenate([rnd, flat, dom, dup]), ["random"] * n + ["flat"] * n + ["dominant"] * n + ["dup"] * n


@pytest.mark.parametrize("V", [3, 80, 255, 256])
def test_rows_against_the_fp64_restatement(V):
    rs = np.random.RandomState(V)
    n = 16
    table, kinds = _tables(V, n, rs)
    table_d = _dev(table, torch.float32)
    temp = 0.7
    S = R.scaled(table, temp)
    orders = np.stack([R.order(s) for s in S])
    boundary_total = rows_total = 0
    for k in sorted({1, 2, 5, max(V - 1, 1), V, V + 7}):
        for p in (1e-6, 0.5, 0.9, 0.999, 1.0):
            cnt, tok, cum = _rows(table_d, V, temp, k, p)
            np.testing.assert_array_equal(tok, orders)               # the whole order, exactly
            for i, s in enumerate(S):
                o, K, e, Cr, nr, before, thr = R.truncate(s, k, p)
                assert 1 <= cnt[i] <= K
                np.testing.assert_array_equal(cum[i, K:], 0)
                np.testing.assert_allclose(cum[i, :K], Cr, rtol=1e-5, atol=0)
                if kinds[i] != "flat":
                    rows_total += 1
                if cnt[i] != nr:
                    assert R.is_boundary(before, thr), (k, p, i, kinds[i], cnt[i], nr)
                    if kinds[i] != "flat":
                        boundary_total += 1
    # (flat rows put the threshold on an integer prefix mass by construction; on the other tables a boundary decision is rare)
    assert boundary_total <= max(2, rows_total // 50), (boundary_total, rows_total)


def test_rows_listed_ids_and_repeatability():
    rs = np.random.RandomState(1)
    V = 80
    table = rs.standard_normal((2 * V, V)).astype(np.float32)
    table_d = _dev(table, torch.float32)
    ids = np.array([7, 0, 159, 7, 42], np.int32)
    a = _rows(table_d, V, 1.3, 20, 0.9, ids)
    b = _rows(table_d, V, 1.3, 20, 0.9)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y[ids])
    c = _rows(table_d, V, 1.3, 20, 0.9)
    for x, y in zip(b, c):
        assert x.tobytes() == y.tobytes()                         # bitwise repeatable


def _replay(table_d, B, V, T, temp, k, p, seed):
    cnt, tok, cum = _rows(table_d, V, temp, k, p)
    return R.walk(lambda r: (cnt[r], tok[r], cum[r]), B, V, T, seed, END)


@pytest.mark.parametrize("V,T,k,p", [(80, 128, 20, 0.9), (80, 1, 0, 0.5), (256, 128, 5, 1.0), (256, 40, 0, 0.9),
                                     (80, 64, 0, 1.0)])
def test_walk_is_the_replay_of_its_rows(V, T, k, p):
    rs = np.random.RandomState(V + T)
    B = 37                                                           # not a multiple of the block's 4 rows
    table = (rs.standard_normal((B * V, V)) * 1.5).astype(np.float32)
    table[:, END] -= 2.0
    table_d = _dev(table, torch.float32)
    for seed in (0, 11, 2 ** 64 - 5):
        tok, fe = _walk(table_d, B, V, T, 1.0, k, p, seed)
        rtok, rfe = _replay(table_d, B, V, T, 1.0, k, p, seed)
        np.testing.assert_array_equal(tok, rtok)
        np.testing.assert_array_equal(fe, rfe)
        again, _ = _walk(table_d, B, V, T, 1.0, k, p, seed)
        assert again.tobytes() == tok.tobytes()
    assert (_walk(table_d, B, V, T, 1.0, k, p, 12)[0] != tok).any() or T == 1 or p < 1e-3


def test_model_walk_graph_replay_and_seed():
    """generate_with_temperature(top_k / top_p): the graph replay with a new seed equals the eager call with that seed, without a
    new capture; both are the replay of the table the pass wrote."""
    cfg, B, T = TINY, 67, 40
    params = O.init_params(cfg, 1234)
    vae = _vae(cfg, params)
    samp = vae.decoder_sampling
    cond = np.random.RandomState(2).standard_normal((B, cfg.C)).astype(np.float32)
    kw = dict(max_length=T, temperature=0.05, early_stopping=False, sample=True, top_k=10, top_p=0.9)
    first = samp.generate_with_temperature(None, cond, seed=1, **kw).cpu().numpy()     # eager, then captured
    n_graphs = len(samp._graphs)
    outs = {}
    for seed in (2, 3, 2 ** 63 + 9):
        outs[seed] = samp.generate_with_temperature(None, cond, seed=seed, **kw).cpu().numpy()   # replays
        assert len(samp._graphs) == n_graphs
    for seed, got in outs.items():
        eager = samp.generate_with_temperature(None, cond, seed=seed, use_graph=False, **kw).cpu().numpy()
        np.testing.assert_array_equal(got, eager)
    assert len(samp._graphs) == n_graphs
    assert (outs[2] != outs[3]).any()
    np.testing.assert_array_equal(samp.generate_with_temperature(None, cond, seed=1, **kw).cpu().numpy(), first)
    table_d = samp.decoder.workspace(B, T).logits
    rtok, _ = _replay(table_d, B, cfg.V, T, 0.05, 10, 0.9, 2 ** 63 + 9)
    np.testing.assert_array_equal(outs[2 ** 63 + 9], rtok)


def _dist_case():
    cfg, B = TINY, 4096
    params = O.init_params(cfg, 1234)
    vae = _vae(cfg, params)
    cond1 = np.random.RandomState(3).standard_normal((1, cfg.C)).astype(np.float32)
    pd = {k[len("decoder."):]: torch.tensor(v, dtype=torch.float64) for k, v in params.items() if k.startswith("decoder.")}
    out = torch.cat([pd["embedding.weight"][torch.tensor([0])], torch.tensor(cond1, dtype=torch.float64)], dim=1)[:, None, :]
    for l in range(cfg.L):
        out, _ = O.mlx_lstm(out, pd[f"lstm_layer_{l}.Wx"], pd[f"lstm_layer_{l}.Wh"], pd[f"lstm_layer_{l}.bias"])
    logits0 = O.mlx_linear(out[:, 0, :], pd["fc_out.weight"], pd["fc_out.bias"])[0].numpy()   # oracle: after the start token
    return cfg, B, vae, np.repeat(cond1, B, axis=0), logits0


def _check_hist(first, want, V, B):
    h = np.bincount(first, minlength=V)
    assert 0.5 * np.abs(h / B - want).sum() < 0.06, 0.5 * np.abs(h / B - want).sum()
    exp = B * want
    big = exp >= 5
    chi2 = (((h - exp) ** 2)[big] / exp[big]).sum()
    assert chi2 < 3.0 * big.sum() + 30, (chi2, int(big.sum()))


@pytest.mark.parametrize("k,p", [(5, None), (None, 0.9), (5, 0.9)])
def test_first_step_distribution_is_the_truncated_softmax(k, p):
    cfg, B, vae, cond, logits0 = _dist_case()
    samp = vae.decoder_sampling
    temp = 0.02
    toks = samp.generate_with_temperature(None, cond, max_length=3, temperature=temp, early_stopping=False, sample=True, seed=11,
                                          top_k=k, top_p=p).cpu().numpy()
    assert toks.min() >= 0 and toks.max() < cfg.V
    want = R.truncated_probs(logits0, temp, k or 0, 1.0 if p is None else p)
    _check_hist(toks[:, 0], want, cfg.V, B)
    assert len(np.unique(toks[:, 0])) > 1
    # support: every first token lies in the fp64 truncated set of its own table row (the kernel's fp32 logits, s bit-exact)
    rows0 = samp.decoder.workspace(B, 3).logits.view(B, cfg.V, cfg.V)[:, 0, :].cpu().numpy()    # row b*V + 0: after the start token
    S = R.scaled(rows0, temp)
    outside = 0
    for b in range(B):
        o, K, e, Cr, n, before, thr = R.truncate(S[b], k or 0, 1.0 if p is None else p)
        if toks[b, 0] not in o[:n]:
            assert R.is_boundary(before, thr), b
            outside += 1
    assert outside <= B // 100


def test_limits():
    cfg, B, vae, cond, logits0 = _dist_case()
    samp = vae.decoder_sampling
    L = _lib()
    T = 24
    cond = cond[:256] + np.random.RandomState(9).standard_normal((256, cfg.C)).astype(np.float32)
    Bs = cond.shape[0]
    # T = 1, top_k = 1 (and top_p -> 0): the walk over mode 0's first-argmax table
    k1 = samp.generate_with_temperature(None, cond, max_length=T, temperature=1.0, early_stopping=False, sample=True, seed=4,
                                        top_k=1).cpu().numpy()
    ws = samp.decoder.workspace(Bs, T)
    tok = torch.empty(Bs, T, dtype=torch.int32, device="cuda")
    fe = torch.empty(Bs, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_sample_chain", L.ptr(ws.nxt), L.ptr(tok), L.ptr(fe), Bs, cfg.V, T, END, L.stream_ptr())
    greedy0 = tok.cpu().numpy()
    np.testing.assert_array_equal(k1, greedy0)
    p0 = samp.generate_with_temperature(None, cond, max_length=T, temperature=1.0, early_stopping=False, sample=True, seed=5,
                                        top_p=1e-9).cpu().numpy()
    np.testing.assert_array_equal(p0, greedy0)
    # top_k >= V with top_p = 1: the untruncated distribution, as sample=True
    temp = 0.02
    cond4 = np.repeat(cond[:1], B, axis=0)
    full = samp.generate_with_temperature(None, cond4, max_length=2, temperature=temp, early_stopping=False, sample=True, seed=6,
                                          top_k=cfg.V + 7, top_p=1.0).cpu().numpy()
    cat = samp.generate_with_temperature(None, cond4, max_length=2, temperature=temp, early_stopping=False, sample=True,
                                         seed=6).cpu().numpy()
    want = R.truncated_probs(samp.decoder.workspace(B, 2).logits[0].cpu().numpy(), temp)
    _check_hist(full[:, 0], want, cfg.V, B)
    _check_hist(cat[:, 0], want, cfg.V, B)
    # sample=True without the new arguments is still arcvae_dec_sample_chain_categorical on the same logits
    tok2 = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    fe2 = torch.empty(B, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_sample_chain_categorical", L.ptr(samp.decoder.workspace(B, 2).logits), L.ptr(tok2), L.ptr(fe2), B, cfg.V, 2,
           END, temp, C.c_ulonglong(6), L.stream_ptr())
    np.testing.assert_array_equal(cat, tok2.cpu().numpy())


def test_argument_errors_and_early_stopping():
    L = _lib()
    lib = L.load()
    B, V, T = 4, 12, 8
    table = torch.zeros(B * V, V, device="cuda")
    tok = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    fe = torch.zeros(B, dtype=torch.int32, device="cuda")
    sd = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(B * V, dtype=torch.int32, device="cuda")
    rt = torch.zeros(B * V, V, dtype=torch.int32, device="cuda")
    rc = torch.zeros(B * V, V, device="cuda")

    ws = _ws(B, V, 3)
    n = C.c_long(0)
    assert lib.arcvae_dec_topkp_ws_bytes(B, V, 3, C.byref(n)) == 0 and n.value == B * V * (4 + 3 * 5)
    assert lib.arcvae_dec_topkp_ws_bytes(B, V, -1, C.byref(n)) == -1 and lib.arcvae_dec_topkp_ws_bytes(B, 257, 0, C.byref(n)) == -1

    def walk(V_=V, temp=1.0, k=3, p=0.9, seed=sd, ws_bytes=ws.numel()):
        return lib.arcvae_dec_sample_chain_topkp(L.ptr(table), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws_bytes, B, V_, T, END, temp, k,
                                                 p, L.ptr(seed), L.stream_ptr())

    def rows(V_=V, temp=1.0, k=3, p=0.9, R_=B * V):
        return lib.arcvae_dec_topkp_rows(L.ptr(table), B * V, None, R_, V_, temp, k, p, L.ptr(cnt), L.ptr(rt), L.ptr(rc),
                                         L.stream_ptr())

    for bad in (dict(k=-1), dict(p=0.0), dict(p=1.0001), dict(p=float("nan")), dict(V_=257), dict(temp=0.0)):
        assert walk(**bad) == -1 and rows(**bad) == -1, bad
    assert walk(seed=None) == -1 and rows(R_=B * V + 1) == -1
    assert walk(ws_bytes=ws.numel() - 1) == -1 and walk(k=4) == -1       # top_k 4 needs more than the top_k 3 workspace
    assert walk() == 0 and rows() == 0
    torch.cuda.synchronize()
    assert cnt.min().item() == 3 and cnt.max().item() == 3          # a flat table: K = 3, every position inside the nucleus at 0.9
    # model level: ValueErrors, and early stopping cuts where every row ended (a decoder that always emits EOS first)
    cfg, Bm = TINY, 6
    params = O.init_params(cfg, 1234)
    params["decoder.fc_out.bias"][2] = 50.0
    vae = _vae(cfg, params)
    cond = np.zeros((Bm, cfg.C), np.float32)
    samp = vae.decoder_sampling
    for kw in (dict(top_k=5), dict(top_p=0.5), dict(top_k=0, sample=True), dict(top_p=0.0, sample=True),
               dict(top_p=1.5, sample=True)):
        with pytest.raises(ValueError):
            samp.generate_with_temperature(None, cond, max_length=20, **kw)
    with pytest.raises(ValueError):
        vae.generate(Bm, cond, max_length=20, beam_width=4, top_k=5)
    with pytest.raises(ValueError):
        vae.generate(Bm, cond, max_length=20, beam_width=4, top_p=0.5)
    got = samp.generate_with_temperature(None, cond, max_length=20, sample=True, seed=3, top_k=5)
    assert tuple(got.shape) == (Bm, 1) and int(got.min()) == 2
    full = samp.generate_with_temperature(None, cond, max_length=20, sample=True, seed=3, top_p=0.9, early_stopping=False)
    assert tuple(full.shape) == (Bm, 20)                                # tokens after EOS are still generated
    via = vae.generate(Bm, cond, max_length=20, sample=True, seed=3, top_k=5, top_p=0.9)
    assert tuple(via.shape) == (Bm, 1)


def test_configs4_shape_draws_stay_in_the_kept_sets():
    """Default dims, bs 1024, max_length 80: every drawn token is among the kept tokens of its (batch row, previous token) row."""
    cfg, B, T = DEFAULT, 1024, 80
    params = O.init_params(cfg, 7)
    vae = _vae(cfg, params)
    samp = vae.decoder_sampling
    cond = np.random.RandomState(0).standard_normal((B, cfg.C)).astype(np.float32)
    for k, p in ((20, None), (None, 0.9), (20, 0.9)):
        toks = samp.generate_with_temperature(None, cond, max_length=T, temperature=1.0, early_stopping=False, sample=True,
                                              seed=21, top_k=k, top_p=p).cpu().numpy()
        prev = np.concatenate([np.zeros((B, 1), np.int32), toks[:, :-1]], axis=1)
        ids = (np.arange(B)[:, None] * cfg.V + prev).reshape(-1).astype(np.int32)
        cnt, tok, _ = _rows(samp.decoder.workspace(B, T).logits, cfg.V, 1.0, k or 0, 1.0 if p is None else p, ids)
        kept = np.arange(cfg.V)[None, :] < cnt[:, None]
        hit = (tok == toks.reshape(-1)[:, None]) & kept
        assert hit.any(axis=1).all()
        if k:
            assert cnt.max() <= k
        assert len(np.unique(toks)) > 10
