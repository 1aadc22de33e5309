"""Min-p, locally typical and minimum-length truncated sampling on the GPU (csrc/sample.hip; an extension with no reference
behaviour to match): the materialised rows against the fp64 restatement (tests/trunc_ref.py), identity with the top-k / top-p
entry points where the new rules are off, the walk bit for bit against a NumPy replay of the kernels' own rows, and the
model-level surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import topkp_ref as T
import trunc_ref as R
from helpers import TINY, dev as _dev, lib as _lib, ws_bytes

pytestmark = pytest.mark.gpu
END = 2
DENSE, TRUNC = "arcvae_dec_forward_dense", "arcvae_dec_sample_chain_trunc"


def _vae(cfg, params):          # the sampler's own decoder loaded directly, the rest left as drawn
    from models.vae import ARCVAE
    vae = ARCVAE(vocab_size=cfg.V, embedding_dim=cfg.E, hidden_dim=cfg.H, latent_dim=cfg.Z, num_conditions=cfg.C,
                 num_layers=cfg.L)
    vae.decoder_sampling.decoder.load_state_dict(params, prefix="decoder.")
    return vae


def _rows(table_d, V, temp, k=0, p=1.0, mp=0.0, tp=1.0, ban=-1, rows=None):
    """arcvae_dec_trunc_rows -> (count [R], tokens [R, V], cum [R, V], dev [R, V], ent [R]) as NumPy."""
    L = _lib()
    Rn = table_d.shape[0] if rows is None else len(rows)
    rows_d = None if rows is None else _dev(rows, torch.int32)
    cnt = torch.full((Rn,), -7, dtype=torch.int32, device="cuda")
    tok = torch.full((Rn, V), -7, dtype=torch.int32, device="cuda")
    cum = torch.full((Rn, V), -7.0, dtype=torch.float32, device="cuda")
    dv = torch.full((Rn, V), -7.0, dtype=torch.float32, device="cuda")
    ent = torch.full((Rn,), -7.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_trunc_rows", L.ptr(table_d), table_d.shape[0], L.ptr(rows_d), Rn, V, float(temp), int(k), float(p), float(mp),
           float(tp), int(ban), L.ptr(cnt), L.ptr(tok), L.ptr(cum), L.ptr(dv), L.ptr(ent), L.stream_ptr())
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), tok.cpu().numpy(), cum.cpu().numpy(), dv.cpu().numpy(), ent.cpu().numpy()


def _seed(seed):
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device="cuda")


def _walk(table_d, B, V, Tn, min_len, temp, k=0, p=1.0, mp=0.0, tp=1.0, seed=0, end=END):
    L = _lib()
    tok = torch.full((B, Tn), -7, dtype=torch.int32, device="cuda")
    fe = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    sd = _seed(seed)
    ws = torch.empty(ws_bytes("trunc", B, V, int(k), int(min_len)), dtype=torch.uint8, device="cuda")
    L.call("arcvae_dec_sample_chain_trunc", L.ptr(table_d), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws.numel(), B, V, Tn, int(min_len),
           int(end), float(temp), int(k), float(p), float(mp), float(tp), L.ptr(sd), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), fe.cpu().numpy()


def _tables(V, n, rs):
    """n rows of each kind (the recipe of the top-k / top-p test): random, flat, one dominant token, duplicated logits at the
    k = 5 and k = V - 1 boundaries; and one random row with a -200 logit, whose mass underflows to 0"""
    rnd = rs.standard_normal((n, V)).astype(np.float32) * 2
    flat = np.full((n, V), 0.25, np.float32)
    dom = rs.standard_normal((n, V)).astype(np.float32)
    dom[np.arange(n), rs.randint(V, size=n)] += 25
    dup = rs.standard_normal((n, V)).astype(np.float32) * 2
    for r in dup:
        o = T.order(r)
        for a, b in ((4, 5), (V - 2, V - 1)):
            if 0 <= a < b < V:
                r[o[b]] = r[o[a]]
    low = rs.standard_normal((1, V)).astype(np.float32) * 2
    low[0, V // 2] = -200.0
    return np.concatenate([rnd, flat, dom, dup, low]), ["random"] * n + ["flat"] * n + ["dominant"] * n + ["dup"] * n + ["low"]


@pytest.mark.parametrize("V", [3, 80, 255, 256])
def test_rows_against_the_fp64_restatement(V):
    rs = np.random.RandomState(V)
    table, kinds = _tables(V, 16, rs)
    table_d = _dev(table, torch.float32)
    temp = 0.7
    S = T.scaled(table, temp)
    boundary = {"min_p": 0, "typical": 0}
    rows_total = {"min_p": 0, "typical": 0}
    worst_dev = worst_ent = 0.0
    for ban in (-1, 2):
        orders = np.stack([R.order(s, ban) for s in S])
        spos = np.argsort(orders, axis=1)                            # spos[i, token] = the token's position in the s-order
        for k in sorted({2, 5, V - 1, V, V + 7}):
            for mp, p in [(mp, p) for mp in (0.01, 0.05, 0.1, 0.5) for p in (0.9, 1.0)]:
                cnt, tok, cum, dv, ent = _rows(table_d, V, temp, k, p, mp, 1.0, ban)
                np.testing.assert_array_equal(tok, orders)           # the whole order, exactly (the banned token last)
                assert not dv.any() and not ent.any()                # written, as 0
                for i, s in enumerate(S):
                    r = R.truncate(s, k, p, mp, 1.0, ban)
                    assert 1 <= cnt[i] <= r.K
                    np.testing.assert_array_equal(cum[i, r.K:], 0)
                    np.testing.assert_allclose(cum[i, :r.K], r.C, rtol=1e-5, atol=0)
                    rows_total["min_p"] += kinds[i] != "flat"
                    if cnt[i] != r.n:
                        assert R.is_min_p_boundary(r, min(cnt[i], r.n)) or (p < 1 and T.is_boundary(r.before, r.thr)), \
                            (ban, k, mp, p, i, kinds[i], cnt[i], r.n)
                        boundary["min_p"] += kinds[i] != "flat"
            for tp in (0.2, 0.5, 0.9, 0.95):
                cnt, tok, cum, dv, ent = _rows(table_d, V, temp, k, 1.0, 0.0, tp, ban)
                for i, s in enumerate(S):
                    r = R.truncate(s, k, 1.0, 0.0, tp, ban)
                    K = r.K
                    assert 1 <= cnt[i] <= K
                    assert sorted(tok[i, :K]) == sorted(orders[i, :K])            # a permutation of the exact top-k set
                    np.testing.assert_array_equal(tok[i, K:], orders[i, K:])      # then the rest of the s-order
                    # the order is EXACTLY the sort of the kernel's own d: d ascending, ties to the earlier s-position
                    d32, sp = dv[i, :K], spos[i, tok[i, :K]]
                    assert np.all((d32[1:] > d32[:-1]) | ((d32[1:] == d32[:-1]) & (sp[1:] > sp[:-1]))), (ban, k, tp, i, kinds[i])
                    np.testing.assert_array_equal(dv[i, K:], 0)
                    np.testing.assert_array_equal(cum[i, K:], 0)
                    # d and H against fp64, token by token, inside the operation-count bound
                    at = np.argsort(r.tokens[:K])[np.searchsorted(np.sort(r.tokens[:K]), tok[i, :K])]   # ref position of each token
                    frac = np.abs(d32.astype(np.float64) - r.d[at]) / R.dev_bound(r)[at]
                    worst_dev = max(worst_dev, float(frac.max()))
                    worst_ent = max(worst_ent, abs(float(ent[i]) - r.H) / R.ent_bound(r))
                    assert frac.max() < 1 and abs(float(ent[i]) - r.H) < R.ent_bound(r), (ban, k, tp, i, kinds[i], frac.max())
                    np.testing.assert_allclose(cum[i, :K], np.cumsum(r.e[at]), rtol=1e-5, atol=0)
                    rows_total["typical"] += kinds[i] != "flat"
                    if set(tok[i, :cnt[i]].tolist()) != set(r.tokens[:r.n].tolist()):
                        assert R.is_typical_boundary(r), (ban, k, tp, i, kinds[i], cnt[i], r.n)
                        boundary["typical"] += kinds[i] != "flat"
    print(f"V {V}: worst |dev - d64| / bound {worst_dev:.4f}, worst |ent - H| / bound {worst_ent:.4f}, boundary rows {boundary} of "
          f"{rows_total}")
    # (flat rows put a threshold on an integer prefix mass by construction; on the other tables a boundary decision is rare)
    for fam in boundary:
        assert boundary[fam] <= max(2, rows_total[fam] // 50), (fam, boundary, rows_total)


def _walk_table(B, V, rs, end):
    table = (rs.standard_normal((B * V, V)) * 1.5).astype(np.float32)
    table[:, end] += 1.0                                             # rows end early: a minimum length shows
    return _dev(table, torch.float32)


@pytest.mark.parametrize("V,Tn,k,p", [(80, 128, 20, 0.9), (256, 40, 0, 1.0)])
def test_identity_with_topkp_where_the_new_rules_are_off(V, Tn, k, p):
    L = _lib()
    B = 37
    table_d = _walk_table(B, V, np.random.RandomState(V), END)
    cnt, tok, cum, _, _ = _rows(table_d, V, 1.0, k, p)
    c0 = torch.full((B * V,), -7, dtype=torch.int32, device="cuda")
    t0 = torch.full((B * V, V), -7, dtype=torch.int32, device="cuda")
    m0 = torch.full((B * V, V), -7.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_topkp_rows", L.ptr(table_d), B * V, None, B * V, V, 1.0, k, p, L.ptr(c0), L.ptr(t0), L.ptr(m0), L.stream_ptr())
    torch.cuda.synchronize()
    assert cnt.tobytes() == c0.cpu().numpy().tobytes()
    assert tok.tobytes() == t0.cpu().numpy().tobytes()
    assert cum.tobytes() == m0.cpu().numpy().tobytes()
    ws = torch.empty(ws_bytes("topkp", B, V, k), dtype=torch.uint8, device="cuda")
    for seed in (0, 11, 2 ** 64 - 5):
        wt = torch.full((B, Tn), -7, dtype=torch.int32, device="cuda")
        wf = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        L.call("arcvae_dec_sample_chain_topkp", L.ptr(table_d), L.ptr(wt), L.ptr(wf), L.ptr(ws), ws.numel(), B, V, Tn, END, 1.0, k, p,
               L.ptr(_seed(seed)), L.stream_ptr())
        torch.cuda.synchronize()
        got_t, got_f = _walk(table_d, B, V, Tn, 0, 1.0, k, p, seed=seed)
        np.testing.assert_array_equal(got_t, wt.cpu().numpy())
        np.testing.assert_array_equal(got_f, wf.cpu().numpy())


@pytest.mark.parametrize("V,Tn,min_len,k,p,mp,tp", [(80, 128, 0, 0, 1.0, 0.05, 1.0), (80, 64, 10, 20, 0.9, 0.1, 1.0),
                                                    (256, 40, 40, 0, 1.0, 0.0, 0.9), (80, 1, 1, 5, 1.0, 0.0, 0.5),
                                                    (2, 16, 7, 0, 1.0, 0.0, 1.0)])
def test_walk_is_the_replay_of_its_rows(V, Tn, min_len, k, p, mp, tp):
    B = 37                                                           # not a multiple of the block's 4 rows
    end = min(END, V - 1)
    table_d = _walk_table(B, V, np.random.RandomState(V + Tn), end)
    pc, pt, pm, _, _ = _rows(table_d, V, 1.0, k, p, mp, tp, -1)
    bc, bt, bm, _, _ = _rows(table_d, V, 1.0, k, p, mp, tp, end)
    assert (bt[:, -1] == end).all() and not any(end in bt[i, :bc[i]] for i in range(B * V))
    for seed in (0, 11, 2 ** 64 - 5):
        tok, fe = _walk(table_d, B, V, Tn, min_len, 1.0, k, p, mp, tp, seed, end)
        rtok, rfe = R.walk(lambda r: (pc[r], pt[r], pm[r]), lambda r: (bc[r], bt[r], bm[r]), B, V, Tn, min_len, seed, end)
        np.testing.assert_array_equal(tok, rtok)
        np.testing.assert_array_equal(fe, rfe)
        again, _ = _walk(table_d, B, V, Tn, min_len, 1.0, k, p, mp, tp, seed, end)
        assert again.tobytes() == tok.tobytes()
        assert (tok[:, :min_len] != end).all() and (fe >= min_len).all()      # no end token before min_len
        if min_len == Tn:
            assert (fe == Tn).all()
    if min_len and Tn > 1:                                           # the mask did something: without it rows end earlier
        assert (_walk(table_d, B, V, Tn, 0, 1.0, k, p, mp, tp, 0, end)[1] < min_len).any()


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


@pytest.fixture(scope="module")
def dist_case():
    return _dist_case()


def _check_hist(first, want, V, B):
    h = np.bincount(first, minlength=V)
    assert 0.5 * np.abs(h / B - want).sum() < 0.06, 0.5 * np.abs(h / B - want).sum()
    exp = B * want
    big = exp >= 5
    chi2 = (((h - exp) ** 2)[big] / exp[big]).sum()
    assert chi2 < 3.0 * big.sum() + 30, (chi2, int(big.sum()))


def test_limits(dist_case):
    cfg, _, vae, cond, _ = dist_case
    samp = vae.decoder_sampling
    L = _lib()
    Bs, Tn = 256, 24
    cond = cond[:Bs] + np.random.RandomState(9).standard_normal((Bs, cfg.C)).astype(np.float32)
    kw = dict(max_length=Tn, early_stopping=False, sample=True)
    # a low temperature for min_p: the kept tokens are those within T * 1e-4 of the largest logit, i.e. the largest alone
    mp = samp.generate_with_temperature(None, cond, temperature=0.05, seed=4, min_p=0.9999, **kw).cpu().numpy()
    ws = samp.decoder.workspace(Bs, Tn)
    tok = torch.empty(Bs, Tn, dtype=torch.int32, device="cuda")
    fe = torch.empty(Bs, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_sample_chain", L.ptr(ws.nxt), L.ptr(tok), L.ptr(fe), Bs, cfg.V, Tn, END, L.stream_ptr())
    greedy0 = tok.cpu().numpy()                                      # the walk over mode 0's first-argmax table
    np.testing.assert_array_equal(mp, greedy0)
    ty1 = samp.generate_with_temperature(None, cond, temperature=1.0, seed=5, typical_p=1e-9, top_k=1, **kw).cpu().numpy()
    np.testing.assert_array_equal(ty1, greedy0)
    # typical_p -> 0 alone: the most typical token of every visited row, position 0 of its typical order
    ty = samp.generate_with_temperature(None, cond, temperature=1.0, seed=6, typical_p=1e-9, **kw).cpu().numpy()
    prev = np.concatenate([np.zeros((Bs, 1), np.int32), ty[:, :-1]], axis=1)
    ids = (np.arange(Bs)[:, None] * cfg.V + prev).reshape(-1).astype(np.int32)
    cnt, rtok, _, _, _ = _rows(samp.decoder.workspace(Bs, Tn).logits, cfg.V, 1.0, tp=1e-9, rows=ids)
    assert (cnt == 1).all()
    np.testing.assert_array_equal(ty.reshape(-1), rtok[:, 0])
    assert (ty != greedy0).any()                                     # the most typical token is not the most likely one


@pytest.mark.parametrize("kw", [dict(min_p=0.1), dict(typical_p=0.9), dict(top_k=5, typical_p=0.9), dict(top_p=0.9, min_p=0.05)])
def test_first_step_distribution_is_the_truncated_softmax(dist_case, kw):
    cfg, B, vae, cond, logits0 = dist_case
    samp = vae.decoder_sampling
    temp = 0.02
    toks = samp.generate_with_temperature(None, cond, max_length=3, temperature=temp, early_stopping=False, sample=True, seed=11,
                                          **kw).cpu().numpy()
    assert toks.min() >= 0 and toks.max() < cfg.V
    args = (kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("min_p", 0.0), kw.get("typical_p", 1.0))
    _check_hist(toks[:, 0], R.truncated_probs(logits0, temp, *args), cfg.V, B)
    assert len(np.unique(toks[:, 0])) > 1
    # support: every first token lies in the fp64 kept set of its own table row (the kernel's fp32 logits, s bit-exact)
    rows0 = samp.decoder.workspace(B, 3).logits.view(B, cfg.V, cfg.V)[:, 0, :].cpu().numpy()    # row b*V + 0: after the start token
    S = T.scaled(rows0, temp)
    outside = 0
    for b in range(B):
        r = R.truncate(S[b], *args)
        if toks[b, 0] not in r.tokens[:r.n]:
            if r.typical:
                assert R.is_typical_boundary(r), b
            else:
                assert R.is_min_p_boundary(r, r.n) or (args[1] < 1 and T.is_boundary(r.before, r.thr)), b
            outside += 1
    assert outside <= B // 100


def test_model_graph_replay_and_launches(monkeypatch):
    """generate_with_temperature(min_p / typical_p / min_length): the graph replay with a new seed equals the eager call with that
    seed, without a new capture; a first call launches dense + walk twice (eagerly, then under capture), a replay nothing."""
    cfg, B, Tn = TINY, 67, 40
    vae = _vae(cfg, O.init_params(cfg, 1234))
    samp = vae.decoder_sampling
    cond = np.random.RandomState(2).standard_normal((B, cfg.C)).astype(np.float32)
    L = _lib()
    real, names = L.check, []

    def recorder(rc, what):
        if not what.endswith("_ws_bytes"):
            names.append(what)
        real(rc, what)

    monkeypatch.setattr(L, "check", recorder)
    for kw in (dict(min_p=0.05, top_k=10), dict(typical_p=0.9), dict(top_p=0.9, min_length=7)):
        kw = dict(max_length=Tn, temperature=0.05, early_stopping=False, sample=True, **kw)
        n_before = len(samp._graphs)
        names.clear()
        first = samp.generate_with_temperature(None, cond, seed=1, **kw).cpu().numpy()     # eager, then captured
        assert names == [DENSE, TRUNC, DENSE, TRUNC]
        assert len(samp._graphs) == n_before + 1
        names.clear()
        outs = {seed: samp.generate_with_temperature(None, cond, seed=seed, **kw).cpu().numpy() for seed in (2, 3, 2 ** 63 + 9)}
        assert names == [] and len(samp._graphs) == n_before + 1     # replays: nothing launched from Python, no new capture
        for seed, got in outs.items():
            eager = samp.generate_with_temperature(None, cond, seed=seed, use_graph=False, **kw).cpu().numpy()
            np.testing.assert_array_equal(got, eager)
        assert names == [DENSE, TRUNC] * 3
        assert (outs[2] != outs[3]).any()
        np.testing.assert_array_equal(samp.generate_with_temperature(None, cond, seed=1, **kw).cpu().numpy(), first)
        if kw.get("min_length"):
            assert (first[:, :7] != END).all()
    # the existing paths are not rerouted: min_p = None, typical_p = None, min_length = 0 is the top-k / top-p call
    names.clear()
    samp.generate_with_temperature(None, cond, max_length=Tn, sample=True, top_k=5, min_p=None, typical_p=None, min_length=0)
    assert names == [DENSE, "arcvae_dec_sample_chain_topkp"] * 2


def test_model_value_errors_and_early_stopping():
    cfg, Bm = TINY, 6
    params = O.init_params(cfg, 1234)
    params["decoder.fc_out.bias"][2] = 50.0                          # a decoder that always emits EOS where it may
    vae = _vae(cfg, params)
    cond = np.zeros((Bm, cfg.C), np.float32)
    samp = vae.decoder_sampling
    for kw in (dict(min_p=0.1), dict(typical_p=0.9), dict(min_length=3), dict(min_p=1.0, sample=True), dict(min_p=-0.1, sample=True),
               dict(typical_p=0.0, sample=True), dict(typical_p=1.5, sample=True), dict(typical_p=0.9, top_p=0.9, sample=True),
               dict(typical_p=0.9, min_p=0.1, sample=True), dict(min_length=21, sample=True), dict(min_length=-1, sample=True)):
        with pytest.raises(ValueError):
            samp.generate_with_temperature(None, cond, max_length=20, **kw)
    for kw in (dict(beam_width=4, min_p=0.1), dict(exact=True, typical_p=0.9), dict(sample=True, num_samples=2, min_length=3),
               dict(min_p=0.1), dict(beam_width=4, min_length=2)):
        with pytest.raises(ValueError):
            vae.generate(Bm, cond, max_length=20, **kw)
    got = samp.generate_with_temperature(None, cond, max_length=20, sample=True, seed=3, min_length=5)
    assert tuple(got.shape) == (Bm, 6) and (got[:, :5] != END).all() and (got[:, 5] == END).all()
    off = samp.generate_with_temperature(None, cond, max_length=20, sample=True, seed=3, min_p=0.0, typical_p=1.0)
    assert tuple(off.shape) == (Bm, 1) and int(off.min()) == END     # 0.0 and 1.0 mean off
    via = vae.generate(Bm, cond, max_length=20, sample=True, seed=3, min_p=0.1, min_length=5)
    assert tuple(via.shape) == (Bm, 6)
    via = vae.generate(Bm, cond, max_length=20, sample=True, seed=3, typical_p=0.9, top_k=5)
    assert tuple(via.shape) == (Bm, 1)


def test_argument_errors():
    L = _lib()
    lib = L.load()
    B, V, Tn = 4, 12, 8
    table = torch.zeros(B * V, V, device="cuda")
    tok = torch.zeros(B, Tn, dtype=torch.int32, device="cuda")
    fe = torch.zeros(B, dtype=torch.int32, device="cuda")
    sd = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(B * V, dtype=torch.int32, device="cuda")
    rt = torch.zeros(B * V, V, dtype=torch.int32, device="cuda")
    rc = torch.zeros(B * V, V, device="cuda")
    n = C.c_long(0)
    one = B * V * (4 + 3 * 5)
    assert lib.arcvae_dec_trunc_ws_bytes(B, V, 3, 0, C.byref(n)) == 0 and n.value == one
    assert lib.arcvae_dec_trunc_ws_bytes(B, V, 3, 2, C.byref(n)) == 0 and n.value == 2 * one
    assert lib.arcvae_dec_trunc_ws_bytes(B, V, 0, 8, C.byref(n)) == 0 and n.value == 2 * B * V * (4 + V * 5)
    assert lib.arcvae_dec_trunc_ws_bytes(B, V, -1, 0, C.byref(n)) == -1 and lib.arcvae_dec_trunc_ws_bytes(B, 257, 0, 0, C.byref(n)) == -1
    assert lib.arcvae_dec_trunc_ws_bytes(B, V, 3, -1, C.byref(n)) == -1
    ws = torch.empty(2 * one, dtype=torch.uint8, device="cuda")

    def walk(V_=V, temp=1.0, k=3, p=1.0, mp=0.0, tp=1.0, min_len=2, end=END, seed=sd, ws_bytes=ws.numel()):
        return lib.arcvae_dec_sample_chain_trunc(L.ptr(table), L.ptr(tok), L.ptr(fe), L.ptr(ws), ws_bytes, B, V_, Tn, min_len, end,
                                                 temp, k, p, mp, tp, L.ptr(seed), L.stream_ptr())

    def rows(V_=V, temp=1.0, k=3, p=1.0, mp=0.0, tp=1.0, ban=-1, R_=B * V):
        return lib.arcvae_dec_trunc_rows(L.ptr(table), B * V, None, R_, V_, temp, k, p, mp, tp, ban, L.ptr(cnt), L.ptr(rt), L.ptr(rc),
                                         None, None, L.stream_ptr())

    for bad in (dict(k=-1), dict(p=0.0), dict(p=1.0001), dict(p=float("nan")), dict(V_=257), dict(temp=0.0), dict(mp=-0.01),
                dict(mp=1.0), dict(mp=float("nan")), dict(tp=0.0), dict(tp=1.0001), dict(tp=float("nan")), dict(tp=0.9, p=0.9),
                dict(tp=0.9, mp=0.1)):
        assert walk(**bad) == -1 and rows(**bad) == -1, bad
    for bad in (dict(min_len=-1), dict(min_len=Tn + 1), dict(min_len=1, end=-1), dict(min_len=1, end=V), dict(min_len=1, V_=1, end=0),
                dict(seed=None), dict(ws_bytes=2 * one - 1), dict(min_len=1, ws_bytes=one), dict(k=4)):
        assert walk(**bad) == -1, bad
    for bad in (dict(ban=-2), dict(ban=V), dict(ban=0, V_=1), dict(R_=B * V + 1)):
        assert rows(**bad) == -1, bad
    assert walk() == 0 and walk(min_len=0, ws_bytes=one) == 0 and walk(min_len=0, end=-5) == 0 and rows() == 0 and rows(ban=0) == 0
    torch.cuda.synchronize()
    assert cnt.min().item() == 3 and cnt.max().item() == 3          # a flat table: K = 3, every position passes min_p = 0
    assert rows(mp=0.5, tp=1.0) == 0 and rows(tp=0.5) == 0
    torch.cuda.synchronize()
    assert cnt.min().item() == 2 and cnt.max().item() == 2          # typical_p 0.5 of three equal masses: before = 0, 1 < 1.5
