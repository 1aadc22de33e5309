"""Exact MAP decoding and exact chain marginals on the GPU (csrc/chain.hip; an extension with no reference behaviour to match):
the Viterbi kernel against the fp32 NumPy restatement (tests/chain_ref.py) operation for operation, the marginals kernel against
the fp64 recursion, and the model-level surface (generate_map, token_marginals, length_distribution,
ARCVAE.generate(exact=True)) against the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import beam_ref as R
import chain_ref as X
from helpers import dev as _dev, ending_model, lib as _lib, ws_bytes

pytestmark = pytest.mark.gpu
END, PAD = 2, 0
U = 2.0 ** -24


def _viterbi(table_d, lse_d, B, V, T, min_len, temp, pad=PAD):
    L = _lib()
    n = ws_bytes("viterbi", B, V, T)
    assert n == B * T * V
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, dtype=torch.float32, device="cuda")
    ln = torch.empty(B, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_viterbi", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok), L.ptr(sc), L.ptr(ln), L.ptr(ws), n, B, V, T,
           min_len, END, pad, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), sc.cpu().numpy(), ln.cpu().numpy()


# (V, max_len, min_len, temperature, table, lowering of the end column): the tables of tests/chain_ref.make_table.  V below a
# wave, V no multiple of 64, V 256 (the table that is read through L2 instead of LDS), max_len 1 (no recursion), min_len = max_len
# (the end token never allowed), exact ties everywhere (q8), sequences that never end (the end column lowered by 4 * max_len: at
# about 2 nats per step, lowering it by 4 alone still ends after a few tokens -- those two cases run as well), back-traces of more
# than one staged chunk (V 80 x 128 steps, V 256 x 48 steps), and both sides of the staging threshold: V 96 (the largest staged
# table), V 97 and 130 (read through L2, V no multiple of 4: padded entries of the vector; V 97 in two parts, V 130 in one).
CASES = [(12, 1, 0, 1.0, "q8", 0), (12, 40, 0, 1.0, "q8", 0), (12, 30, 30, 0.7, "normal", 0), (80, 64, 5, 1.0, "normal", 0),
         (80, 128, 0, 1.0, "q8-lowered-end", 4 * 128), (256, 48, 2, 1.0, "q8", 0), (256, 16, 0, 1.3, "normal-lowered-end", 4 * 16),
         (80, 128, 0, 1.0, "q8-lowered-end", 4), (256, 16, 0, 1.3, "normal-lowered-end", 4), (256, 48, 48, 1.0, "q8", 0),
         (96, 6, 0, 1.0, "q8", 0), (97, 6, 1, 1.0, "normal", 0), (130, 8, 8, 1.0, "q8", 0)]


@pytest.mark.parametrize("V,T,min_len,temp,kind,lower", CASES)
def test_viterbi_kernel_is_the_fp32_restatement(V, T, min_len, temp, kind, lower):
    """Tokens and lengths equal; scores BIT-equal: every score is a chain of single IEEE fp32 operations (one multiply and one
    subtract per step term, one add per step) in the same order on both sides, with the same lse passed in -- nothing is
    reassociated, so there is no rounding difference to tolerate.  The sequence log-likelihood kernel returns the same bits."""
    B = 6
    table = X.make_table(np.random.RandomState(V * 1000 + T), B, V, kind, END, float(lower))
    lse = R.row_lse(table, temp).astype(np.float32)
    table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)
    tok, sc, ln = _viterbi(table_d, lse_d, B, V, T, min_len, temp)
    lp = R.step_terms(table, lse, temp)
    rtok, rsc, rln = X.viterbi(lp, B, V, T, min_len, END, PAD)
    np.testing.assert_array_equal(ln, rln)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    if lower > 4:
        assert np.sum(ln == T) >= B // 2, ln                    # (the unfinished branch and whole-length back-traces)
    if min_len == T:
        assert np.all(ln == T) and not np.any(tok == END)
    L = _lib()
    tok_d = _dev(tok, torch.int32)
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_sequence_logprob", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok_d), L.ptr(out), B, T, V, END, float(temp),
           L.stream_ptr())
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), sc.view(np.uint32))


def test_viterbi_pad_token_and_beam():
    """A pad token outside the vocabulary fills the positions after the end; the score is never below the beam kernel's best."""
    B, V, T, min_len, temp = 6, 80, 64, 5, 1.0
    table = X.make_table(np.random.RandomState(V * 1000 + T), B, V, "normal", END)
    lse = R.row_lse(table, temp).astype(np.float32)
    table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)
    tok, sc, ln = _viterbi(table_d, lse_d, B, V, T, min_len, temp, pad=255)
    for b in range(B):
        assert np.all(tok[b, ln[b]:] == 255) and np.all((tok[b, :ln[b]] >= 0) & (tok[b, :ln[b]] < V))
    L = _lib()
    K = 32
    n = C.c_long(0)
    L.call("arcvae_dec_beam_ws_bytes", B, K, T, C.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    btok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
    bsc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    bln = torch.empty(B, K, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_beam_search", L.ptr(table_d), L.ptr(lse_d), L.ptr(btok), L.ptr(bsc), L.ptr(bln), L.ptr(ws), n.value, B, V, K,
           T, min_len, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    assert np.all(sc >= bsc.cpu().numpy()[:, 0])


def _marginals(table_d, lse_d, B, V, T, temp):
    L = _lib()
    out = torch.full((B, T, V), -1.0, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_chain_marginals", L.ptr(table_d), L.ptr(lse_d), L.ptr(out), B, V, T, END, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V,T,temp", [(12, 16, 1.0), (12, 24, 0.7), (80, 12, 1.0), (256, 8, 1.3), (12, 1, 1.0),
                                      (96, 5, 1.0), (97, 5, 1.0), (130, 4, 0.7)])
def test_marginals_kernel_against_fp64(V, T, temp):
    """The fp64 recursion runs over the FP32 step terms (the same lse passed in, beam_ref.step_terms in fp32), so only expf, the
    products and the sums differ: per step at most (V + 8) * 2^-24 relative, for any order of V non-negative products."""
    B = 6
    table = X.make_table(np.random.RandomState(V * 10 + T), B, V, "normal", END)
    lse = R.row_lse(table, temp).astype(np.float32)
    table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)
    got = _marginals(table_d, lse_d, B, V, T, temp)
    again = _marginals(table_d, lse_d, B, V, T, temp)
    np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    ref = X.marginals(R.step_terms(table, lse, temp), B, V, T, END, np.float64)
    bound = np.broadcast_to((np.arange(T) + 1)[None, :, None] * (V + 8) * U, ref.shape)
    ok = ref >= 1e-30
    rel = np.abs(got.astype(np.float64) / np.where(ok, ref, 1.0) - 1.0)
    print("worst |got/ref - 1| / bound:", (rel / bound)[ok].max())
    assert np.all(rel[ok] <= bound[ok]), (rel / bound)[ok].max()
    assert np.all(got >= 0.0)
    total = X.length_distribution(got.astype(np.float64), END).sum(axis=1)
    rtotal = X.length_distribution(ref, END).sum(axis=1)
    assert np.all(np.abs(total - rtotal) <= T * T * (V + 8) * U * rtotal), np.abs(total - rtotal).max()


# ---- model level: TINY, B 64 ---------------------------------------------------------------------------------------------------
B_M, T_M = 64, 20


@pytest.fixture(scope="module")
def model():
    return ending_model(B_M, END)


@pytest.mark.parametrize("temp,min_len", [(1.0, 0), (0.5, 6)])
def test_generate_map_scores(model, temp, min_len):
    cfg, params, vae, cond, loglik = model
    samp = vae.decoder_sampling
    tok, sc = samp.generate_map(torch.zeros(B_M, cfg.Z), cond, max_length=T_M, temperature=temp, min_length=min_len)
    tok, sc = tok.cpu().numpy(), sc.cpu().numpy()
    assert tok.dtype == np.int32 and tok.shape[0] == B_M and 1 <= tok.shape[1] <= T_M and np.all(np.isfinite(sc))
    ends = tok == END
    first = np.where(ends.any(1), ends.argmax(1), tok.shape[1])
    assert np.all(first >= min_len)                            # min_length is honoured
    assert np.where(ends.any(1), first + 1, T_M).max() == tok.shape[1]      # early stopping: L = the longest returned sequence
    ref = loglik(params, cfg, cond, tok, temp)
    assert np.all(np.abs(sc - ref) <= 1e-4 * np.abs(ref)), np.abs(sc - ref).max()
    # the scores ARE the sequence log-likelihood of the tokens (same table, same lse, same order of additions)
    lpm = samp.decoder.sequence_log_prob(torch.as_tensor(tok), cond, temperature=temp).cpu().numpy()
    np.testing.assert_array_equal(lpm.view(np.uint32), sc.view(np.uint32))
    lpt = vae.decoder.sequence_log_prob(torch.as_tensor(tok), cond, temperature=temp).cpu().numpy()     # (the trained copy)
    np.testing.assert_array_equal(lpt.view(np.uint32), sc.view(np.uint32))
    # never below the widest beam, on every row
    _, bsc = samp.generate_beam(torch.zeros(B_M, cfg.Z), cond, max_length=T_M, beam_width=32, temperature=temp, min_length=min_len)
    assert np.all(sc >= bsc.cpu().numpy()[:, 0])
    full, sc2 = samp.generate_map(None, cond, max_length=T_M, temperature=temp, min_length=min_len, early_stopping=False)
    assert full.shape == (B_M, T_M) and np.array_equal(full.cpu().numpy()[:, :tok.shape[1]], tok)
    assert np.all(full.cpu().numpy()[:, tok.shape[1]:] == PAD)
    np.testing.assert_array_equal(sc2.cpu().numpy().view(np.uint32), sc.view(np.uint32))


def test_generate_exact(model):
    cfg, params, vae, cond, _ = model
    tok, _ = vae.decoder_sampling.generate_map(None, cond, max_length=16)
    got = vae.generate(B_M, cond, max_length=16, exact=True)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), tok.cpu().numpy())
    for bad in (dict(sample=True), dict(beam_width=4), dict(top_k=5), dict(top_p=0.9), dict(sample=True, top_k=5)):
        with pytest.raises(ValueError):
            vae.generate(B_M, cond, max_length=16, exact=True, **bad)
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(min_length=17),
                dict(min_length=-1), dict(max_length=0)):
        with pytest.raises(ValueError):
            vae.decoder_sampling.generate_map(None, cond, **{"max_length": 16, **bad})
    with pytest.raises(ValueError):
        vae.decoder_sampling.token_marginals(cond, max_length=0)
    with pytest.raises(ValueError):
        vae.decoder_sampling.length_distribution(cond, max_length=8, temperature=-1.0)


def test_token_marginals_against_the_oracle(model):
    """fp64 recursion on the ORACLE's fp64 logits.  eps = max |engine dense logits - oracle logits| is measured here; a step's
    probabilities then move by at most e^{2 eps} - 1 (the logit and the lse by eps each), so after t + 1 steps
    |got/ref - 1| <= (t+1) * (4 eps + (V + 8) * 2^-24), the factor 4 leaving room for the second order."""
    cfg, params, vae, cond, _ = model
    samp = vae.decoder_sampling
    V, T, temp = cfg.V, 12, 1.0
    alive = samp.token_marginals(cond, max_length=T, temperature=temp)
    assert alive.shape == (B_M, T, V) and alive.dtype == torch.float32
    engine = samp.decoder.workspace(B_M, T).logits.cpu().numpy().astype(np.float64).reshape(B_M, V, V)
    got = alive.cpu().numpy().astype(np.float64)
    # the oracle's table: teacher-forced on 0, 1, .., V-1, the logits at step c + 1 are those after token c (Q1: no state)
    pd = {k[len("decoder."):]: torch.tensor(v, dtype=torch.float64) for k, v in params.items() if k.startswith("decoder.")}
    x = torch.arange(V + 1, dtype=torch.int64).clamp(max=V - 1)[None, :].repeat(B_M, 1)
    logits, _ = O.decoder_forward(pd, torch.zeros(B_M, cfg.Z, dtype=torch.float64), torch.tensor(cond, dtype=torch.float64), cfg.L,
                                  x, [True] * (V + 1))
    oracle = logits[:, 1:, :].numpy()                                                  # [B, c, v]
    eps = np.abs(engine - oracle).max()
    print("eps", eps, "max|logit|", np.abs(oracle).max())
    assert eps <= 1e-4 * np.abs(oracle).max()
    lp = torch.log_softmax(torch.tensor(oracle) / temp, dim=-1).numpy().reshape(B_M * V, V)
    ref = X.marginals(lp, B_M, V, T, END, np.float64)
    bound = np.broadcast_to((np.arange(T) + 1)[None, :, None] * (4 * eps + (V + 8) * U), ref.shape)
    ok = ref >= 1e-6
    rel = np.abs(got / np.where(ok, ref, 1.0) - 1.0)
    print("worst |got/ref - 1| / bound:", (rel / bound)[ok].max())
    assert ok.sum() > B_M * T and np.all(rel[ok] <= bound[ok]), (rel / bound)[ok].max()
    ld = samp.length_distribution(cond, max_length=T, temperature=temp).cpu().numpy()
    assert ld.shape == (B_M, T + 1)
    np.testing.assert_array_equal(ld[:, :T], alive.cpu().numpy()[:, :, END])
    assert np.all(np.abs(ld.astype(np.float64).sum(1) - 1.0) <= 1e-5 * (T + 1))


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    B, V, T = 2, 12, 8
    table = torch.zeros(B * 257, 257, device="cuda")            # (large enough for the V = 257 call, should it launch)
    lse = torch.zeros(B * 257, device="cuda")
    tok = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    sc = torch.zeros(B, device="cuda")
    ln = torch.zeros(B, dtype=torch.int32, device="cuda")
    alive = torch.zeros(B, T, 257, device="cuda")
    n = C.c_long(0)
    assert lib.arcvae_dec_viterbi_ws_bytes(B, V, T, C.byref(n)) == 0 and n.value == B * V * T
    assert lib.arcvae_dec_viterbi_ws_bytes(B, 257, T, C.byref(n)) == -1
    assert lib.arcvae_dec_viterbi_ws_bytes(B, 0, T, C.byref(n)) == -1
    assert lib.arcvae_dec_viterbi_ws_bytes(B, V, 0, C.byref(n)) == -1
    assert lib.arcvae_dec_viterbi_ws_bytes(0, V, T, C.byref(n)) == -1
    assert lib.arcvae_dec_viterbi_ws_bytes(B, V, T, None) == -1
    need = B * V * T
    ws = torch.zeros(B * 257 * T, dtype=torch.uint8, device="cuda")

    def vit(ws_bytes=need, V_=V, T_=T, min_len=0, end=END, pad=PAD, temp=1.0, out=tok, score=sc, length=ln, scratch=ws):
        return lib.arcvae_dec_viterbi(L.ptr(table), L.ptr(lse), L.ptr(out), L.ptr(score), L.ptr(length), L.ptr(scratch), ws_bytes,
                                      B, V_, T_, min_len, end, pad, temp, L.stream_ptr())

    def mar(V_=V, T_=T, end=END, temp=1.0, out=alive):
        return lib.arcvae_dec_chain_marginals(L.ptr(table), L.ptr(lse), L.ptr(out), B, V_, T_, end, temp, L.stream_ptr())

    assert vit(ws_bytes=need - 1) == -1
    assert vit(V_=257, ws_bytes=B * 257 * T) == -1 and mar(V_=257) == -1
    assert vit(V_=0) == -1 and mar(V_=0) == -1
    assert vit(end=V) == -1 and vit(end=-1) == -1 and mar(end=V) == -1 and mar(end=-1) == -1
    assert vit(pad=256) == -1 and vit(pad=-1) == -1
    assert vit(min_len=T + 1) == -1 and vit(min_len=-1) == -1
    assert vit(T_=0) == -1 and mar(T_=0) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert vit(temp=bad) == -1 and mar(temp=bad) == -1
    assert vit(out=None) == -1 and vit(score=None) == -1 and vit(length=None) == -1 and vit(scratch=None) == -1
    assert mar(out=None) == -1
    assert vit() == 0 and mar() == 0                            # and the valid calls still run
    torch.cuda.synchronize()
    assert np.all(ln.cpu().numpy() >= 1)
