"""Sampling without replacement on the GPU (csrc/swor.hip; an extension with no reference behaviour to match): the kernel against
the fp64 NumPy restatement of the header's contract (tests/swor_ref.py), its statistics against Plackett-Luce, the unbiased
estimator against the chain's exact length distribution, and the model-level surface (generate_without_replacement,
importance_weights, ARCVAE.generate(sample=True, num_samples=...)) against the fp64 oracle."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_ref
import swor_ref as R
from helpers import bits, dev as _dev, ending_model, lib as _lib, ws_bytes
from test_swor_ref import _chain, pair_z_scores

pytestmark = pytest.mark.gpu
END, PAD = 2, 0


def _swor(table_d, lse_d, B, V, K, T, seed, temp=1.0):
    L = _lib()
    ws = torch.empty(ws_bytes("swor", B, K, T), dtype=torch.uint8, device="cuda")
    seed_d = torch.tensor([seed], dtype=torch.int64, device="cuda")
    tok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
    lp, G = torch.empty(B, K, dtype=torch.float32, device="cuda"), torch.empty(B, K, dtype=torch.float32, device="cuda")
    ln = torch.empty(B, K, dtype=torch.int32, device="cuda")
    thr = torch.empty(B, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_swor", L.ptr(table_d), L.ptr(lse_d), L.ptr(seed_d), L.ptr(tok), L.ptr(lp), L.ptr(G), L.ptr(ln), L.ptr(thr),
           L.ptr(ws), ws.numel(), B, V, K, T, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return dict(tokens=tok.cpu().numpy(), log_probs=lp.cpu().numpy(), perturbed=G.cpu().numpy(), lengths=ln.cpu().numpy(),
                threshold=thr.cpu().numpy())


def _sets(tokens):
    return [{tuple(s) for s in row} for row in tokens]


CASES = [(12, 1, 16), (12, 4, 16), (80, 8, 24), (256, 32, 12), (12, 32, 8)]


@pytest.mark.parametrize("V,K,T", CASES)
def test_kernel_against_the_fp64_restatement(V, K, T):
    """Figures measured on an MI355X are in DESIGN.md section 10 (largest deviation from fp64 per case, next to E_ref)."""
    B, seed = 48, 1234
    rs = np.random.RandomState(V * 1000 + K * 10 + T)
    table = rs.standard_normal((B * V, V)).astype(np.float32) * 2.0
    table[:, END] += 0.5
    lse = beam_ref.row_lse(table, 1.0).astype(np.float32)
    table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)
    got = _swor(table_d, lse_d, B, V, K, T, seed)
    ref = R.swor(table, lse, B, V, K, T, seed, END, PAD, dtype=np.float64)
    r32 = R.swor(table, lse, B, V, K, T, seed, END, PAD, dtype=np.float32)
    # on all rows: log_probs are the sequence log-likelihood of the tokens bit for bit, perturbed descends, sequences distinct
    assert np.all(np.isfinite(got["log_probs"])) and np.all(np.isfinite(got["perturbed"]))
    L = _lib()
    for k in range(K):
        rows_d = _dev(got["tokens"][:, k, :], torch.int32)
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        L.call("arcvae_dec_sequence_logprob", L.ptr(table_d), L.ptr(lse_d), L.ptr(rows_d), L.ptr(out), B, T, V, END, 1.0,
               L.stream_ptr())
        np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(got["log_probs"][:, k]))
    assert np.all(np.diff(got["perturbed"], axis=1) <= 0)
    assert all(len(s) == K for s in _sets(got["tokens"]))
    ends = got["tokens"] == END
    np.testing.assert_array_equal(got["lengths"], np.where(ends.any(2), ends.argmax(2) + 1, T))
    after = np.arange(T)[None, None, :] >= got["lengths"][:, :, None]
    assert np.all(got["tokens"][after] == PAD)
    # rows with a clear boundary: the reference's set of sequences, and its values within the fp32 restatement's own error
    clear = ref["gap"] >= 1e-3
    assert (~clear).sum() <= B // 10, (~clear).sum()
    gs, fs = _sets(got["tokens"]), _sets(ref["tokens"])
    assert [b for b in np.flatnonzero(clear) if gs[b] != fs[b]] == []
    assert np.all(np.isfinite(ref["perturbed"])) and np.all(np.isfinite(ref["threshold"]))      # (every case rejects something)
    dev = lambda x, name: np.abs(x[name].astype(np.float64) - ref[name])[clear].max()     # noqa: E731
    e_ref = max(dev(r32, "perturbed"), dev(r32, "threshold"))  # from the two restatements, never from the kernel
    dG, dT = dev(got, "perturbed"), dev(got, "threshold")
    print(f"V {V} K {K} T {T}: left out {(~clear).sum()}, E_ref {e_ref:.3e}, |perturbed - fp64| {dG:.3e}, |threshold - fp64| {dT:.3e}")
    assert dG <= 8 * e_ref + 1e-5 and dT <= 8 * e_ref + 1e-5, (dG, dT, e_ref)


@functools.lru_cache(maxsize=None)
def _tiny_chain(B):
    table, lse, lp = _chain(B, seed=3, same=True)
    return _dev(table, torch.float32), _dev(lse, torch.float32), R.sequence_probs(lp[0], 3, 2, END, PAD)


def test_ordered_pairs_follow_plackett_luce_on_the_device():
    B = 20000
    table_d, lse_d, probs = _tiny_chain(B)
    got = _swor(table_d, lse_d, B, 3, 2, 2, 2024)
    worst, cells = pair_z_scores(got["tokens"], probs)
    print("max |z| =", worst, "over", cells, "cells")
    assert cells >= 20 and worst <= 5.0, (worst, cells)


def test_one_sample_follows_the_sequence_distribution():
    B = 20000
    table_d, lse_d, probs = _tiny_chain(B)
    got = _swor(table_d, lse_d, B, 3, 1, 2, 77)
    seqs, counts = np.unique(got["tokens"][:, 0, :], axis=0, return_counts=True)
    seen = {tuple(s): c for s, c in zip(seqs, counts)}
    assert set(seen) <= set(probs)
    assert np.all(got["perturbed"] == 0) and np.all(np.isfinite(got["threshold"]))
    cells = 0
    for s, p in probs.items():
        if B * p >= 50:
            z = (seen.get(s, 0) - B * p) / np.sqrt(B * p * (1 - p))
            assert abs(z) <= 5.0, (s, z)
            cells += 1
    assert cells >= 6


def test_exhaustion():
    B, V, T = 8, 3, 2
    table, lse, lp = _chain(B)
    got = _swor(_dev(table, torch.float32), _dev(lse, torch.float32), B, V, 9, T, 9)
    for b in range(B):
        assert {tuple(s) for s in got["tokens"][b, :7]} == set(R.sequence_probs(lp[b], V, T, END, PAD))
    assert np.all(np.isneginf(got["log_probs"][:, 7:])) and np.all(np.isneginf(got["perturbed"][:, 7:]))
    assert np.all(got["lengths"][:, 7:] == 0) and np.all(got["tokens"][:, 7:] == PAD)
    assert np.all(np.isneginf(got["threshold"]))
    np.testing.assert_allclose(np.exp(got["log_probs"][:, :7].astype(np.float64)).sum(1), 1.0, atol=1e-6)


def test_estimator_of_the_expected_length_is_unbiased():
    """sum_k weights * f over the K-1 highest ranks (return_weights=True) against the exact E[f] of the chain, f = the number of
    tokens up to the first end_token (T + 1 without one): within 5 standard errors, the standard error from the rows' spread."""
    from models.decoder_sampling import importance_weights, unconditioned
    B, K, T = 4096, 8, 20
    cfg, params, vae, cond, _ = ending_model(1)
    cond = np.repeat(cond, B, axis=0)
    samp = vae.decoder_sampling
    tok, lp, G, thr, w = samp.generate_without_replacement(None, cond, max_length=T, num_samples=K, seed=5, early_stopping=False,
                                                           return_weights=True)
    dist = samp.length_distribution(cond[:1], max_length=T).double().cpu().numpy()[0]
    exact = float((dist * np.arange(1, T + 2)).sum())
    tok, w = tok.cpu().numpy(), w.double().cpu().numpy()
    ends = tok == END
    f = np.where(ends.any(2), ends.argmax(2) + 1, T + 1)
    est = (w * f).sum(1)
    assert np.all(w[:, K - 1] == 0) and np.all(w[:, :K - 1] > 0)
    assert np.all(G[:, 0].cpu().numpy() == 0)                   # the walk's values are conditioned on the row's largest being 0
    free = unconditioned(G, 5)
    assert np.all(np.diff(free.cpu().numpy(), axis=1) <= 0)     # (monotone: the order is kept)
    full = importance_weights(lp, free[:, K - 1]).cpu().numpy()
    np.testing.assert_array_equal(full[:, :K - 1], w[:, :K - 1].astype(np.float32))
    se = est.std(ddof=1) / np.sqrt(B)
    print(f"estimate {est.mean():.5f} +- {se:.5f}, exact {exact:.5f}, mass-weight mean {w.sum(1).mean():.5f}")
    assert abs(est.mean() - exact) <= 5 * se, (est.mean(), exact, se)
    assert abs(w.sum(1).mean() - 1.0) <= 5 * w.sum(1).std(ddof=1) / np.sqrt(B)          # f = 1: the weights average to one


def test_same_seed_same_output():
    B, K, T = 64, 4, 20
    cfg, params, vae, cond, _ = ending_model(B)
    samp = vae.decoder_sampling
    run = lambda **kw: [bits(x.cpu().numpy()) if x.dtype == torch.float32 else x.cpu().numpy()       # noqa: E731
                        for x in samp.generate_without_replacement(None, cond, max_length=T, early_stopping=False, **kw)]
    eager = run(num_samples=K, seed=7, use_graph=False)
    first = run(num_samples=K, seed=7)                           # eager, then captured
    other = run(num_samples=K, seed=8)                           # a replay, another seed
    replay = run(num_samples=K, seed=7)                          # a replay, the first seed again
    for a, b_, c in zip(eager, first, replay):
        np.testing.assert_array_equal(a, b_)
        np.testing.assert_array_equal(a, c)
    assert (other[0] != eager[0]).any(axis=(1, 2)).sum() >= B // 2
    one = run(num_samples=1, seed=7)
    for a, b_ in zip(one[:3], eager[:3]):                        # rank 0 does not depend on K: tokens, log_probs, perturbed
        np.testing.assert_array_equal(a[:, 0], b_[:, 0])


def test_model_level():
    B, K, T = 32, 8, 20
    cfg, params, vae, cond, oracle_loglik = ending_model(B)
    samp = vae.decoder_sampling
    tok, lp, G, thr = samp.generate_without_replacement(torch.zeros(B, cfg.Z), cond, max_length=T, num_samples=K, seed=3)
    tok, lp, G, thr = tok.cpu().numpy(), lp.cpu().numpy(), G.cpu().numpy(), thr.cpu().numpy()
    assert tok.shape[:2] == (B, K) and 1 <= tok.shape[2] <= T and lp.shape == G.shape == (B, K) and thr.shape == (B,)
    assert np.all(np.isfinite(lp)) and np.all(np.diff(G, axis=1) <= 0) and np.all(thr <= G[:, -1])
    assert all(len({tuple(s) for s in row}) == K for row in tok)
    flat = tok.reshape(B * K, -1)
    ref = oracle_loglik(params, cfg, np.repeat(cond, K, axis=0), flat, 1.0)
    assert np.all(np.abs(lp.reshape(-1) - ref) <= 1e-4 * np.abs(ref)), np.abs(lp.reshape(-1) - ref).max()
    lpm = vae.decoder.sequence_log_prob(torch.as_tensor(flat), np.repeat(cond, K, axis=0)).cpu().numpy()
    np.testing.assert_array_equal(bits(lpm), bits(lp.reshape(-1)))
    gen = vae.generate(B, cond, max_length=T, sample=True, num_samples=4, seed=3)
    tok4 = samp.generate_without_replacement(None, cond, max_length=T, num_samples=4, seed=3)[0]
    assert gen.dim() == 3 and gen.shape[:2] == (B, 4) and gen.dtype == torch.int32
    assert np.array_equal(gen.cpu().numpy(), tok4.cpu().numpy())
    for bad in (dict(num_samples=0), dict(num_samples=33), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            samp.generate_without_replacement(None, cond, max_length=T, **{"num_samples": 4, **bad})
    for bad in (dict(beam_width=4), dict(exact=True), dict(top_k=5)):
        with pytest.raises(ValueError):
            vae.generate(B, cond, max_length=T, sample=True, num_samples=4, **bad)
    with pytest.raises(ValueError):
        vae.generate(B, cond, max_length=T, num_samples=4)                   # needs sample=True


def test_importance_weights():
    from models.decoder_sampling import importance_weights
    lp = torch.tensor([[-1.0, -2.0, -float("inf")], [-0.5, -3.0, -4.0]], device="cuda")
    thr = torch.tensor([-float("inf"), -2.5], device="cuda")
    w = importance_weights(lp, thr).cpu().numpy().astype(np.float64)
    q = -np.expm1(-np.exp(np.array([-0.5, -3.0, -4.0]) + 2.5))
    np.testing.assert_allclose(w[0], [np.exp(-1.0), np.exp(-2.0), 0.0], rtol=1e-6)
    np.testing.assert_allclose(w[1], np.exp([-0.5, -3.0, -4.0]) / q, rtol=1e-6)


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    B, V, K, T = 2, 12, 4, 8
    table = torch.zeros(B * V, V, device="cuda")
    lse = torch.zeros(B * V, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    tok = torch.zeros(B, 32, T, dtype=torch.int32, device="cuda")
    lp, G = torch.zeros(B, 32, device="cuda"), torch.zeros(B, 32, device="cuda")
    ln = torch.zeros(B, 32, dtype=torch.int32, device="cuda")
    thr = torch.zeros(B, device="cuda")
    n = C.c_long(0)
    assert lib.arcvae_dec_swor_ws_bytes(B, K, T, C.byref(n)) == 0 and n.value > 0
    assert lib.arcvae_dec_swor_ws_bytes(B, 0, T, C.byref(n)) == -1
    assert lib.arcvae_dec_swor_ws_bytes(B, 33, T, C.byref(n)) == -1
    assert lib.arcvae_dec_swor_ws_bytes(0, K, T, C.byref(n)) == -1
    assert lib.arcvae_dec_swor_ws_bytes(B, K, 0, C.byref(n)) == -1
    assert lib.arcvae_dec_swor_ws_bytes(B, K, T, None) == -1
    lib.arcvae_dec_swor_ws_bytes(B, 32, T, C.byref(n))
    ws = torch.zeros(n.value, dtype=torch.uint8, device="cuda")

    def walk(ws_bytes=n.value, V_=V, K_=K, T_=T, B_=B, pad=PAD, temp=1.0, tab=table, tokens=tok, seed_=seed):
        return lib.arcvae_dec_swor(L.ptr(tab), L.ptr(lse), L.ptr(seed_) if seed_ is not None else None,
                                   L.ptr(tokens) if tokens is not None else None, L.ptr(lp), L.ptr(G), L.ptr(ln), L.ptr(thr),
                                   L.ptr(ws), ws_bytes, B_, V_, K_, T_, END, pad, temp, L.stream_ptr())

    need = C.c_long(0)
    lib.arcvae_dec_swor_ws_bytes(B, K, T, C.byref(need))
    assert walk(ws_bytes=need.value - 1) == -1                  # one byte short
    assert walk(K_=0) == -1 and walk(K_=33) == -1
    big = torch.zeros(B * 257, 257, device="cuda")
    assert walk(V_=257, tab=big) == -1 and walk(V_=0) == -1
    assert walk(B_=0) == -1 and walk(T_=0) == -1
    assert walk(pad=-1) == -1 and walk(pad=256) == -1
    assert walk(temp=0.0) == -1 and walk(temp=-1.0) == -1 and walk(temp=float("nan")) == -1
    assert walk(tokens=None) == -1 and walk(seed_=None) == -1
    assert walk(ws_bytes=need.value) == 0                       # and the valid call still runs
    torch.cuda.synchronize()
    assert np.all(np.isfinite(lp[:, :K].cpu().numpy()))
