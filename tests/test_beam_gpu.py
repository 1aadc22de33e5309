"""Beam search and sequence log-likelihood on the GPU (csrc/beam.hip; an extension with no reference behaviour to match):
the kernels against the fp32 NumPy restatement (tests/beam_ref.py) operation for operation, and the model-level surface
(generate_beam, sequence_log_prob, ARCVAE.generate(beam_width=...)) against the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import beam_ref as R
from helpers import DEFAULT, TINY, dev as _dev, lib as _lib, oracle_loglik as _oracle_loglik, sampling_vae as _vae, ws_bytes

pytestmark = pytest.mark.gpu
END, PAD = 2, 0


def _search(table, lse, B, V, K, T, min_len, temp):
    L = _lib()
    ws = torch.empty(ws_bytes("beam", B, K, T), dtype=torch.uint8, device="cuda")
    tok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    ln = torch.empty(B, K, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_beam_search", L.ptr(table), L.ptr(lse), L.ptr(tok), L.ptr(sc), L.ptr(ln), L.ptr(ws), ws.numel(), B, V, K, T,
           min_len, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), sc.cpu().numpy(), ln.cpu().numpy()


# (V, K, max_len, min_len, temperature, table): "q8" = multiples of 1/8 (exact ties everywhere), "normal" = continuous,
# "near" = every even token's value + 2e-7 on the next token at a cold temperature: children whose lp differ round to one
# score, the case where the walk leaves its pre-pass lists for a full scan of the row
CASES = [(12, 1, 40, 0, 1.0, "q8"), (12, 4, 64, 3, 1.0, "q8"), (12, 32, 30, 2, 1.0, "q8"), (12, 8, 40, 0, 0.7, "normal"),
         (80, 4, 128, 5, 1.0, "normal"), (80, 8, 80, 0, 1.0, "q8"), (80, 32, 48, 0, 1.3, "normal"), (80, 16, 64, 4, 0.02, "near"),
         (256, 8, 64, 4, 1.0, "normal"), (256, 32, 128, 2, 1.0, "q8"), (256, 4, 40, 0, 0.02, "near")]


@pytest.mark.parametrize("V,K,T,min_len,temp,kind", CASES)
def test_kernel_is_the_fp32_restatement(V, K, T, min_len, temp, kind):
    """Tokens and lengths equal; scores BIT-equal: every score is a chain of single IEEE fp32 operations (one multiply and one
    subtract per step term, one add per step) in the same order on both sides, with the same lse passed in -- nothing is
    reassociated, so there is no rounding difference to tolerate."""
    rs = np.random.RandomState(V * 1000 + K * 10 + T)
    B = 6
    table = rs.standard_normal((B * V, V)).astype(np.float32) * 2.0
    table[:, END] += 0.5                                        # some hypotheses finish, some do not
    if kind == "q8":
        table = np.round(table * 8) / 8
    if kind == "near":
        table[:, 1::2] = table[:, 0::2][:, :V // 2] + np.float32(2e-7)
    lse = R.row_lse(table, temp).astype(np.float32)
    table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)    # (held: the launches are asynchronous)
    tok, sc, ln = _search(table_d, lse_d, B, V, K, T, min_len, temp)
    lp = R.step_terms(table, lse, temp)
    rtok, rsc, rln = R.beam_search(lp, B, V, K, T, min_len, END, PAD)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(ln, rln)
    np.testing.assert_array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    # the sequence log-likelihood kernel on the same table, for the returned hypotheses
    L = _lib()
    # (the kernel takes [B, T] tokens over the table's B rows: one launch per hypothesis slot)
    for k in range(K):
        rows = tok[:, k, :]
        rows_d = _dev(rows, torch.int32)
        out = torch.empty(B, dtype=torch.float32, device="cuda")
        L.call("arcvae_dec_sequence_logprob", L.ptr(table_d), L.ptr(lse_d), L.ptr(rows_d), L.ptr(out), B, T, V, END, float(temp),
               L.stream_ptr())
        got = out.cpu().numpy()
        ok = sc[:, k] > -np.inf
        np.testing.assert_array_equal(got[ok].view(np.uint32), sc[ok, k].view(np.uint32))
        np.testing.assert_array_equal(got, R.sequence_logprob(lp, rows, V, END))


@pytest.mark.parametrize("temp", [1.0, 0.3])
def test_row_lse_against_fp64(temp):
    rs = np.random.RandomState(7)
    for V in (12, 80, 256):
        table = (rs.standard_normal((300, V)) * 3.0).astype(np.float32)
        table_d = _dev(table, torch.float32)
        out = torch.empty(300, dtype=torch.float32, device="cuda")
        L = _lib()
        L.call("arcvae_dec_row_lse", L.ptr(table_d), L.ptr(out), 300, V, float(temp), L.stream_ptr())
        ref = R.row_lse(table.astype(np.float64), float(np.float32(temp)))
        got = out.cpu().numpy().astype(np.float64)
        # relative, with a floor of 1 where lse passes near zero (its absolute error is that of the log of the row sum)
        assert np.all(np.abs(got - ref) <= 1e-6 * np.maximum(1.0, np.abs(ref))), np.abs(got - ref).max()


@pytest.mark.parametrize("cfg,B,K,T,temp,min_len", [(TINY, 64, 8, 30, 1.0, 2), (TINY, 32, 32, 20, 0.5, 0),
                                                    (DEFAULT, 1024, 4, 40, 1.0, 0)])
def test_model_scores_are_oracle_log_likelihoods(cfg, B, K, T, temp, min_len):
    params = O.init_params(cfg, 1234)
    params["decoder.fc_out.bias"][END] += 2.0                 # (hypotheses that end, and ones that do not)
    vae = _vae(cfg, params)
    cond = np.random.RandomState(3).standard_normal((B, cfg.C)).astype(np.float32)
    tok, sc = vae.decoder_sampling.generate_beam(torch.zeros(B, cfg.Z), cond, max_length=T, beam_width=K, temperature=temp,
                                                 min_length=min_len)
    tok, sc = tok.cpu().numpy(), sc.cpu().numpy()
    assert tok.shape[:2] == (B, K) and tok.shape[2] <= T and np.all(np.isfinite(sc))
    assert np.all(np.diff(sc, axis=1) <= 0)
    for b in range(B):
        assert len({tuple(r) for r in tok[b]}) == K
    flat = tok.reshape(B * K, -1)
    ends = flat == END
    first = np.where(ends.any(1), ends.argmax(1), flat.shape[1])
    assert np.all(first >= min_len)
    ref = _oracle_loglik(params, cfg, np.repeat(cond, K, axis=0), flat, temp)
    assert np.all(np.abs(sc.reshape(-1) - ref) <= 1e-4 * np.abs(ref)), np.abs(sc.reshape(-1) - ref).max()
    # the scores ARE the model's sequence log-likelihood of the tokens (same table, same lse, same order of additions)
    lpm = vae.decoder.sequence_log_prob(torch.as_tensor(flat), np.repeat(cond, K, axis=0), temperature=temp).cpu().numpy()
    assert np.all(np.abs(lpm - sc.reshape(-1)) <= 1e-6 * np.abs(sc.reshape(-1)))


def test_width_equal_to_vocabulary_is_exact():
    """max_length 2, K = V: every one-token prefix is kept, so the K scores are the K best of all V^2 sequences (fp64
    enumeration with the oracle)."""
    cfg = O.Config(vocab_size=8, embedding_dim=16, hidden_dim=64, latent_dim=8, num_conditions=1, num_layers=2)
    params = O.init_params(cfg, 99)
    vae = _vae(cfg, params)
    B, V, temp = 3, cfg.V, 2.0
    cond = np.random.RandomState(4).standard_normal((B, cfg.C)).astype(np.float32)
    tok, sc = vae.decoder_sampling.generate_beam(torch.zeros(B, cfg.Z), cond, max_length=2, beam_width=V, temperature=temp,
                                                 early_stopping=False)
    sc = sc.cpu().numpy()
    seqs = np.array([(a, b if a != END else PAD) for a in range(V) for b in range(V)])
    seqs = np.unique(seqs, axis=0)
    for b in range(B):
        ref = _oracle_loglik(params, cfg, np.repeat(cond[b:b + 1], len(seqs), axis=0), seqs, temp)
        top = np.sort(ref)[::-1][:V]
        assert np.all(np.abs(sc[b] - top) <= 1e-4 * np.abs(top)), (sc[b], top)


def test_width_one_is_the_greedy_sampler():
    cfg, B, T = TINY, 256, 30
    params = O.init_params(cfg, 1234)
    vae = _vae(cfg, params)
    samp = vae.decoder_sampling
    cond = np.random.RandomState(5).standard_normal((B, cfg.C)).astype(np.float32)
    tok, _ = samp.generate_beam(torch.zeros(B, cfg.Z), cond, max_length=T, beam_width=1, early_stopping=False)
    table = samp.decoder.workspace(B, T).logits.cpu().numpy()     # the dense table the search walked
    greedy = samp.generate_with_temperature(torch.zeros(B, cfg.Z), cond, max_length=T, early_stopping=False).cpu().numpy()
    tok = tok.cpu().numpy()[:, 0, :]
    checked = 0
    for b in range(B):
        c, clear = 0, True
        for t in range(T):
            row = np.sort(table[b * cfg.V + c])
            clear &= bool(row[-1] - row[-2] >= 1e-6)
            c = greedy[b, t]
            if c == END:
                break
        if not clear:
            continue
        n = t + 1
        assert np.array_equal(tok[b, :n], greedy[b, :n]), b
        checked += 1
    assert checked > B // 2


def test_sequence_log_prob_is_minus_the_recon_loss():
    """Without EOS: sum_b log p(x_b) = -B*T*recon, recon the oracle's mean CE of the teacher-forced logits (all coins true)."""
    cfg, B, T = TINY, 16, 12
    params = O.init_params(cfg, 1234)
    vae = _vae(cfg, params)
    rs = np.random.RandomState(6)
    x = rs.randint(3, cfg.V, size=(B, T)).astype(np.int32)
    cond = rs.standard_normal((B, cfg.C)).astype(np.float32)
    got = vae.decoder.sequence_log_prob(x, cond).cpu().numpy().astype(np.float64)
    pd = {k[len("decoder."):]: torch.tensor(v, dtype=torch.float64) for k, v in params.items() if k.startswith("decoder.")}
    logits, _ = O.decoder_forward(pd, torch.zeros(B, cfg.Z, dtype=torch.float64), torch.tensor(cond, dtype=torch.float64), cfg.L,
                                  torch.tensor(x, dtype=torch.int64), [True] * T)
    recon = float(O.reconstruction_loss(logits, torch.tensor(x, dtype=torch.int64)))
    assert abs(got.sum() - (-B * T * recon)) <= 1e-4 * B * T * recon
    with pytest.raises(ValueError):
        vae.decoder.sequence_log_prob(np.full((B, T), cfg.V, np.int32), cond)


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    B, V, K, T = 2, 12, 4, 8
    table = torch.zeros(B * V, V, device="cuda")
    lse = torch.zeros(B * V, device="cuda")
    tok = torch.zeros(B, 32, T, dtype=torch.int32, device="cuda")
    sc = torch.zeros(B, 32, device="cuda")
    ln = torch.zeros(B, 32, dtype=torch.int32, device="cuda")
    n = C.c_long(0)
    assert lib.arcvae_dec_beam_ws_bytes(B, K, T, C.byref(n)) == 0 and n.value > 0
    assert lib.arcvae_dec_beam_ws_bytes(B, 0, T, C.byref(n)) == -1
    assert lib.arcvae_dec_beam_ws_bytes(B, 33, T, C.byref(n)) == -1
    lib.arcvae_dec_beam_ws_bytes(B, 32, T, C.byref(n))
    ws = torch.zeros(n.value, dtype=torch.uint8, device="cuda")

    def search(ws_bytes=n.value, V_=V, K_=K, T_=T, min_len=0, temp=1.0, tab=table):
        return lib.arcvae_dec_beam_search(L.ptr(tab), L.ptr(lse), L.ptr(tok), L.ptr(sc), L.ptr(ln), L.ptr(ws), ws_bytes, B, V_, K_,
                                          T_, min_len, END, PAD, temp, L.stream_ptr())

    need = C.c_long(0)
    lib.arcvae_dec_beam_ws_bytes(B, K, T, C.byref(need))
    assert search(ws_bytes=need.value - 1) == -1
    assert search(K_=0) == -1 and search(K_=33) == -1
    big = torch.zeros(B * 257, 257, device="cuda")
    assert search(V_=257, tab=big) == -1
    assert search(min_len=T + 1) == -1
    assert search(temp=0.0) == -1 and search(temp=float("nan")) == -1
    assert lib.arcvae_dec_beam_search(L.ptr(table), L.ptr(lse), C.c_void_p(0), L.ptr(sc), L.ptr(ln), L.ptr(ws), n.value, B, V, K,
                                      T, 0, END, PAD, 1.0, L.stream_ptr()) == -1
    assert lib.arcvae_dec_row_lse(L.ptr(table), L.ptr(lse), B * 257, 257, 1.0, L.stream_ptr()) == -1
    assert lib.arcvae_dec_sequence_logprob(L.ptr(table), L.ptr(lse), L.ptr(tok), L.ptr(sc), B, T, V, END, 0.0, L.stream_ptr()) == -1
    assert search() == 0                                        # and the valid call still runs
    torch.cuda.synchronize()


def test_generate_with_beam_width():
    cfg, B = TINY, 8
    params = O.init_params(cfg, 1234)
    vae = _vae(cfg, params)
    cond = np.random.RandomState(8).standard_normal((B, cfg.C)).astype(np.float32)
    greedy = vae.generate(B, cond, max_length=16)
    beam = vae.generate(B, cond, max_length=16, beam_width=4)
    assert beam.dim() == greedy.dim() == 2 and beam.shape[0] == greedy.shape[0] == B and beam.dtype == greedy.dtype
    assert 1 <= beam.shape[1] <= 16
    tok, _ = vae.decoder_sampling.generate_beam(None, cond, max_length=16, beam_width=4)
    assert np.array_equal(beam.cpu().numpy(), tok[:, 0, :beam.shape[1]].cpu().numpy())
    with pytest.raises(ValueError):
        vae.generate(B, cond, max_length=16, beam_width=4, sample=True)
    for bad in (dict(beam_width=0), dict(beam_width=33), dict(temperature=0.0), dict(min_length=20)):
        with pytest.raises(ValueError):
            vae.decoder_sampling.generate_beam(None, cond, max_length=16, **{"beam_width": 4, **bad})
