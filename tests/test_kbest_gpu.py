"""Exact K-best decoding on the GPU (csrc/kbest.hip; an extension with no reference behaviour to match): the kernel against the
fp32 NumPy restatement (tests/kbest_ref.py) operation for operation, against the Viterbi, beam and sequence log-likelihood
kernels on the same device tables, its row loop and return codes, and the model-level surface (generate_kbest,
ARCVAE.generate(exact=True, num_best=K)) against the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ref as R
import kbest_ref as KB
from helpers import bits as _bits, dev as _dev, ending_model, lib as _lib, ws_bytes

pytestmark = pytest.mark.gpu
END, PAD = 2, 0


def _ws_bytes(B, V, K, T):
    return ws_bytes("kbest", B, V, K, T)


def _kbest(table_d, lse_d, B, V, K, T, min_len, temp, pad=PAD):
    L = _lib()
    n = _ws_bytes(B, V, K, T)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok = torch.full((B, K, T), -7, dtype=torch.int32, device="cuda")
    sc = torch.full((B, K), 7.0, dtype=torch.float32, device="cuda")
    ln = torch.full((B, K), -7, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_kbest", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok), L.ptr(sc), L.ptr(ln), L.ptr(ws), n, B, V, K, T, min_len,
           END, pad, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), sc.cpu().numpy(), ln.cpu().numpy()


_tables = {}


def _table(V, K, T, temp, kind, lower, B):
    """(table, lse, step terms) of a case, host and device: made once, shared, never modified."""
    key = (V, K, T, temp, kind, lower, B)
    if key not in _tables:
        table, lse = KB.make_table(np.random.RandomState(V * 1000 + T), B, V, kind, temp, END, float(lower))
        lp = R.step_terms(table, lse, temp)
        table_d, lse_d = _dev(table, torch.float32), _dev(lse, torch.float32)
        for a in (table, lse, lp):
            a.setflags(write=False)
        _tables[key] = (table, lse, lp, table_d, lse_d)
    return _tables[key]


# (V, K, max_len, min_len, temperature, table, lowering of the end column): the tables of tests/kbest_ref.make_table.  No
# recursion (max_len 1); exact ties everywhere (q8d); fewer admissible sequences than K with V below 4 (empty slots); lists that
# fill up over the first steps; the end never allowed (min_len = max_len); the workload's V; whole-length back-traces (the end
# column lowered by 4 * max_len: at about 2 nats per step the optimum then does not end); the largest LDS footprint (V 256, K 32).
# The kernel is built per number of list heads a lane holds -- ceil(V / 16) = 1 .. 8 up to V 128 (16 lanes per column), ceil(V / 64)
# = 3, 4 above (a wave per column) -- and per staging of the step terms in LDS (while lists and terms fit in 64 KB: always up to
# V 96, never above V 124): V 12, 20, 40, 64, 80, 96, 97, 116 run the staged forms with 1 .. 8 heads, V 100 and 120 at K 32 the
# unstaged ones with 7 and 8, V 130 and 256 the wave-wide ones with 3 and 4; V 97 and 130 are no multiple of 4.
CASES = [(12, 1, 1, 0, 1.0, "q8", 4), (12, 4, 40, 0, 1.0, "q8d", 4), (3, 32, 3, 0, 1.0, "q8d", 4), (12, 32, 6, 0, 1.0, "q8d", 4),
         (12, 8, 30, 30, 0.7, "normal", 4), (80, 16, 64, 5, 1.0, "normal", 4), (80, 4, 128, 0, 1.0, "q8-lowered-end", 4 * 128),
         (96, 8, 6, 0, 1.0, "q8", 4), (97, 8, 6, 1, 1.0, "normal", 4), (130, 4, 8, 8, 1.0, "q8", 4),
         (256, 32, 12, 2, 1.0, "q8d", 4), (256, 2, 48, 0, 1.3, "normal", 4), (120, 32, 5, 0, 1.0, "q8", 4),
         (20, 4, 5, 0, 1.0, "q8d", 4), (40, 8, 5, 1, 1.0, "normal", 4), (64, 32, 4, 0, 1.0, "q8", 4),
         (100, 32, 4, 0, 1.0, "normal", 4), (116, 4, 5, 0, 1.0, "q8", 4)]


@pytest.mark.parametrize("V,K,T,min_len,temp,kind,lower", CASES)
def test_kbest_kernel_is_the_fp32_restatement(V, K, T, min_len, temp, kind, lower):
    """Tokens, lengths and score BITS equal: every score is a chain of single IEEE fp32 operations (one multiply and one subtract
    per step term, one add per step) in the same order on both sides, with the same lse passed in, and every choice between equal
    scores is fixed by the contract -- there is no rounding difference and no freedom to tolerate.  The sequence log-likelihood
    kernel returns the same bits for the returned tokens."""
    B = 4 if V == 256 else 6
    table, lse, lp, table_d, lse_d = _table(V, K, T, temp, kind, lower, B)
    tok, sc, ln = _kbest(table_d, lse_d, B, V, K, T, min_len, temp)
    rtok, rsc, rln = KB.kbest(lp, B, V, K, T, min_len, END, PAD)
    np.testing.assert_array_equal(ln, rln)
    np.testing.assert_array_equal(tok, rtok)
    np.testing.assert_array_equal(_bits(sc), _bits(rsc))
    filled = rsc > -np.inf
    if V == 3:
        assert np.all(filled.sum(1) == 15) and np.all(ln[~filled] == 0)      # 1 + 2 + 4 + 8 admissible sequences, 17 empty slots
    else:
        assert np.all(filled)
    if lower > 4:
        assert np.sum(ln[:, 0] == T) >= B // 2, ln[:, 0]        # (the unfinished branch and whole-length back-traces)
    if min_len == T:
        assert np.all(ln == T) and not np.any(tok == END)
    if kind == "q8d" and T > 1:
        assert np.any((sc[:, :-1] == sc[:, 1:]) & filled[:, 1:])               # (ties between adjacent returned scores)
    L = _lib()
    out = torch.empty(B, dtype=torch.float32, device="cuda")
    for j in range(K):
        tok_d = _dev(tok[:, j, :], torch.int32)
        L.call("arcvae_dec_sequence_logprob", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok_d), L.ptr(out), B, T, V, END, float(temp),
               L.stream_ptr())
        got = out.cpu().numpy()
        np.testing.assert_array_equal(_bits(got[filled[:, j]]), _bits(sc[filled[:, j], j]))


@pytest.mark.parametrize("V,K,T,min_len,temp,kind,lower", [CASES[1], CASES[5], CASES[6], CASES[9], CASES[11]])
def test_k1_is_the_viterbi_kernel(V, K, T, min_len, temp, kind, lower):
    """On the same device table, K = 1 returns arcvae_dec_viterbi's tokens, length and score bits."""
    B = 4 if V == 256 else 6
    _, _, _, table_d, lse_d = _table(V, K, T, temp, kind, lower, B)
    tok, sc, ln = _kbest(table_d, lse_d, B, V, 1, T, min_len, temp)
    L = _lib()
    n = C.c_long(0)
    L.call("arcvae_dec_viterbi_ws_bytes", B, V, T, C.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    vtok = torch.empty(B, T, dtype=torch.int32, device="cuda")
    vsc = torch.empty(B, dtype=torch.float32, device="cuda")
    vln = torch.empty(B, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_viterbi", L.ptr(table_d), L.ptr(lse_d), L.ptr(vtok), L.ptr(vsc), L.ptr(vln), L.ptr(ws), n.value, B, V, T,
           min_len, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tok[:, 0], vtok.cpu().numpy())
    np.testing.assert_array_equal(ln[:, 0], vln.cpu().numpy())
    np.testing.assert_array_equal(_bits(sc[:, 0]), _bits(vsc.cpu().numpy()))


def test_no_rank_is_below_the_beam_and_the_pad_token_fills_the_tail():
    """V 80, K 32, max_len 64, min_len 5, on one device table: every rank >= the beam kernel's at the same K; a pad token outside
    the vocabulary fills exactly the positions after each sequence's end."""
    B, V, K, T, min_len, temp = 6, 80, 32, 64, 5, 1.0
    _, _, _, table_d, lse_d = _table(V, K, T, temp, "normal", 4, B)
    tok, sc, ln = _kbest(table_d, lse_d, B, V, K, T, min_len, temp, pad=255)
    assert np.all(ln >= 1)
    pos = np.arange(T)[None, None, :]
    assert np.all((tok == 255) == (pos >= ln[:, :, None]))
    assert np.all((tok[pos < ln[:, :, None]] >= 0) & (tok[pos < ln[:, :, None]] < V))
    L = _lib()
    n = C.c_long(0)
    L.call("arcvae_dec_beam_ws_bytes", B, K, T, C.byref(n))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    btok = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
    bsc = torch.empty(B, K, dtype=torch.float32, device="cuda")
    bln = torch.empty(B, K, dtype=torch.int32, device="cuda")
    L.call("arcvae_dec_beam_search", L.ptr(table_d), L.ptr(lse_d), L.ptr(btok), L.ptr(bsc), L.ptr(bln), L.ptr(ws), n.value, B, V, K,
           T, min_len, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    assert np.all(sc >= bsc.cpu().numpy())


def test_row_loop_reuses_the_slices():
    """The scratch is sized for the rows in flight, not for B: ws_bytes grows with B up to G rows and is constant above.  B = G + 3
    rows of seven distinct tables repeated with period 7 (so a workgroup's second row differs from its first): every row equals
    the restatement of its table."""
    V, K, T = 12, 2, 4
    per_row = 2 * T * V * K
    G = _ws_bytes(1 << 20, V, K, T) // per_row
    assert G >= 1 and _ws_bytes(1 << 20, V, K, T) == G * per_row
    for B in (1, 5, G - 1, G):
        assert _ws_bytes(B, V, K, T) == B * per_row
    for B in (G + 1, G + 3, 4 * G):
        assert _ws_bytes(B, V, K, T) == G * per_row
    B = G + 3
    table7, lse7 = KB.make_table(np.random.RandomState(77), 7, V, "q8d", 1.0, END)
    rtok, rsc, rln = KB.kbest(R.step_terms(table7, lse7, 1.0), 7, V, K, T, 0, END, PAD)
    idx = np.arange(B) % 7
    table = table7.reshape(7, V, V)[idx].reshape(B * V, V)
    lse = lse7.reshape(7, V)[idx].reshape(B * V)
    tok, sc, ln = _kbest(_dev(table, torch.float32), _dev(lse, torch.float32), B, V, K, T, 0, 1.0)
    np.testing.assert_array_equal(tok, rtok[idx])
    np.testing.assert_array_equal(ln, rln[idx])
    np.testing.assert_array_equal(_bits(sc), _bits(rsc[idx]))


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    B, V, K, T = 2, 12, 4, 8
    table = torch.zeros(B * 257, 257, device="cuda")            # (large enough for the V = 257 call, should it launch)
    lse = torch.zeros(B * 257, device="cuda")
    tok = torch.zeros(B, 33, T + 1, dtype=torch.int32, device="cuda")
    sc = torch.zeros(B, 33, device="cuda")
    ln = torch.zeros(B, 33, dtype=torch.int32, device="cuda")
    n = C.c_long(0)
    assert lib.arcvae_dec_kbest_ws_bytes(B, V, K, T, C.byref(n)) == 0 and n.value == B * 2 * T * V * K
    for bad in ((0, V, K, T), (B, 0, K, T), (B, 257, K, T), (B, V, 0, T), (B, V, 33, T), (B, V, K, 0)):
        assert lib.arcvae_dec_kbest_ws_bytes(*bad, C.byref(n)) == -1
    assert lib.arcvae_dec_kbest_ws_bytes(B, V, K, T, None) == -1
    need = B * 2 * T * V * K
    ws = torch.zeros(B * 2 * (T + 1) * 257 * 33, dtype=torch.uint8, device="cuda")

    def kb(ws_bytes=ws.numel(), V_=V, K_=K, T_=T, min_len=0, end=END, pad=PAD, temp=1.0, x=table, l=lse, out=tok, score=sc,
           length=ln, scratch=ws):
        return lib.arcvae_dec_kbest(L.ptr(x), L.ptr(l), L.ptr(out), L.ptr(score), L.ptr(length), L.ptr(scratch), ws_bytes, B, V_,
                                    K_, T_, min_len, end, pad, temp, L.stream_ptr())

    assert kb(K_=0) == -1 and kb(K_=33) == -1
    assert kb(V_=0) == -1 and kb(V_=257) == -1
    assert kb(end=V) == -1 and kb(end=-1) == -1
    assert kb(pad=256) == -1 and kb(pad=-1) == -1
    assert kb(min_len=T + 1) == -1 and kb(min_len=-1) == -1
    assert kb(T_=0) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert kb(temp=bad) == -1
    assert kb(x=None) == -1 and kb(l=None) == -1 and kb(out=None) == -1 and kb(score=None) == -1 and kb(length=None) == -1
    assert kb(scratch=None) == -1
    assert kb(ws_bytes=need - 1) == -1
    assert kb(ws_bytes=need) == 0                               # and the valid call still runs
    torch.cuda.synchronize()
    assert np.all(ln.cpu().numpy().reshape(-1)[:B * K] >= 1)


# ---- model level: TINY, B 64 ---------------------------------------------------------------------------------------------------
B_M, T_M, K_M = 64, 20, 8


@pytest.fixture(scope="module")
def model():
    return ending_model(B_M, END)


@pytest.mark.parametrize("temp,min_len", [(1.0, 0), (0.5, 6)])
def test_generate_kbest(model, temp, min_len):
    cfg, params, vae, cond, loglik = model
    samp = vae.decoder_sampling
    z = torch.zeros(B_M, cfg.Z)
    tok, sc = samp.generate_kbest(z, cond, max_length=T_M, num_best=K_M, temperature=temp, min_length=min_len)
    assert tok.dtype == torch.int32 and sc.dtype == torch.float32
    tok, sc = tok.cpu().numpy(), sc.cpu().numpy()
    Lr = tok.shape[2]
    assert tok.shape[:2] == (B_M, K_M) and 1 <= Lr <= T_M and sc.shape == (B_M, K_M) and np.all(np.isfinite(sc))
    assert np.all(sc[:, :-1] >= sc[:, 1:])
    ends = tok == END
    first = np.where(ends.any(2), ends.argmax(2), Lr)
    assert np.all(first >= min_len)                            # min_length is honoured
    assert np.where(ends.any(2), first + 1, T_M).max() == Lr   # early stopping: L = the longest returned sequence
    for b in range(B_M):                                       # the K sequences of a row are pairwise distinct
        assert len({tuple(r) for r in tok[b]}) == K_M
    flat = tok.reshape(B_M * K_M, Lr)
    ref = loglik(params, cfg, np.repeat(cond, K_M, axis=0), flat, temp).reshape(B_M, K_M)
    assert np.all(np.abs(sc - ref) <= 1e-4 * np.abs(ref)), np.abs(sc - ref).max()
    # the scores ARE the sequence log-likelihood of the tokens (same table, same lse, same order of additions)
    for j in range(K_M):
        lpm = samp.decoder.sequence_log_prob(torch.as_tensor(tok[:, j, :].copy()), cond, temperature=temp).cpu().numpy()
        np.testing.assert_array_equal(_bits(lpm), _bits(sc[:, j]))
    # rank 0 is generate_map's, bit for bit
    mtok, msc = samp.generate_map(z, cond, max_length=T_M, temperature=temp, min_length=min_len, early_stopping=False)
    full, sc2 = samp.generate_kbest(None, cond, max_length=T_M, num_best=K_M, temperature=temp, min_length=min_len,
                                    early_stopping=False)
    full = full.cpu().numpy()
    np.testing.assert_array_equal(full[:, 0, :], mtok.cpu().numpy())
    np.testing.assert_array_equal(_bits(sc[:, 0]), _bits(msc.cpu().numpy()))
    # early_stopping=False agrees on the common prefix and pads the rest
    assert full.shape == (B_M, K_M, T_M) and np.array_equal(full[:, :, :Lr], tok) and np.all(full[:, :, Lr:] == PAD)
    np.testing.assert_array_equal(_bits(sc2.cpu().numpy()), _bits(sc))
    # never below the beam of the same width, at every rank
    _, bsc = samp.generate_beam(z, cond, max_length=T_M, beam_width=K_M, temperature=temp, min_length=min_len)
    assert np.all(sc >= bsc.cpu().numpy())


def test_generate_exact_num_best(model):
    cfg, params, vae, cond, _ = model
    tok, _ = vae.decoder_sampling.generate_kbest(None, cond, max_length=16, num_best=K_M)
    got = vae.generate(B_M, cond, max_length=16, exact=True, num_best=K_M)
    assert got.dtype == torch.int32 and got.dim() == 3 and np.array_equal(got.cpu().numpy(), tok.cpu().numpy())
    one = vae.generate(B_M, cond, max_length=16, exact=True)                # num_best=None: the [B, L] result as before
    assert one.dim() == 2 and np.array_equal(one.cpu().numpy(), tok.cpu().numpy()[:, 0, :one.shape[1]])
    with pytest.raises(ValueError):
        vae.generate(B_M, cond, max_length=16, num_best=4)                  # num_best needs exact=True
    for bad in (dict(sample=True), dict(beam_width=4), dict(top_k=5), dict(top_p=0.9)):
        with pytest.raises(ValueError):
            vae.generate(B_M, cond, max_length=16, exact=True, num_best=4, **bad)
    for bad in (dict(num_best=0), dict(num_best=33), dict(temperature=0.0), dict(temperature=float("nan")),
                dict(temperature=float("inf")), dict(min_length=17), dict(min_length=-1), dict(max_length=0)):
        with pytest.raises(ValueError):
            vae.decoder_sampling.generate_kbest(None, cond, **{"max_length": 16, **bad})
