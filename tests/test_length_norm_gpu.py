"""Length-normalised exact decoding and the best-sequence-per-length profile on the GPU (csrc/chain.hip, csrc/kbest.hip; extensions
with no reference behaviour to match): the three kernels against the fp32 NumPy restatement (tests/length_norm_ref.py) operation
for operation, their identities with the un-normalised entry points and the sequence log-likelihood kernel on the same device
tables, the back-trace at every length, return codes, and the model-level surface (length_penalty=, best_by_length,
generate_of_length, ARCVAE.generate(exact=True, length_penalty=)).

Every comparison is of BITS: a raw score is a chain of single IEEE fp32 additions in the contract's order, a key is one correctly
rounded fp32 division of it, and every choice between equal keys is fixed by the contract -- there is nothing to tolerate."""
import ctypes as C

import numpy as np
import pytest
import torch

import arcvae_oracle as O
import beam_ref as R
import kbest_ref as KB
import length_norm_ref as LN
from helpers import TINY, bits as _bits, dev as _dev, ending_model, lib as _lib, sampling_vae, ws_bytes

pytestmark = pytest.mark.gpu
END, PAD = 2, 0
B = 4

_tables = {}


def _table(V, T, temp, kind, rows=B):
    """(step terms, device table, device lse) of a case: made once, shared, never modified."""
    key = (V, T, temp, kind, rows)
    if key not in _tables:
        table, lse = KB.make_table(np.random.RandomState(V * 1000 + T), rows, V, kind, temp, END)
        lp = R.step_terms(table, lse, temp)
        lp.setflags(write=False)
        _tables[key] = (lp, _dev(table, torch.float32), _dev(lse, torch.float32))
    return _tables[key]


def _f32(*shape):
    return torch.full(shape, 7.0, dtype=torch.float32, device="cuda")


def _i32(*shape):
    return torch.full(shape, -7, dtype=torch.int32, device="cuda")


def _viterbi_norm(table_d, lse_d, div, rows, V, T, min_len, temp, pad=PAD, profile=True, keep_ws=False):
    """-> tokens, keys, raw, lengths, by_length, open_score (host arrays; the last two None without `profile`) [, the scratch]."""
    L = _lib()
    n = ws_bytes("viterbi", rows, V, T)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok, key, raw, ln = _i32(rows, T), _f32(rows), _f32(rows), _i32(rows)
    byl, op = (_f32(rows, T), _f32(rows)) if profile else (None, None)
    div_d = None if div is None else _dev(div, torch.float32)
    L.call("arcvae_dec_viterbi_norm", L.ptr(table_d), L.ptr(lse_d), L.ptr(div_d), L.ptr(tok), L.ptr(key), L.ptr(raw), L.ptr(ln),
           L.ptr(byl), L.ptr(op), L.ptr(ws), n, rows, V, T, min_len, END, pad, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    out = tuple(None if a is None else a.cpu().numpy() for a in (tok, key, raw, ln, byl, op))
    return out + (ws,) if keep_ws else out


def _viterbi(table_d, lse_d, rows, V, T, min_len, temp):
    L = _lib()
    n = ws_bytes("viterbi", rows, V, T)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok, sc, ln = _i32(rows, T), _f32(rows), _i32(rows)
    L.call("arcvae_dec_viterbi", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok), L.ptr(sc), L.ptr(ln), L.ptr(ws), n, rows, V, T, min_len,
           END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), sc.cpu().numpy(), ln.cpu().numpy()


def _kbest_norm(table_d, lse_d, div, rows, V, K, T, min_len, temp, norm=True):
    """arcvae_dec_kbest_norm (or, norm=False, arcvae_dec_kbest: then raw is None) -> tokens, keys, raw, lengths."""
    L = _lib()
    n = ws_bytes("kbest", rows, V, K, T)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok, key, raw, ln = _i32(rows, K, T), _f32(rows, K), _f32(rows, K), _i32(rows, K)
    if norm:
        div_d = None if div is None else _dev(div, torch.float32)
        L.call("arcvae_dec_kbest_norm", L.ptr(table_d), L.ptr(lse_d), L.ptr(div_d), L.ptr(tok), L.ptr(key), L.ptr(raw), L.ptr(ln),
               L.ptr(ws), n, rows, V, K, T, min_len, END, PAD, float(temp), L.stream_ptr())
    else:
        L.call("arcvae_dec_kbest", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok), L.ptr(key), L.ptr(ln), L.ptr(ws), n, rows, V, K, T,
               min_len, END, PAD, float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy(), key.cpu().numpy(), raw.cpu().numpy() if norm else None, ln.cpu().numpy()


def _logprob(table_d, lse_d, tok, rows, V, temp):
    """arcvae_dec_sequence_logprob of host tokens [rows, T] on the device table."""
    L = _lib()
    tok_d = _dev(tok, torch.int32)
    out = torch.empty(rows, dtype=torch.float32, device="cuda")
    L.call("arcvae_dec_sequence_logprob", L.ptr(table_d), L.ptr(lse_d), L.ptr(tok_d), L.ptr(out), rows, tok.shape[1], V, END,
           float(temp), L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _min_lens(T):
    return sorted({0, min(3, T), T})


def _runs(T):
    """(table kind, temperature, divisors) of a case: alpha 0.5 and 1 at both temperatures, the tie array on the exact table."""
    return [("normal", temp, LN.divisors(alpha, T)) for temp in (1.0, 0.7) for alpha in (0.5, 1.0)] + [("q8d", 1.0, LN.tie_divisors(T))]


# V 5 and 12 (below a wave), 80 (the workload: staged, three parts), 97 (the first V that is not staged), 256 (one part, read through
# L2); max_len 1 (no recursion), 8, 16, and 40 at V 256: a back-trace of two staged chunks (32 steps of 256 bytes each).
VT = [(V, T) for V in (5, 12, 80, 97, 256) for T in (1, 8, 16)] + [(256, 40)]


@pytest.mark.parametrize("V,T", VT)
def test_viterbi_norm_kernel_is_the_fp32_restatement(V, T):
    """Tokens, lengths, by_length and the bits of key, raw score and open score equal the restatement's, for alpha 0.5 and 1, the
    tie divisors on the exact table, min_len 0, 3 and max_len, temperature 1 and 0.7; and raw_score is what the sequence
    log-likelihood kernel returns for the tokens."""
    for kind, temp, d in _runs(T):
        lp, table_d, lse_d = _table(V, T, temp, kind)
        for min_len in _min_lens(T):
            tok, key, raw, ln, byl, op = _viterbi_norm(table_d, lse_d, d, B, V, T, min_len, temp)
            rtok, rkey, rraw, rln, rbyl, rop = LN.viterbi_norm(lp, B, V, T, min_len, END, PAD, d)
            what = f"{kind} T {temp} min_len {min_len} d {d[:3]}"
            np.testing.assert_array_equal(ln, rln, err_msg=what)
            np.testing.assert_array_equal(tok, rtok, err_msg=what)
            np.testing.assert_array_equal(_bits(key), _bits(rkey), err_msg=what)
            np.testing.assert_array_equal(_bits(raw), _bits(rraw), err_msg=what)
            np.testing.assert_array_equal(_bits(byl), _bits(rbyl), err_msg=what)
            np.testing.assert_array_equal(_bits(op), _bits(rop), err_msg=what)
            np.testing.assert_array_equal(_bits(_logprob(table_d, lse_d, tok, B, V, temp)), _bits(raw), err_msg=what)
            if min_len == T:
                assert np.all(ln == T) and not np.any(tok == END)
            # the profile is optional: without it the same result
            tok2, key2, raw2, ln2, _, _ = _viterbi_norm(table_d, lse_d, d, B, V, T, min_len, temp, profile=False)
            assert np.array_equal(tok2, tok) and np.array_equal(ln2, ln)
            assert np.array_equal(_bits(key2), _bits(key)) and np.array_equal(_bits(raw2), _bits(raw))


@pytest.mark.parametrize("V,T", VT)
def test_unit_divisors_are_the_viterbi_kernel(V, T):
    """len_div all ones, and NULL: tokens, length and score bits of arcvae_dec_viterbi on the same device table; raw = score."""
    for kind, temp in (("normal", 0.7), ("q8d", 1.0)):
        _, table_d, lse_d = _table(V, T, temp, kind)
        for min_len in _min_lens(T):
            vtok, vsc, vln = _viterbi(table_d, lse_d, B, V, T, min_len, temp)
            for d in (np.ones(T, dtype=np.float32), None):
                tok, key, raw, ln, _, _ = _viterbi_norm(table_d, lse_d, d, B, V, T, min_len, temp)
                np.testing.assert_array_equal(tok, vtok)
                np.testing.assert_array_equal(ln, vln)
                np.testing.assert_array_equal(_bits(key), _bits(vsc))
                np.testing.assert_array_equal(_bits(raw), _bits(vsc))


@pytest.mark.parametrize("V,T", [(4, 5), (5, 6)])
def test_the_earliest_end_wins_a_tie_on_the_device(V, T):
    """48 rows of the exact table with the tie divisors: tables of tests/test_length_norm_ref.py on which the best key IS attained
    at more than one length in some rows (asserted from the kernel's own profile).  The kernel returns the restatement's tokens
    and lengths there: the shortest of the tying end candidates; K-best at K 8 agrees with its restatement on the same rows."""
    rows, d, ties = 48, LN.tie_divisors(T), 0
    table, lse = KB.make_table(np.random.RandomState(V * 100 + T), rows, V, "q8d", 1.0, END)
    lp, table_d, lse_d = R.step_terms(table, lse, 1.0), _dev(table, torch.float32), _dev(lse, torch.float32)
    for min_len in (0, 1, 2):
        tok, key, raw, ln, byl, op = _viterbi_norm(table_d, lse_d, d, rows, V, T, min_len, 1.0)
        rtok, rkey, _, rln, _, _ = LN.viterbi_norm(lp, rows, V, T, min_len, END, PAD, d)
        np.testing.assert_array_equal(ln, rln)
        np.testing.assert_array_equal(tok, rtok)
        np.testing.assert_array_equal(_bits(key), _bits(rkey))
        cand = byl / d                                             # exact: multiples of 1/8 over powers of two
        cand[:, :min_len] = -np.inf
        open_key = op / d[T - 1]
        for b in range(rows):
            at = np.flatnonzero(cand[b] == key[b])
            if at.size + (open_key[b] == key[b]) > 1:
                ties += 1
                assert at.size and ln[b] == at[0] + 1
        ktok, kkey, kraw, kln = _kbest_norm(table_d, lse_d, d, rows, V, 8, T, min_len, 1.0)
        rktok, rkkey, rkraw, rkln = LN.kbest_norm(lp, rows, V, 8, T, min_len, END, PAD, d)
        np.testing.assert_array_equal(kln, rkln)
        np.testing.assert_array_equal(ktok, rktok)
        np.testing.assert_array_equal(_bits(kkey), _bits(rkkey))
        np.testing.assert_array_equal(_bits(kraw), _bits(rkraw))
    assert ties >= 1


def test_the_penalty_moves_the_chosen_lengths():
    """V 12, T 16, eight rows of the "normal" table: the lengths chosen with alpha = 0.5 are not all those of alpha = 0
    (tests/test_length_norm_ref.py shows the restatement satisfies this on the same table)."""
    V, T, rows = 12, 16, 8
    _, table_d, lse_d = _table(V, T, 1.0, "normal", rows)
    l0 = _viterbi_norm(table_d, lse_d, LN.divisors(0.0, T), rows, V, T, 0, 1.0)[3]
    l5 = _viterbi_norm(table_d, lse_d, LN.divisors(0.5, T), rows, V, T, 0, 1.0)[3]
    print("lengths at alpha 0:", l0.tolist(), "at alpha 0.5:", l5.tolist())
    assert not np.array_equal(l0, l5)


# V 12 and 80 (groups of 16 lanes, staged), 129 and 256 (a wave per column; 256 x 32: the largest LDS footprint), K 1, 4 and 32,
# max_len 1 (no recursion: only the two arrivals) and 8.
VKT = [(V, K, T) for V in (12, 80, 129, 256) for K in (1, 4, 32) for T in (1, 8)]


# (table, temperature, divisors, min_len 0 or 3): a case of its own each, the restatement of V 256 x K 32 taking two seconds
KRUNS = [("normal", 1.0, "alpha", 0), ("normal", 0.7, "alpha", 3), ("q8d", 1.0, "ties", 0), ("q8d", 1.0, "ties", 3)]


@pytest.mark.parametrize("kind,temp,divs,min_len", KRUNS)
@pytest.mark.parametrize("V,K,T", VKT)
def test_kbest_norm_kernel_is_the_fp32_restatement(V, K, T, kind, temp, divs, min_len):
    """Tokens, lengths and the bits of keys and raw scores equal the restatement's; the keys descend; each raw score is what the
    sequence log-likelihood kernel returns for its tokens; K = 1 equals arcvae_dec_viterbi_norm on the same device table."""
    d = LN.divisors(0.5, T) if divs == "alpha" else LN.tie_divisors(T)
    min_len = min(min_len, T)
    lp, table_d, lse_d = _table(V, T, temp, kind, 3)
    rows = 3
    tok, key, raw, ln = _kbest_norm(table_d, lse_d, d, rows, V, K, T, min_len, temp)
    rtok, rkey, rraw, rln = LN.kbest_norm(lp, rows, V, K, T, min_len, END, PAD, d)
    what = f"{kind} T {temp} min_len {min_len}"
    np.testing.assert_array_equal(ln, rln, err_msg=what)
    np.testing.assert_array_equal(tok, rtok, err_msg=what)
    np.testing.assert_array_equal(_bits(key), _bits(rkey), err_msg=what)
    np.testing.assert_array_equal(_bits(raw), _bits(rraw), err_msg=what)
    assert np.all(key[:, :-1] >= key[:, 1:])
    for j in range(K):
        full = ln[:, j] > 0
        lpj = _logprob(table_d, lse_d, tok[:, j, :].copy(), rows, V, temp)
        np.testing.assert_array_equal(_bits(lpj[full]), _bits(raw[full, j]), err_msg=what)
        assert np.all(raw[~full, j] == -np.inf) and np.all(key[~full, j] == -np.inf) and np.all(tok[~full, j] == PAD)
    if K == 1:
        vtok, vkey, vraw, vln, _, _ = _viterbi_norm(table_d, lse_d, d, rows, V, T, min_len, temp)
        np.testing.assert_array_equal(tok[:, 0], vtok)
        np.testing.assert_array_equal(ln[:, 0], vln)
        np.testing.assert_array_equal(_bits(key[:, 0]), _bits(vkey))
        np.testing.assert_array_equal(_bits(raw[:, 0]), _bits(vraw))


@pytest.mark.parametrize("V,K,T", [(12, 4, 8), (80, 32, 8), (129, 4, 8), (256, 32, 8), (12, 32, 1)])
def test_unit_divisors_are_the_kbest_kernel(V, K, T):
    """len_div all ones, and NULL: tokens, lengths and score bits of arcvae_dec_kbest on the same device table; raw = scores."""
    for kind, temp, min_len in (("normal", 0.7, 0), ("q8d", 1.0, min(3, T))):
        _, table_d, lse_d = _table(V, T, temp, kind, 3)
        ktok, ksc, _, kln = _kbest_norm(table_d, lse_d, None, 3, V, K, T, min_len, temp, norm=False)
        for d in (np.ones(T, dtype=np.float32), None):
            tok, key, raw, ln = _kbest_norm(table_d, lse_d, d, 3, V, K, T, min_len, temp)
            np.testing.assert_array_equal(tok, ktok)
            np.testing.assert_array_equal(ln, kln)
            np.testing.assert_array_equal(_bits(key), _bits(ksc))
            np.testing.assert_array_equal(_bits(raw), _bits(ksc))


def test_kbest_norm_row_loop():
    """B = ARCVAE_KBEST_ROWS_IN_FLIGHT + 6 rows of seven distinct tables repeated with period 7 (a workgroup's second row differs
    from its first): every row equals the restatement of its table, the result's raw scores included."""
    V, K, T = 5, 2, 4
    per_row = 2 * T * V * K
    G = ws_bytes("kbest", 1 << 20, V, K, T) // per_row
    rows = G + 6
    d = LN.divisors(0.5, T)
    table7, lse7 = KB.make_table(np.random.RandomState(77), 7, V, "q8d", 1.0, END)
    rtok, rkey, rraw, rln = LN.kbest_norm(R.step_terms(table7, lse7, 1.0), 7, V, K, T, 0, END, PAD, d)
    idx = np.arange(rows) % 7
    table = table7.reshape(7, V, V)[idx].reshape(rows * V, V)
    lse = lse7.reshape(7, V)[idx].reshape(rows * V)
    tok, key, raw, ln = _kbest_norm(_dev(table, torch.float32), _dev(lse, torch.float32), d, rows, V, K, T, 0, 1.0)
    np.testing.assert_array_equal(tok, rtok[idx])
    np.testing.assert_array_equal(ln, rln[idx])
    np.testing.assert_array_equal(_bits(key), _bits(rkey[idx]))
    np.testing.assert_array_equal(_bits(raw), _bits(rraw[idx]))


def _trace(ws, lengths, rows, V, T, pad):
    L = _lib()
    tok = _i32(rows, T)
    n_d = _dev(np.asarray(lengths, dtype=np.int32), torch.int32)
    L.call("arcvae_dec_viterbi_trace", L.ptr(ws), ws.numel(), L.ptr(n_d), L.ptr(tok), rows, V, T, END, pad, L.stream_ptr())
    torch.cuda.synchronize()
    return tok.cpu().numpy()


@pytest.mark.parametrize("V,T,lengths", [(12, 16, tuple(range(1, 17))), (256, 40, (1, 33, 40))])
def test_trace_at_every_length(V, T, lengths):
    """One forward call, then a trace per n: no end token before position n-1, the end token there, pads after; the tokens are the
    restatement's; their sequence log-likelihood is by_length[:, n-1] bit for bit where that is finite.  n = 0 gives pads only;
    lengths outside [0, max_len] are clamped; rows may ask for different lengths."""
    pad, temp = 255, 1.0
    lp, table_d, lse_d = _table(V, T, temp, "normal")
    *_, byl, _, ws = _viterbi_norm(table_d, lse_d, LN.divisors(0.5, T), B, V, T, 3, temp, pad=pad, keep_ws=True)
    for n in lengths:
        tok = _trace(ws, [n] * B, B, V, T, pad)
        assert np.all(tok[:, n - 1] == END) and not np.any(tok[:, :n - 1] == END) and np.all(tok[:, n:] == pad)
        np.testing.assert_array_equal(tok, LN.trace(lp, B, V, T, [n] * B, END, pad))
        fin = np.isfinite(byl[:, n - 1])
        assert fin.all()                                           # (these tables reach the end token from everywhere)
        np.testing.assert_array_equal(_bits(_logprob(table_d, lse_d, tok, B, V, temp)[fin]), _bits(byl[fin, n - 1]))
    assert np.all(_trace(ws, [0] * B, B, V, T, pad) == pad)
    mixed = [0, -5, T + 9, min(7, T)]
    np.testing.assert_array_equal(_trace(ws, mixed, B, V, T, pad), LN.trace(lp, B, V, T, mixed, END, pad))
    # a plain arcvae_dec_viterbi call leaves the same pointers
    L = _lib()
    ws2 = torch.zeros_like(ws)
    L.call("arcvae_dec_viterbi", L.ptr(table_d), L.ptr(lse_d), L.ptr(_i32(B, T)), L.ptr(_f32(B)), L.ptr(_i32(B)), L.ptr(ws2),
           ws2.numel(), B, V, T, 0, END, PAD, temp, L.stream_ptr())
    np.testing.assert_array_equal(_trace(ws2, [T] * B, B, V, T, pad), _trace(ws, [T] * B, B, V, T, pad))


def test_argument_errors_return_codes():
    L = _lib()
    lib = L.load()
    rows, V, K, T = 2, 12, 4, 8
    table = torch.zeros(rows * 257, 257, device="cuda")         # (large enough for the V = 257 calls, should they launch)
    lse = torch.zeros(rows * 257, device="cuda")
    tok = torch.zeros(rows, 33, T + 1, dtype=torch.int32, device="cuda")
    sc, raw = torch.zeros(rows, 33, device="cuda"), torch.zeros(rows, 33, device="cuda")
    ln = torch.zeros(rows, 33, dtype=torch.int32, device="cuda")
    byl, op = torch.zeros(rows, T + 1, device="cuda"), torch.zeros(rows, device="cuda")
    div = torch.ones(T + 1, device="cuda")
    ws = torch.zeros(rows * 2 * (T + 1) * 257 * 33, dtype=torch.uint8, device="cuda")
    need_v, need_k = rows * V * T, rows * 2 * T * V * K
    assert ws_bytes("viterbi", rows, V, T) == need_v and ws_bytes("kbest", rows, V, K, T) == need_k

    def vn(ws_bytes=ws.numel(), V_=V, T_=T, min_len=0, end=END, pad=PAD, temp=1.0, x=table, l=lse, d=div, out=tok, score=sc, r=raw,
           length=ln, prof=byl, opn=op, scratch=ws):
        return lib.arcvae_dec_viterbi_norm(L.ptr(x), L.ptr(l), L.ptr(d), L.ptr(out), L.ptr(score), L.ptr(r), L.ptr(length),
                                           L.ptr(prof), L.ptr(opn), L.ptr(scratch), ws_bytes, rows, V_, T_, min_len, end, pad, temp,
                                           L.stream_ptr())

    def tr(ws_bytes=ws.numel(), V_=V, T_=T, end=END, pad=PAD, n=ln, out=tok, scratch=ws, rows_=rows):
        return lib.arcvae_dec_viterbi_trace(L.ptr(scratch), ws_bytes, L.ptr(n), L.ptr(out), rows_, V_, T_, end, pad, L.stream_ptr())

    def kn(ws_bytes=ws.numel(), V_=V, K_=K, T_=T, min_len=0, end=END, pad=PAD, temp=1.0, x=table, l=lse, d=div, out=tok, score=sc,
           r=raw, length=ln, scratch=ws):
        return lib.arcvae_dec_kbest_norm(L.ptr(x), L.ptr(l), L.ptr(d), L.ptr(out), L.ptr(score), L.ptr(r), L.ptr(length),
                                         L.ptr(scratch), ws_bytes, rows, V_, K_, T_, min_len, end, pad, temp, L.stream_ptr())

    for f in (vn, kn):
        assert f(V_=0) == -1 and f(V_=257) == -1
        assert f(end=V) == -1 and f(end=-1) == -1 and f(pad=256) == -1 and f(pad=-1) == -1
        assert f(min_len=T + 1) == -1 and f(min_len=-1) == -1 and f(T_=0) == -1
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert f(temp=bad) == -1
        assert f(x=None) == -1 and f(l=None) == -1 and f(out=None) == -1 and f(score=None) == -1 and f(r=None) == -1
        assert f(length=None) == -1 and f(scratch=None) == -1
    assert kn(K_=0) == -1 and kn(K_=33) == -1
    assert vn(ws_bytes=need_v - 1) == -1 and kn(ws_bytes=need_k - 1) == -1 and tr(ws_bytes=need_v - 1) == -1
    assert tr(V_=0) == -1 and tr(V_=257) == -1 and tr(T_=0) == -1 and tr(end=V) == -1 and tr(end=-1) == -1
    assert tr(pad=256) == -1 and tr(pad=-1) == -1 and tr(rows_=0) == -1
    assert tr(n=None) == -1 and tr(out=None) == -1 and tr(scratch=None) == -1
    # and the valid calls still run: the optional pointers NULL, the exact scratch size
    assert vn(ws_bytes=need_v, d=None, prof=None, opn=None) == 0 and vn(ws_bytes=need_v) == 0
    ln.fill_(T)
    assert tr(ws_bytes=need_v) == 0
    assert kn(ws_bytes=need_k, d=None) == 0 and kn(ws_bytes=need_k) == 0
    torch.cuda.synchronize()
    assert np.all(ln.cpu().numpy().reshape(-1)[:rows * K] >= 1)


# ---- model level: TINY, B 16 ---------------------------------------------------------------------------------------------------
B_M, T_M, K_M = 16, 20, 4


@pytest.fixture(scope="module")
def model():
    return ending_model(B_M, END)


def _engine_terms(samp, T, temp):
    """The fp32 step terms of the table the sampler's last call left in its workspace, with the device's own lse."""
    ws = samp.decoder.workspace(B_M, T)
    lse = samp.decoder.table_lse(ws, temp)
    torch.cuda.synchronize()
    return R.step_terms(ws.logits.cpu().numpy().reshape(B_M * samp.decoder.vocab_size, -1), lse.cpu().numpy(), temp)


@pytest.mark.parametrize("temp,min_len", [(1.0, 0), (0.7, 4)])
def test_generate_map_with_a_length_penalty(model, temp, min_len):
    cfg, _, vae, cond, _ = model
    samp = vae.decoder_sampling
    out = samp.generate_map(None, cond, max_length=T_M, temperature=temp, min_length=min_len, length_penalty=0.5,
                            early_stopping=False)
    assert len(out) == 3
    tok, key, raw = out
    assert tok.shape == (B_M, T_M) and tok.dtype == torch.int32 and key.shape == raw.shape == (B_M,) and key.dtype == torch.float32
    rtok, rkey, rraw, rln, _, _ = LN.viterbi_norm(_engine_terms(samp, T_M, temp), B_M, cfg.V, T_M, min_len, END, PAD,
                                                  LN.divisors(0.5, T_M))
    np.testing.assert_array_equal(tok.cpu().numpy(), rtok)
    np.testing.assert_array_equal(_bits(key.cpu().numpy()), _bits(rkey))
    np.testing.assert_array_equal(_bits(raw.cpu().numpy()), _bits(rraw))
    lpm = samp.decoder.sequence_log_prob(tok, cond, temperature=temp).cpu().numpy()
    np.testing.assert_array_equal(_bits(lpm), _bits(raw.cpu().numpy()))
    # the same divisors as a list, an array and a tensor; early stopping cuts at the longest sequence
    d = LN.divisors(0.5, T_M)
    for given in (d.tolist(), d, torch.as_tensor(d), torch.as_tensor(d).cuda()):
        tok2, key2, raw2 = samp.generate_map(None, cond, max_length=T_M, temperature=temp, min_length=min_len, length_penalty=given)
        assert tok2.shape == (B_M, int(rln.max())) and np.array_equal(tok2.cpu().numpy(), rtok[:, :rln.max()])
        np.testing.assert_array_equal(_bits(key2.cpu().numpy()), _bits(rkey))
    # without the keyword: the two-tuple as before, and alpha = 0 returns its tokens and scores
    tok0, sc0 = samp.generate_map(None, cond, max_length=T_M, temperature=temp, min_length=min_len)
    tokz, keyz, rawz = samp.generate_map(None, cond, max_length=T_M, temperature=temp, min_length=min_len, length_penalty=0.0)
    assert np.array_equal(tok0.cpu().numpy(), tokz.cpu().numpy())
    np.testing.assert_array_equal(_bits(sc0.cpu().numpy()), _bits(keyz.cpu().numpy()))
    np.testing.assert_array_equal(_bits(sc0.cpu().numpy()), _bits(rawz.cpu().numpy()))


def test_generate_kbest_with_a_length_penalty(model):
    cfg, _, vae, cond, _ = model
    samp = vae.decoder_sampling
    out = samp.generate_kbest(None, cond, max_length=T_M, num_best=K_M, length_penalty=0.5, early_stopping=False)
    assert len(out) == 3
    tok, key, raw = out
    assert tok.shape == (B_M, K_M, T_M) and key.shape == raw.shape == (B_M, K_M)
    rtok, rkey, rraw, rln = LN.kbest_norm(_engine_terms(samp, T_M, 1.0), B_M, cfg.V, K_M, T_M, 0, END, PAD, LN.divisors(0.5, T_M))
    np.testing.assert_array_equal(tok.cpu().numpy(), rtok)
    np.testing.assert_array_equal(_bits(key.cpu().numpy()), _bits(rkey))
    np.testing.assert_array_equal(_bits(raw.cpu().numpy()), _bits(rraw))
    mtok, mkey, mraw = samp.generate_map(None, cond, max_length=T_M, length_penalty=0.5, early_stopping=False)
    np.testing.assert_array_equal(tok[:, 0].cpu().numpy(), mtok.cpu().numpy())       # rank 0 is generate_map's
    np.testing.assert_array_equal(_bits(key[:, 0].cpu().numpy()), _bits(mkey.cpu().numpy()))
    cut, _, _ = samp.generate_kbest(None, cond, max_length=T_M, num_best=K_M, length_penalty=0.5)
    assert cut.shape == (B_M, K_M, int(rln.max())) and np.array_equal(cut.cpu().numpy(), rtok[:, :, :rln.max()])
    assert len(samp.generate_kbest(None, cond, max_length=T_M, num_best=K_M)) == 2


def test_generate_exact_with_a_length_penalty(model):
    cfg, _, vae, cond, _ = model
    samp = vae.decoder_sampling
    tok, _, _ = samp.generate_map(None, cond, max_length=16, length_penalty=0.5)
    got = vae.generate(B_M, cond, max_length=16, exact=True, length_penalty=0.5)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), tok.cpu().numpy())
    ktok, _, _ = samp.generate_kbest(None, cond, max_length=16, num_best=K_M, length_penalty=0.5)
    got = vae.generate(B_M, cond, max_length=16, exact=True, length_penalty=0.5, num_best=K_M)
    assert got.dim() == 3 and np.array_equal(got.cpu().numpy(), ktok.cpu().numpy())
    for kw in (dict(), dict(beam_width=4), dict(sample=True)):
        with pytest.raises(ValueError):
            vae.generate(B_M, cond, max_length=16, length_penalty=0.5, **kw)       # length_penalty needs exact=True
    bad = [float("nan"), float("inf"), -float("inf"), 400.0, -400.0, [1.0] * 15, [1.0] * 17, [1.0] * 15 + [0.0],
           [1.0] * 15 + [-2.0], [1.0] * 15 + [float("nan")], [1.0] * 15 + [float("inf")], np.ones((2, 8)), torch.ones(4, 4), "half",
           [1.0] * 15 + [1e-60]]
    for lp in bad:
        for method, kw in ((samp.generate_map, dict()), (samp.generate_kbest, dict(num_best=K_M))):
            with pytest.raises(ValueError):
                method(None, cond, max_length=16, length_penalty=lp, **kw)


def test_best_by_length_and_generate_of_length(model):
    cfg, _, vae, cond, _ = model
    samp = vae.decoder_sampling
    byl, op = samp.best_by_length(cond, max_length=T_M, temperature=0.7)
    assert byl.shape == (B_M, T_M) and op.shape == (B_M,) and byl.dtype == op.dtype == torch.float32
    *_, rbyl, rop = LN.viterbi_norm(_engine_terms(samp, T_M, 0.7), B_M, cfg.V, T_M, 0, END, PAD, None)
    np.testing.assert_array_equal(_bits(byl.cpu().numpy()), _bits(rbyl))
    np.testing.assert_array_equal(_bits(op.cpu().numpy()), _bits(rop))
    # the best score of any length is generate_map's
    _, msc = samp.generate_map(None, cond, max_length=T_M, temperature=0.7)
    best = torch.maximum(byl.max(dim=1).values, op)
    np.testing.assert_array_equal(_bits(best.cpu().numpy()), _bits(msc.cpu().numpy()))
    per_row = (np.arange(B_M) % T_M + 1).astype(np.int64)
    for lengths, n in ((7, np.full(B_M, 7)), (torch.as_tensor(per_row), per_row), (per_row.tolist(), per_row),
                       (torch.as_tensor(per_row, dtype=torch.int32).cuda(), per_row)):
        tok, sc = samp.generate_of_length(cond, lengths, max_length=T_M, temperature=0.7)
        assert tok.shape == (B_M, int(n.max())) and tok.dtype == torch.int32 and sc.shape == (B_M,)
        t = tok.cpu().numpy()
        for b in range(B_M):
            assert t[b, n[b] - 1] == END and END not in t[b, :n[b] - 1] and np.all(t[b, n[b]:] == PAD)
        np.testing.assert_array_equal(_bits(sc.cpu().numpy()), _bits(rbyl[np.arange(B_M), n - 1]))
        lpm = samp.decoder.sequence_log_prob(tok, cond, temperature=0.7).cpu().numpy()
        np.testing.assert_array_equal(_bits(lpm), _bits(sc.cpu().numpy()))
    for bad in (0, T_M + 1, [1] * (B_M - 1), [0] * B_M, 2.5, [[1] * B_M]):
        with pytest.raises(ValueError):
            samp.generate_of_length(cond, bad, max_length=T_M)
    for kw in (dict(temperature=0.0), dict(temperature=float("inf")), dict(max_length=0)):
        with pytest.raises(ValueError):
            samp.best_by_length(cond, **{"max_length": T_M, **kw})


def test_which_entry_points_run(monkeypatch):
    """Without the new keywords the methods launch exactly what they launched before; with them, and the two new methods, one
    dense pass, one lse and their own kernels (recorded as tests/test_sampler_calls_gpu.py does)."""
    samp = sampling_vae(TINY, O.init_params(TINY, 1234)).decoder_sampling
    cond = np.random.RandomState(3).standard_normal((3, TINY.C)).astype(np.float32)
    L = _lib()
    real, names = L.check, []

    def recorder(rc, what):
        if not what.endswith("_ws_bytes"):
            names.append(what)
        real(rc, what)

    monkeypatch.setattr(L, "check", recorder)

    def took(f, *a, **kw):
        names.clear()
        f(*a, **kw)
        return list(names)

    dense, lse = "arcvae_dec_forward_dense", "arcvae_dec_row_lse"
    assert took(samp.generate_map, None, cond, max_length=6) == [dense, lse, "arcvae_dec_viterbi"]
    assert took(samp.generate_kbest, None, cond, max_length=6) == [dense, lse, "arcvae_dec_kbest"]
    assert took(samp.generate_map, None, cond, max_length=6, length_penalty=None) == [dense, lse, "arcvae_dec_viterbi"]
    assert took(samp.generate_kbest, None, cond, max_length=6, length_penalty=None) == [dense, lse, "arcvae_dec_kbest"]
    assert took(samp.generate_map, None, cond, max_length=6, length_penalty=0.5) == [dense, lse, "arcvae_dec_viterbi_norm"]
    assert took(samp.generate_kbest, None, cond, max_length=6, length_penalty=0.5) == [dense, lse, "arcvae_dec_kbest_norm"]
    assert took(samp.best_by_length, cond, max_length=6) == [dense, lse, "arcvae_dec_viterbi_norm"]
    assert took(samp.generate_of_length, cond, 3, max_length=6) == [dense, lse, "arcvae_dec_viterbi_norm", "arcvae_dec_viterbi_trace"]
    with pytest.raises(ValueError):
        took(samp.generate_map, None, cond, max_length=6, length_penalty=float("nan"))
    assert names == []                                             # a bad value is refused before any device work
