"""NumPy restatement of length-normalised exact decoding and the best-sequence-per-length profile over a dense decoder table (the
contracts of include/arcvae_hip.h arcvae_dec_viterbi_norm / arcvae_dec_viterbi_trace / arcvae_dec_kbest_norm; test
infrastructure, like chain_ref.py and kbest_ref.py, whose tables, step terms and list selection it uses).

Everything works in lp's dtype, one rounding per operation: a raw score is the left-to-right sum fl(s + lp), a KEY is
fl(raw / d_n) with d_n the divisor of the sequence's length n (the end token counts; a sequence without one has n = max_len).
In fp32 these are the kernels' operations; in fp64 the same formulas serve as an oracle.  enumerate_all lists every admissible
sequence's raw score and length, keys_of turns them into keys: what the restatements are checked against."""
from __future__ import annotations

import numpy as np

import beam_ref  # noqa: F401  (step_terms / sequence_logprob are what the callers pair this module with)
import chain_ref  # noqa: F401
import kbest_ref


def divisors(alpha: float, max_len: int) -> np.ndarray:
    """fp32(float(n) ** alpha), n = 1 .. max_len: computed in float64, rounded once (what the Python surface passes for a number)."""
    return np.array([float(n) ** float(alpha) for n in range(1, max_len + 1)], dtype=np.float64).astype(np.float32)


def tie_divisors(max_len: int) -> np.ndarray:
    """[1, 2, 2, 4, 4, 8, ..]: powers of two, so that on a "q8d" table (every raw score a small multiple of 1/8) every key is
    exact and keys tie across lengths."""
    return (2.0 ** (np.arange(1, max_len + 1) // 2)).astype(np.float32)


def _div(div, max_len: int, dtype) -> np.ndarray:
    d = np.ones(max_len, dtype=dtype) if div is None else np.asarray(div).astype(dtype)
    assert d.shape == (max_len,)
    return d


def _forward(M: np.ndarray, V: int, max_len: int, end_token: int):
    """The Viterbi recursion of one row -> (bp [max_len, V], e [max_len] = the maximum into end_token at every step,
    a [V] = a_{max_len-1} with the end token's entry -inf)."""
    dt = M.dtype
    bp = np.zeros((max_len, V), dtype=np.int64)
    e = np.zeros(max_len, dtype=dt)
    a = (dt.type(0) + M[0]).astype(dt)
    for t in range(max_len):
        if t > 0:
            with np.errstate(invalid="ignore"):
                cand = (a[:, None] + M).astype(dt)                 # [u, v], one rounding per candidate; a[end] = -inf
            bp[t] = cand.argmax(axis=0)                            # the first (lowest) u of the maximum
            a = cand[bp[t], np.arange(V)]
        e[t] = a[end_token]
        a = a.copy()
        a[end_token] = -np.inf                                     # the end token never continues
    return bp, e, a


def _follow(bp: np.ndarray, out: np.ndarray, n: int, last: int) -> None:
    tok = last
    out[n - 1] = tok
    for t in range(n - 1, 0, -1):
        tok = int(bp[t, tok])
        out[t - 1] = tok


def viterbi_norm(lp: np.ndarray, B: int, V: int, max_len: int, min_len: int = 0, end_token: int = 2, pad_token: int = 0, div=None):
    """-> tokens [B, max_len] int32, keys [B], raw [B], lengths [B] int32, by_length [B, max_len], open_score [B].
    Candidates: e_t for t = min_len .. max_len-1 with key fl(e_t / d[t]); then ONE open candidate, the maximum raw
    a_{max_len-1}[v], v != end, the lowest v of a tie, with key fl(. / d[max_len-1]).  The first is taken; a later one replaces
    it only when its key is strictly greater."""
    dt = lp.dtype
    d = _div(div, max_len, dt)
    ninf = dt.type(-np.inf)
    tokens = np.full((B, max_len), pad_token, dtype=np.int32)
    keys, raws, opens = (np.full(B, ninf, dtype=dt) for _ in range(3))
    lengths = np.full(B, max_len, dtype=np.int32)
    by_length = np.zeros((B, max_len), dtype=dt)
    for b in range(B):
        bp, e, a = _forward(lp[b * V:(b + 1) * V], V, max_len, end_token)
        by_length[b] = e
        chosen, key, raw, n, last = False, ninf, ninf, max_len, 0
        for t in range(min_len, max_len):
            k = dt.type(e[t] / d[t])
            if not chosen or k > key:
                chosen, key, raw, n, last = True, k, e[t], t + 1, end_token
        os_, ow, have = ninf, 0, False
        for v in range(V):
            if v != end_token and (not have or a[v] > os_):
                os_, ow, have = a[v], v, True
        opens[b] = os_
        k = dt.type(os_ / d[max_len - 1])
        if not chosen or k > key:
            key, raw, n, last = k, os_, max_len, ow
        keys[b], raws[b], lengths[b] = key, raw, n
        _follow(bp, tokens[b], n, last)
    return tokens, keys, raws, lengths, by_length, opens


def trace(lp: np.ndarray, B: int, V: int, max_len: int, lengths, end_token: int = 2, pad_token: int = 0) -> np.ndarray:
    """tokens [B, max_len]: per row the sequence that ends with end_token at position n-1 (n = lengths[b] clamped into
    [0, max_len]), followed back through the recursion's pointers, then pad_token; n = 0: pad tokens only."""
    tokens = np.full((B, max_len), pad_token, dtype=np.int32)
    for b in range(B):
        n = min(max(int(lengths[b]), 0), max_len)
        if n > 0:
            bp, _, _ = _forward(lp[b * V:(b + 1) * V], V, max_len, end_token)
            _follow(bp, tokens[b], n, end_token)
    return tokens


def kbest_norm(lp: np.ndarray, B: int, V: int, K: int, max_len: int, min_len: int = 0, end_token: int = 2, pad_token: int = 0,
               div=None):
    """-> tokens [B, K, max_len] int32, keys [B, K] (descending), raw [B, K], lengths [B, K] int32.  The lists of kbest_ref.kbest,
    on raw scores.  Arriving lists: for t = min_len .. max_len-1 the list into end_token at step t; then the first K of the
    stable sort by raw score descending of a_{max_len-1}[v], v != end ascending, by rank.  Keys fl(raw / d_n); each list is merged
    stably into the running result by key, the result's entries first on ties.  A slot is empty by its raw score (-inf):
    key and raw -inf, length 0, pad tokens."""
    dt = lp.dtype
    d = _div(div, max_len, dt)
    ninf = dt.type(-np.inf)
    tokens = np.full((B, K, max_len), pad_token, dtype=np.int32)
    keys = np.full((B, K), ninf, dtype=dt)
    raws = np.full((B, K), ninf, dtype=dt)
    lengths = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        M = lp[b * V:(b + 1) * V]
        bp_u = np.zeros((max_len, V, K), dtype=np.int64)
        bp_r = np.zeros((max_len, V, K), dtype=np.int64)
        a = np.full((V, K), ninf, dtype=dt)
        a[:, 0] = (dt.type(0) + M[0]).astype(dt)
        r_k = np.full(K, ninf, dtype=dt)
        r_s = np.full(K, ninf, dtype=dt)
        r_m = np.zeros((K, 3), dtype=np.int64)                     # (step, last token, rank)

        def arrive(s, meta, dn):
            nonlocal r_k, r_s, r_m
            k = (s / dn).astype(dt)                                # one division per entry; -inf stays -inf
            all_k, all_s, all_m = np.concatenate([r_k, k]), np.concatenate([r_s, s]), np.concatenate([r_m, meta])
            order = np.argsort(-all_k, kind="stable")[:K]
            r_k, r_s, r_m = all_k[order], all_s[order], all_m[order]

        for t in range(max_len):
            if t > 0:
                with np.errstate(invalid="ignore"):
                    cand = (a[:, :, None] + M[:, None, :]).astype(dt).reshape(V * K, V)      # [(u, r'), v]
                idx = kbest_ref.first_k_stable(cand, K)
                a = cand[idx, np.arange(V)[None, :]].T.copy()
                bp_u[t] = (idx // K).T
                bp_r[t] = (idx % K).T
            if t >= min_len:
                arrive(a[end_token].copy(), np.stack([np.full(K, t), np.full(K, end_token), np.arange(K)], axis=1), d[t])
            a[end_token] = ninf
        # the final list: (raw desc, v asc, rank asc), the first K
        flat = a.reshape(V * K)                                    # index v * K + r: already (v asc, r asc)
        order = np.argsort(-flat, kind="stable")[:K]
        arrive(flat[order].copy(), np.stack([np.full(order.size, max_len - 1), order // K, order % K], axis=1), d[max_len - 1])
        for j in range(K):
            if not r_s[j] > ninf:
                continue
            t, v, r = (int(x) for x in r_m[j])
            n = t + 1
            keys[b, j], raws[b, j], lengths[b, j] = r_k[j], r_s[j], n
            tokens[b, j, n - 1] = v
            for s in range(n - 1, 0, -1):
                v, r = int(bp_u[s, v, r]), int(bp_r[s, v, r])
                tokens[b, j, s - 1] = v
    return tokens, keys, raws, lengths


def enumerate_all(lp: np.ndarray, b: int, V: int, max_len: int, end_token: int = 2):
    """EVERY sequence of batch row b that ends with its first end_token or runs to max_len without one (min_len = 0), by
    enumeration, in lp's dtype -> (raw [N], n [N] int, ended [N] bool): the left-to-right sums, the lengths, and whether the
    sequence ends with end_token."""
    dt = lp.dtype
    M = lp[b * V:(b + 1) * V]
    others = np.array([v for v in range(V) if v != end_token], dtype=np.int64)
    s = np.zeros(1, dtype=dt)
    last = np.zeros(1, dtype=np.int64)
    raw, ns, ended = [], [], []
    for n in range(1, max_len + 1):
        e = (s + M[last, end_token]).astype(dt)
        raw.append(e)
        ns.append(np.full(e.size, n))
        ended.append(np.ones(e.size, dtype=bool))
        ext = (s[:, None] + M[last][:, others]).astype(dt)          # one rounding per extension
        last = np.tile(others, s.size)
        s = ext.reshape(-1)
        if n == max_len:
            raw.append(s)
            ns.append(np.full(s.size, n))
            ended.append(np.zeros(s.size, dtype=bool))
    return np.concatenate(raw), np.concatenate(ns), np.concatenate(ended)


def keys_of(raw: np.ndarray, n: np.ndarray, ended: np.ndarray, min_len: int, div) -> np.ndarray:
    """The key fl(raw / d_n) of every ADMISSIBLE sequence of enumerate_all's result under min_len (an end at position n-1 needs
    n-1 >= min_len), sorted descending."""
    ok = ~ended | (n - 1 >= min_len)
    d = np.asarray(div).astype(raw.dtype)
    k = (raw[ok] / d[n[ok] - 1]).astype(raw.dtype)
    return np.sort(k)[::-1]


def top(keys: np.ndarray, K: int) -> np.ndarray:
    """The K largest of a descending array, -inf where there are fewer."""
    out = np.full(K, -np.inf, dtype=keys.dtype)
    m = min(K, keys.size)
    out[:m] = keys[:m]
    return out
