"""NumPy restatement of exact K-best decoding over a dense decoder table (the contract of include/arcvae_hip.h arcvae_dec_kbest;
test infrastructure, like chain_ref.py and beam_ref.py).

A table is [B*V, V]: row b*V + c holds batch row b's logits after token c; the step terms lp come from beam_ref.step_terms (in
fp32 the kernel's two roundings).  kbest works in lp's dtype, one rounding per addition: in fp32 it performs the kernel's
operations, in fp64 the same formulas serve as an oracle.  brute_force_scores enumerates every admissible sequence."""
from __future__ import annotations

import itertools

import numpy as np

import beam_ref
import chain_ref


def first_k_stable(cand: np.ndarray, K: int) -> np.ndarray:
    """cand [N, C], N >= K -> idx [K, C]: per column the first K rows of a STABLE sort by value descending (what
    np.argsort(-cand, axis=0, kind="stable")[:K] returns, without sorting all N rows: the K-th largest value is found by
    selection, the rows above it are taken, then the earliest rows equal to it; only those K are sorted)."""
    N, C = cand.shape
    kth = np.partition(cand, N - K, axis=0)[N - K]                      # the K-th largest of every column
    above = cand > kth
    equal = cand == kth
    room = K - above.sum(axis=0)                                         # >= 1: how many rows equal to kth are taken
    take = above | (equal & (np.cumsum(equal, axis=0) <= room))
    cols, rows = np.nonzero(take.T)                                      # column-major: rows ascending within a column
    assert rows.size == K * C and np.array_equal(cols, np.repeat(np.arange(C), K))
    rows = rows.reshape(C, K)
    vals = cand[rows, np.arange(C)[:, None]]
    order = np.argsort(-vals, axis=1, kind="stable")
    return np.take_along_axis(rows, order, axis=1).T


def kbest(lp: np.ndarray, B: int, V: int, K: int, max_len: int, min_len: int = 0, end_token: int = 2, pad_token: int = 0):
    """-> tokens [B, K, max_len] int32, scores [B, K] (lp's dtype, descending), lengths [B, K] int32.
    a_t[v] = the first K of the candidates fl(a_{t-1}[u][r'] + lp(u, v)), u != end, enumerated (u asc, r' asc) and sorted stably
    by score descending; -inf = empty, never a candidate.  Result candidates: the lists into end_token of steps min_len ..
    max_len-1 by rank, then a_{max_len-1}[v] for v != end ascending by rank; the first K of their stable sort by score descending.
    A slot without a candidate: score -inf, length 0, pad tokens."""
    dt = lp.dtype
    ninf = dt.type(-np.inf)
    tokens = np.full((B, K, max_len), pad_token, dtype=np.int32)
    scores = np.full((B, K), ninf, dtype=dt)
    lengths = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        M = lp[b * V:(b + 1) * V]
        bp_u = np.zeros((max_len, V, K), dtype=np.int64)
        bp_r = np.zeros((max_len, V, K), dtype=np.int64)
        a = np.full((V, K), ninf, dtype=dt)
        a[:, 0] = (dt.type(0) + M[0]).astype(dt)
        # the running result: (score, step, last token, rank), kept sorted; a stable merge = the stable sort of all arrivals
        r_s = np.full(K, ninf, dtype=dt)
        r_m = np.zeros((K, 3), dtype=np.int64)

        def arrive(s, meta):
            nonlocal r_s, r_m
            all_s = np.concatenate([r_s, s])
            all_m = np.concatenate([r_m, meta])
            order = np.argsort(-all_s, kind="stable")[:K]
            r_s, r_m = all_s[order], all_m[order]

        for t in range(max_len):
            if t > 0:
                with np.errstate(invalid="ignore"):
                    cand = (a[:, :, None] + M[:, None, :]).astype(dt).reshape(V * K, V)      # [(u, r'), v], one rounding each
                idx = first_k_stable(cand, K)                                                   # [K, v]
                a = cand[idx, np.arange(V)[None, :]].T.copy()                                   # [v, K]
                bp_u[t] = (idx // K).T
                bp_r[t] = (idx % K).T
            if t >= min_len:
                arrive(a[end_token].copy(), np.stack([np.full(K, t), np.full(K, end_token), np.arange(K)], axis=1))
            a[end_token] = ninf                                                                 # the end token never continues
        for v in range(V):
            if v != end_token:
                arrive(a[v].copy(), np.stack([np.full(K, max_len - 1), np.full(K, v), np.arange(K)], axis=1))
        for j in range(K):
            if not r_s[j] > ninf:
                continue
            t, v, r = (int(x) for x in r_m[j])
            n = t + 1
            scores[b, j], lengths[b, j] = r_s[j], n
            tokens[b, j, n - 1] = v
            for s in range(n - 1, 0, -1):
                v, r = int(bp_u[s, v, r]), int(bp_r[s, v, r])
                tokens[b, j, s - 1] = v
    return tokens, scores, lengths


def brute_force_scores(lp: np.ndarray, b: int, V: int, max_len: int, min_len: int, end_token: int) -> np.ndarray:
    """The contract score of EVERY admissible sequence of batch row b, by enumeration, in lp's dtype, sorted descending."""
    dt = lp.dtype.type
    M = lp[b * V:(b + 1) * V]
    others = [v for v in range(V) if v != end_token]
    out = []

    def score(seq):
        s, c = dt(0), 0
        for x in seq:
            s = dt(s + M[c, x])
            c = x
        return s

    for n in range(1, max_len + 1):
        for body in itertools.product(others, repeat=n - 1):
            if n - 1 >= min_len:
                out.append(score(body + (end_token,)))
            if n == max_len:
                out.extend(score(body + (v,)) for v in others)
    return np.sort(np.array(out, dtype=lp.dtype))[::-1]


def top_scores(all_scores: np.ndarray, K: int) -> np.ndarray:
    """The K largest of brute_force_scores' result, -inf where there are fewer than K."""
    out = np.full(K, -np.inf, dtype=all_scores.dtype)
    n = min(K, all_scores.size)
    out[:n] = all_scores[:n]
    return out


def make_table(rs, B: int, V: int, kind: str, temperature: float = 1.0, end_token: int = 2, lower: float = 4.0):
    """-> (table [B*V, V] fp32, lse [B*V] fp32).  The kinds of chain_ref.make_table with beam_ref.row_lse, and "q8d": the "q8"
    table with the lse ROUNDED to multiples of 1/8.  The lse is an input of the kernel, so this is inside the contract; at
    temperature 1 every step term and every partial sum is then a small multiple of 1/8, exact in fp32, and ties are everywhere."""
    table = chain_ref.make_table(rs, B, V, "q8" if kind == "q8d" else kind, end_token, lower)
    lse = beam_ref.row_lse(table, temperature).astype(np.float32)
    if kind == "q8d":
        lse = (np.round(lse * 8) / 8).astype(np.float32)
    return table, lse
