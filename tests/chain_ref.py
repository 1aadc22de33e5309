"""NumPy restatement of exact MAP decoding (Viterbi) and the exact chain marginals over a dense decoder table (the contract of
include/arcvae_hip.h arcvae_dec_viterbi / arcvae_dec_chain_marginals; test infrastructure, like beam_ref.py).

A table is [B*V, V]: row b*V + c holds batch row b's logits after token c; the step terms lp come from beam_ref.step_terms (in
fp32 the kernel's two roundings).  viterbi works in lp's dtype, one rounding per addition: in fp32 it performs the kernel's
operations, in fp64 the same formulas serve as an oracle.  brute_force enumerates every admissible sequence."""
from __future__ import annotations

import itertools

import numpy as np


def viterbi(lp: np.ndarray, B: int, V: int, max_len: int, min_len: int = 0, end_token: int = 2, pad_token: int = 0):
    """-> tokens [B, max_len] int32, scores [B] (lp's dtype), lengths [B] int32.  a_t[v] = max over u != end of fl(a_{t-1}[u] +
    lp(u, v)), back pointer = the lowest u attaining it; candidates e_{min_len} .. e_{max_len-1}, then a_{max_len-1}[v] for
    v != end ascending: the first is taken, a later one replaces it only when strictly greater."""
    dt = lp.dtype.type
    tokens = np.full((B, max_len), pad_token, dtype=np.int32)
    scores = np.full(B, -np.inf, dtype=lp.dtype)
    lengths = np.full(B, max_len, dtype=np.int32)
    for b in range(B):
        M = lp[b * V:(b + 1) * V]
        bp = np.zeros((max_len, V), dtype=np.int64)
        a = (dt(0) + M[0]).astype(lp.dtype)
        chosen, best, n, last = False, dt(-np.inf), max_len, 0
        for t in range(max_len):
            if t > 0:
                with np.errstate(invalid="ignore"):
                    cand = (a[:, None] + M).astype(lp.dtype)          # [u, v], one rounding per candidate; a[end] = -inf
                bp[t] = cand.argmax(axis=0)                            # the first (lowest) u of the maximum
                a = cand[bp[t], np.arange(V)]
            e = a[end_token]
            if t >= min_len and (not chosen or e > best):
                chosen, best, n, last = True, e, t + 1, end_token
            a = a.copy()
            a[end_token] = -np.inf                                     # the end token never continues
        for v in range(V):
            if v != end_token and (not chosen or a[v] > best):
                chosen, best, n, last = True, a[v], max_len, v
        scores[b], lengths[b] = best, n
        tok = last
        tokens[b, n - 1] = tok
        for t in range(n - 1, 0, -1):
            tok = int(bp[t, tok])
            tokens[b, t - 1] = tok
    return tokens, scores, lengths


def brute_force(lp: np.ndarray, b: int, V: int, max_len: int, min_len: int, end_token: int):
    """The maximum of the contract score over all admissible sequences of batch row b, by enumeration, in lp's dtype."""
    dt = lp.dtype.type
    M = lp[b * V:(b + 1) * V]
    others = [v for v in range(V) if v != end_token]
    best = dt(-np.inf)

    def score(seq):
        s, c = dt(0), 0
        for x in seq:
            s = dt(s + M[c, x])
            c = x
        return s

    for n in range(1, max_len + 1):
        for body in itertools.product(others, repeat=n - 1):
            if n - 1 >= min_len:
                best = max(best, score(body + (end_token,)))
            if n == max_len:
                for v in others:
                    best = max(best, score(body + (v,)))
    return best


def marginals(lp: np.ndarray, B: int, V: int, max_len: int, end_token: int = 2, dtype=np.float64) -> np.ndarray:
    """alive [B, max_len, V] in `dtype`: alive[b, 0, v] = p(0, v), alive[b, t, v] = sum over u != end of alive[b, t-1, u] p(u, v),
    p = exp(lp) evaluated in `dtype` (the sums sequential in u for fp32 -- the kernel's order is its own)."""
    P = np.exp(lp.astype(dtype)).astype(dtype).reshape(B, V, V)
    out = np.zeros((B, max_len, V), dtype=dtype)
    for b in range(B):
        a = P[b, 0].copy()
        out[b, 0] = a
        for t in range(1, max_len):
            a = a.copy()
            a[end_token] = 0
            if dtype == np.float64:
                a = a @ P[b]
            else:
                acc = np.zeros(V, dtype=dtype)
                for u in range(V):
                    acc = (acc + (a[u] * P[b, u]).astype(dtype)).astype(dtype)
                a = acc
            out[b, t] = a
    return out


def length_distribution(alive: np.ndarray, end_token: int = 2) -> np.ndarray:
    """[B, max_len + 1]: entry t < max_len = P(length = t+1), the last = P(no end within max_len)."""
    rest = np.delete(alive[:, -1, :], end_token, axis=1).sum(axis=1)
    return np.concatenate([alive[:, :, end_token], rest[:, None]], axis=1)


def make_table(rs, B: int, V: int, kind: str, end_token: int = 2, lower: float = 4.0) -> np.ndarray:
    """The tables of tests/test_beam_gpu.py: "normal" = 2 * N(0, 1) with the end column raised by 0.5 (the optimum ends after a
    few tokens), "q8" = the same rounded to multiples of 1/8 (exact ties everywhere); "-lowered-end" lowers the end column by
    `lower` instead.  A step of these tables costs about 1.5 to 2 nats at its best, so an optimum that runs to max_len without
    ending needs lower >= 4 * max_len (ending must cost more than all the steps it saves); lower = 4 still ends early."""
    table = rs.standard_normal((B * V, V)).astype(np.float32) * 2.0
    if kind.endswith("-lowered-end"):
        table[:, end_token] -= np.float32(lower)
    else:
        table[:, end_token] += 0.5
    if kind.startswith("q8"):
        table = np.round(table * 8) / 8
    return table.astype(np.float32)
