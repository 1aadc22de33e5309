"""NumPy restatement of beam search and sequence log-likelihood over a dense decoder table (the contract of
include/arcvae_hip.h arcvae_dec_beam_search / arcvae_dec_sequence_logprob; test infrastructure, like oracle/).

A table is [B*V, V]: row b*V + c holds the logits of batch row b after token c.  In fp32 every operation is the kernel's,
one IEEE operation at a time: lp = fl(fl(x * fl(1 / T)) - lse), score = fl(s + lp).  In fp64 the same formulas serve as an
oracle.  The search here merges all K x V candidates of a step (no pre-pass), in the contract's total order:
score descending, then parent slot ascending, then token ascending."""
from __future__ import annotations

import numpy as np


def row_lse(table: np.ndarray, temperature: float) -> np.ndarray:
    """logsumexp(x / T) of every row in fp64 (the kernel's fp32 lse is checked against it)."""
    x = np.asarray(table, dtype=np.float64) / float(temperature)
    m = x.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(x - m).sum(axis=1))


def step_terms(table: np.ndarray, lse: np.ndarray, temperature: float, dtype=np.float32) -> np.ndarray:
    """lp[r, v] = x[r, v] * inv_temp - lse[r]: fp32 = the kernel's two roundings (inv_temp = 1.0f / T), fp64 = plain."""
    if dtype == np.float32:
        inv = np.float32(1.0) / np.float32(temperature)
        a = np.asarray(table, dtype=np.float32) * inv
        return (a - np.asarray(lse, dtype=np.float32)[:, None]).astype(np.float32)
    return np.asarray(table, dtype=np.float64) / float(temperature) - np.asarray(lse, dtype=np.float64)[:, None]


def beam_search(lp: np.ndarray, B: int, V: int, K: int, max_len: int, min_len: int = 0, end_token: int = 2,
                pad_token: int = 0):
    """-> tokens [B, K, max_len] int32, scores [B, K] (lp's dtype), lengths [B, K] int32."""
    dt = lp.dtype.type
    tokens = np.full((B, K, max_len), pad_token, dtype=np.int32)
    scores = np.full((B, K), -np.inf, dtype=lp.dtype)
    lengths = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        sc = np.full(K, -np.inf, dtype=lp.dtype)
        sc[0] = dt(0)
        last = np.zeros(K, dtype=np.int64)
        fin = np.zeros(K, dtype=bool)
        hist = np.full((K, max_len), pad_token, dtype=np.int32)
        for t in range(max_len):
            c_sc, c_par, c_tok = [], [], []
            for k in range(K):
                if not sc[k] > -np.inf:
                    continue
                if fin[k]:                               # EOS is absorbing: pad continuation, same score
                    c_sc.append(np.array([sc[k]], dtype=lp.dtype))
                    c_par.append(np.array([k]))
                    c_tok.append(np.array([pad_token]))
                    continue
                s = (sc[k] + lp[b * V + last[k]]).astype(lp.dtype)      # one rounding per candidate
                v = np.arange(V)
                if t < min_len:
                    keep = v != end_token
                    s, v = s[keep], v[keep]
                c_sc.append(s)
                c_par.append(np.full(len(v), k))
                c_tok.append(v)
            s = np.concatenate(c_sc)
            par = np.concatenate(c_par)
            tok = np.concatenate(c_tok)
            ok = s > -np.inf
            s, par, tok = s[ok], par[ok], tok[ok]
            order = np.lexsort((tok, par, -s))[:K]
            n = len(order)
            new_hist = np.full((K, max_len), pad_token, dtype=np.int32)
            new_hist[:n] = hist[par[order]]
            new_hist[:n, t] = tok[order]
            new_fin = np.zeros(K, dtype=bool)
            new_fin[:n] = fin[par[order]] | (tok[order] == end_token)
            new_sc = np.full(K, -np.inf, dtype=lp.dtype)
            new_sc[:n] = s[order]
            new_last = np.zeros(K, dtype=np.int64)
            new_last[:n] = tok[order]
            sc, last, fin, hist = new_sc, new_last, new_fin, new_hist
            if not np.any((sc > -np.inf) & ~fin):        # all finished: later steps only append pad tokens
                break
        tokens[b] = hist
        scores[b] = sc
        for k in range(K):
            if sc[k] > -np.inf:
                e = np.flatnonzero(hist[k] == end_token)
                lengths[b, k] = e[0] + 1 if e.size else max_len
    return tokens, scores, lengths


def sequence_logprob(lp: np.ndarray, tokens: np.ndarray, V: int, end_token: int = 2, batch=None) -> np.ndarray:
    """sum_{t<=e} lp[b*V + fed_t, x_t] accumulated left to right in lp's dtype; fed_0 = 0, fed_t = x_{t-1}, e = first EOS.
    batch[i] = the table's batch row b of sequence i (default: i)."""
    dt = lp.dtype.type
    N, T = tokens.shape
    batch = np.arange(N) if batch is None else np.asarray(batch)
    out = np.zeros(N, dtype=lp.dtype)
    for n in range(N):
        b = int(batch[n])
        s, c = dt(0), 0
        for t in range(T):
            x = int(tokens[n, t])
            s = dt(s + lp[b * V + c, x])
            if x == end_token:
                break
            c = x
        out[n] = s
    return out
