"""NumPy restatement of top-k / nucleus (top-p) truncated sampling over a dense decoder table (the contract of
include/arcvae_hip.h arcvae_dec_topkp_rows / arcvae_dec_sample_chain_topkp; test infrastructure, like oracle/).

A table is [B*V, V]: row b*V + c holds the logits of batch row b after token c.  The scaled logits s = fl(x * fl(1 / T)) are one
IEEE fp32 multiply, reproduced here bit for bit, so the order and the top-k set are exact.  The masses and the nucleus test are
restated in fp64 (the oracle the kernels' fp32 prefix sums are held to).  The walk is replayed from materialised rows (count,
tokens, cum) -- the kernels' own -- with the splitmix64 generator in Python ints, so the replay is bit-exact."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """splitmix64 finaliser (csrc/common.h mix64), 64-bit arithmetic by masking."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def u24(seed: int, b: int, t: int) -> int:
    """The 24 uniform bits of batch row b at step t: mix64(mix64(seed ^ (b << 32)) + t) >> 40."""
    return mix64((mix64((seed & M64) ^ ((b << 32) & M64)) + t) & M64) >> 40


def scaled(rows: np.ndarray, temperature: float) -> np.ndarray:
    """s = fl(x * fl(1.0f / T)) in fp32, as the kernels."""
    inv = np.float32(1.0) / np.float32(temperature)
    return (np.asarray(rows, dtype=np.float32) * inv).astype(np.float32)


def order(s_row: np.ndarray) -> np.ndarray:
    """Tokens by s descending, ties to the lower token index (-0 and +0 compare equal, as in IEEE)."""
    s64 = np.asarray(s_row, dtype=np.float64)
    return np.lexsort((np.arange(len(s64)), -s64))


def set_size(V: int, top_k) -> int:
    return V if not top_k else min(int(top_k), V)


def truncate(s_row: np.ndarray, top_k=0, top_p: float = 1.0):
    """fp64 restatement of one row -> (order, |K|, e [|K|], C [|K|], n, before [|K|], thr): e = exp(s - max s) over the order,
    C = inclusive prefix sums, before = C - e (the mass strictly before each position), thr = p * M_K with p rounded to fp32
    as the kernel receives it; n = the first position >= 1 failing before < thr (|K| if none); top_p = 1 keeps e > 0."""
    o = order(s_row)
    K = set_size(len(o), top_k)
    s = np.asarray(s_row, dtype=np.float64)[o[:K]]
    e = np.exp(s - s[0])
    C = np.cumsum(e)
    before = C - e
    p = float(np.float32(top_p))
    thr = p * C[-1]
    keep = e > 0 if p >= 1.0 else before < thr
    keep[0] = True
    fail = np.flatnonzero(~keep)
    n = int(fail[0]) if fail.size else K
    return o, K, e, C, n, before, thr


def brute_force_sets(s_row: np.ndarray, top_k=0, top_p: float = 1.0):
    """(K, P) as token sets by direct enumeration: i is in K iff fewer than k tokens precede it; i in K is in P iff the fp64
    mass of the tokens of K preceding it is below p * M_K (p = 1: iff its mass is positive)."""
    s = np.asarray(s_row, dtype=np.float64)
    V = len(s)
    k = set_size(V, top_k)
    prec = lambda i: [j for j in range(V) if s[j] > s[i] or (s[j] == s[i] and j < i)]   # noqa: E731
    Kset = {i for i in range(V) if len(prec(i)) < k}
    mx = s.max()
    e = {i: np.exp(s[i] - mx) for i in Kset}
    MK = sum(sorted(e.values()))
    p = float(np.float32(top_p))
    if p >= 1.0:
        P = {i for i in Kset if e[i] > 0 or len(prec(i)) == 0}
    else:
        P = {i for i in Kset if len(prec(i)) == 0 or sum(sorted(e[j] for j in prec(i) if j in Kset)) < p * MK}
    return Kset, P


def is_boundary(before: np.ndarray, thr: float, rel: float = 1e-5) -> bool:
    """A row whose fp64 prefix mass lies within `rel` (relative) of the threshold at some position: fp32 rounding may decide its
    nucleus count either way."""
    return bool(np.any(np.abs(before[1:] - thr) <= rel * thr))


def pick(count: int, cum_row: np.ndarray, u: int) -> int:
    """The walk's decision on a materialised row: theta = fl(fl(u24 * 2^-24) * C_{n-1}); the first position i < n with
    C_i > theta, n - 1 if none."""
    c = np.asarray(cum_row[:count], dtype=np.float32)
    theta = np.float32(np.float32(u) * np.float32(2.0 ** -24)) * c[count - 1]
    over = np.flatnonzero(c > theta)
    return int(over[0]) if over.size else count - 1


def walk(materialised, B: int, V: int, max_len: int, seed: int, end_token: int = 2):
    """Replay arcvae_dec_sample_chain_topkp from materialised table rows: materialised(r) -> (count, tokens [V], cum [V]) of
    table row r.  -> tokens [B, max_len] int32, first_end [B] int32."""
    tokens = np.zeros((B, max_len), dtype=np.int32)
    first_end = np.full(B, max_len, dtype=np.int32)
    for b in range(B):
        cur = 0
        for t in range(max_len):
            n, tok, cum = materialised(b * V + cur)
            cur = int(tok[pick(int(n), cum, u24(seed, b, t))])
            tokens[b, t] = cur
            if cur == end_token and first_end[b] == max_len:
                first_end[b] = t
    return tokens, first_end


def truncated_probs(logits: np.ndarray, temperature: float, top_k=0, top_p: float = 1.0) -> np.ndarray:
    """fp64 truncated, renormalised softmax(logits / T) over the vocabulary (the distribution the walk draws from)."""
    s = np.asarray(logits, dtype=np.float64) / float(temperature)
    o, K, e, C, n, _, _ = truncate(s, top_k, top_p)
    out = np.zeros(len(s))
    out[o[:n]] = e[:n] / e[:n].sum()
    return out
