"""NumPy restatement of min-p, locally typical and minimum-length truncated sampling over a dense decoder table (the contract of
include/arcvae_hip.h arcvae_dec_trunc_rows / arcvae_dec_sample_chain_trunc; test infrastructure, built on tests/topkp_ref.py).

The scaled logits s are fp32 and exact (topkp_ref.scaled), so the s-order and the top-k set are exact; the masses, the entropy,
the deviations d = |log p + H| and every test against a threshold are restated in fp64, the oracle the kernels' fp32 arithmetic
is held to.  The walk is replayed from materialised rows -- the kernels' own -- so the replay is bit-exact."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import topkp_ref as T


def set_size(V: int, top_k, ban: int = -1) -> int:
    """|K| = min(top_k or V, V - 1 with a banned token)."""
    return min(T.set_size(V, top_k), V - 1 if ban >= 0 else V)


def order(s_row: np.ndarray, ban: int = -1) -> np.ndarray:
    """The s-order (topkp_ref.order) with the banned token moved behind every other one."""
    o = T.order(s_row)
    return o if ban < 0 else np.concatenate([o[o != ban], [ban]])


def truncate(s_row: np.ndarray, top_k=0, top_p: float = 1.0, min_p: float = 0.0, typical_p: float = 1.0, ban: int = -1):
    """fp64 restatement of one row.  top_p, min_p and typical_p are rounded to fp32 first, as the kernel receives them.  Fields:
    s_order = the s-order (banned token last), K = |K|, tokens = the row's whole order (the typical order over K, then the rest of
    the s-order, in the typical family; the s-order otherwise), e / C / before = the masses exp(s - max s) in THAT order, their
    inclusive prefix sums and C - e, n = the count, thr = the prefix threshold (top_p * M_K or typical_p * M_K), min_p; and in the
    typical family H = -sum p log p over K, d = |log p + H| in `tokens` order, a = s - s_0 in that order, logM, abs_l = sum p |l|."""
    so = order(s_row, ban)
    K = set_size(len(so), top_k, ban)
    s = np.asarray(s_row, dtype=np.float64)[so[:K]]
    a = s - s[0]
    e = np.exp(a)
    M = e.sum()
    p, mp, tp = float(np.float32(top_p)), float(np.float32(min_p)), float(np.float32(typical_p))
    if tp >= 1.0:
        C = np.cumsum(e)
        before = C - e
        thr = p * C[-1]
        keep = (e > 0 if p >= 1.0 else before < thr) & (e >= mp)
        keep[0] = True
        fail = np.flatnonzero(~keep)
        return SimpleNamespace(typical=False, s_order=so, K=K, tokens=so, e=e, C=C, before=before, thr=thr, min_p=mp,
                               n=int(fail[0]) if fail.size else K)
    assert p >= 1.0 and mp == 0.0, "typical_p < 1 takes no top_p and no min_p"
    logM = np.log(M)
    l = a - logM
    H = -(e * l).sum() / M
    d = np.abs(l + H)
    perm = np.lexsort((np.arange(K), d))                                 # d ascending, then the s-position ascending
    e2 = e[perm]
    C = np.cumsum(e2)
    before = C - e2
    thr = tp * C[-1]
    keep = before < thr
    keep[0] = True
    fail = np.flatnonzero(~keep)
    return SimpleNamespace(typical=True, s_order=so, K=K, tokens=np.concatenate([so[:K][perm], so[K:]]), e=e2, C=C, before=before,
                           thr=thr, min_p=0.0, n=int(fail[0]) if fail.size else K, H=H, d=d[perm], a=a[perm], logM=logM,
                           abs_l=float((e * np.abs(l)).sum() / M))


def dev_bound(r) -> np.ndarray:
    """The worst case of |d_fp32 - d_fp64| per position of K (typical family): (|K| + 16) * 2^-23 * (1 + |s_i - s_0| + |log M_K| +
    sum p |l|), a bound over the operation count of the contract (|K| roundings of the sums, a few of exp, log and the rest)."""
    return (r.K + 16) * 2.0 ** -23 * (1.0 + np.abs(r.a) + abs(r.logM) + r.abs_l)


def ent_bound(r) -> float:
    """dev_bound without the s term: the worst case of |H_fp32 - H_fp64|."""
    return (r.K + 16) * 2.0 ** -23 * (1.0 + abs(r.logM) + r.abs_l)


def is_min_p_boundary(r, at: int, rel: float = 1e-5) -> bool:
    """fp32 rounding of e may decide position `at` (the cut: the first position where two counts differ) either way:
    |e_at - min_p| <= rel * min_p."""
    return bool(0 < at < r.K and abs(r.e[at] - r.min_p) <= rel * r.min_p)


def is_typical_boundary(r, rel: float = 1e-5) -> bool:
    """The prefix mass of some position lies within `rel` (relative) of the threshold, or the fp64 gap in d between the last
    kept and the first dropped position is below twice their bound: fp32 rounding may order them either way."""
    if np.any(np.abs(r.before[1:] - r.thr) <= rel * r.thr):
        return True
    if 0 < r.n < r.K:
        b = dev_bound(r)
        return bool(r.d[r.n] - r.d[r.n - 1] < 2 * max(b[r.n], b[r.n - 1]))
    return False


def truncated_probs(logits: np.ndarray, temperature: float, top_k=0, top_p: float = 1.0, min_p: float = 0.0,
                    typical_p: float = 1.0, ban: int = -1) -> np.ndarray:
    """fp64 truncated, renormalised softmax(logits / T) over the vocabulary (the distribution a step of the walk draws from)."""
    s = np.asarray(logits, dtype=np.float64) / float(temperature)
    r = truncate(s, top_k, top_p, min_p, typical_p, ban)
    out = np.zeros(len(s))
    out[r.tokens[:r.n]] = r.e[:r.n] / r.e[:r.n].sum()
    return out


def walk(materialised_plain, materialised_banned, B: int, V: int, max_len: int, min_len: int, seed: int, end_token: int = 2):
    """Replay arcvae_dec_sample_chain_trunc from materialised table rows: materialised_*(r) -> (count, tokens [V], cum [V]) of
    table row r, the banned ones (built with ban_token = end_token) read by the steps t < min_len.  -> tokens [B, max_len] int32,
    first_end [B] int32.  With min_len = 0 it is topkp_ref.walk."""
    tokens = np.zeros((B, max_len), dtype=np.int32)
    first_end = np.full(B, max_len, dtype=np.int32)
    for b in range(B):
        cur = 0
        for t in range(max_len):
            n, tok, cum = (materialised_banned if t < min_len else materialised_plain)(b * V + cur)
            cur = int(tok[T.pick(int(n), cum, T.u24(seed, b, t))])
            tokens[b, t] = cur
            if cur == end_token and first_end[b] == max_len:
                first_end[b] = t
    return tokens, first_end
