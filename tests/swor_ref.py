"""NumPy restatement of sampling WITHOUT replacement over a dense decoder table: stochastic beam search (Kool, van Hoof and
Welling, ICML 2019), the contract of include/arcvae_hip.h arcvae_dec_swor (test infrastructure, like oracle/).

A table is [B*V, V]: row b*V + c holds the logits of batch row b after token c.  `dtype` switches the arithmetic: float64 is the
reference the kernel's perturbed values are held to, float32 performs the kernel's operations in the kernel's precision and
gives the rounding error to expect of it.  Both are written in the cancellation-free form: the children of one parent are
compared through a = lp + g (the parent's phi is common to them and drops out), and every slot carries r = G - phi next to G, so
no step subtracts two numbers of size |phi|.  The noise is the splitmix64 generator in integer (uint64) arithmetic, keyed by
(seed, batch row, token prefix), so both precisions see the same uniform bits.

brute_force() evaluates the same definition over the WHOLE tree of a small chain with the contract's formula as written (no
beam, no rearrangement): the perturbed value of every complete sequence, which a K-wide walk must return the K largest of."""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
LN2 = math.log(2.0)


def mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser (csrc/common.h mix64) on a uint64 array (integer arithmetic, wrapping)."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def mix64_int(x: int) -> int:
    """The same finaliser on a Python int (brute_force)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def root_hash(seed: int, B: int) -> np.ndarray:
    """h_root[b] = mix64(seed ^ (b << 32))."""
    b = np.arange(B, dtype=np.uint64)
    return mix64(np.uint64(seed & M64) ^ (b << np.uint64(32)))


def gumbel(h: np.ndarray, dtype) -> np.ndarray:
    """g = -log(-log(u)), u = ((h >> 40) + 0.5) * 2^-24.  n + 0.5 is not an fp32 number for n >= 2^23, so -log(u) is taken there
    as -log1p(-(2^24 - n - 0.5) * 2^-24), whose argument is one: every u in (0, 1) keeps its own finite g in both precisions."""
    n = (h >> np.uint64(40)).astype(np.int64)
    hi = n >= (1 << 23)
    scale = dtype(2.0 ** -24)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo_e = -np.log((np.where(hi, 0, n).astype(dtype) + dtype(0.5)) * scale)
        hi_e = -np.log1p(-((np.where(hi, (1 << 24) - n, 1).astype(dtype) - dtype(0.5)) * scale))
        return (-np.log(np.where(hi, hi_e, lo_e))).astype(dtype)


def step_terms(table: np.ndarray, lse: np.ndarray, temperature: float, dtype) -> np.ndarray:
    """lp[r, v] = x[r, v] * (1 / T) - lse[r] in `dtype` (float32: csrc/beam.hip's step term bit for bit)."""
    inv = dtype(1.0) / dtype(temperature)
    return ((np.asarray(table).astype(dtype) * inv).astype(dtype) - np.asarray(lse).astype(dtype)[:, None]).astype(dtype)


def swor(table, lse, B: int, V: int, K: int, max_len: int, seed: int, end_token: int = 2, pad_token: int = 0,
         temperature: float = 1.0, dtype=np.float64):
    """-> dict(tokens [B, K, max_len] int32, log_probs [B, K], perturbed [B, K], lengths [B, K] int32, threshold [B],
    gap [B]): the outputs of arcvae_dec_swor in `dtype`, and per row the smallest boundary gap over the steps, (K-th kept G) -
    (best rejected G) (+inf for a row that never rejected anything).  Vectorised over the batch; rows whose slots are all
    finished keep copying themselves, which is what the kernel's early end leaves behind."""
    lp_all = step_terms(table, lse, temperature, dtype).reshape(B, V, V)
    ninf = dtype(-np.inf)
    phi = np.full((B, K), ninf, dtype)
    G = np.full((B, K), ninf, dtype)
    r = np.zeros((B, K), dtype)
    phi[:, 0] = G[:, 0] = 0
    h = np.zeros((B, K), np.uint64)
    h[:, 0] = root_hash(seed, B)
    last = np.zeros((B, K), np.int64)                           # the start token
    fin = np.zeros((B, K), bool)
    live = np.zeros((B, K), bool)
    live[:, 0] = True
    toks = np.full((B, K, max_len), pad_token, np.int32)
    threshold = np.full(B, ninf, dtype)
    gap = np.full(B, np.inf)
    rows = np.arange(B)[:, None]
    tok_ids = np.arange(V, dtype=np.uint64)
    for t in range(max_len):
        lp = lp_all[rows, last]                                 # [B, K, V]
        hc = mix64(h[:, :, None] + tok_ids + np.uint64(1))
        g = gumbel(hc, dtype)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = (lp + g).astype(dtype)
            d = a - a.max(axis=2, keepdims=True)                # Gp_c - Z, from the small quantities
            lg = np.where(d > -LN2, np.log(-np.expm1(d)), np.log1p(-np.exp(d)))
            v = (r[:, :, None] - a) + lg                        # G_S - Gp_c + log1p(-exp(Gp_c - Z))
            hi, lo = np.maximum(v, 0), np.log1p(np.exp(-np.abs(v)))
            cG = ((G[:, :, None] - hi) - lo).astype(dtype)
            cr = (((r[:, :, None] - lp) - hi) - lo).astype(dtype)
            cphi = (phi[:, :, None] + lp).astype(dtype)
        ok = np.broadcast_to((live & ~fin)[:, :, None], (B, K, V)).copy()
        is_pad = np.broadcast_to(np.arange(V) == pad_token, (B, K, V))
        done = (live & fin)[:, :, None] & is_pad                # a finished parent: one continuation, pad, unchanged
        cG = np.where(done, G[:, :, None], cG)
        cr = np.where(done, r[:, :, None], cr)
        cphi = np.where(done, phi[:, :, None], cphi)
        hc = np.where(done, h[:, :, None], hc)
        ok |= done
        key = np.where(ok, cG, ninf).reshape(B, K * V)
        order = np.argsort(-key, axis=1, kind="stable")[:, :K + 1]     # (G desc, parent slot asc, token asc)
        n_ok = ok.reshape(B, K * V).sum(1)
        sel = order[:, :K]
        filled = np.arange(K)[None, :] < n_ok[:, None]
        if order.shape[1] > K:
            rej = np.take_along_axis(key, order[:, K:K + 1], 1)[:, 0]
            has = n_ok > K
            threshold = np.where(has, np.maximum(threshold, rej), threshold)
            kth = np.take_along_axis(key, order[:, K - 1:K], 1)[:, 0]
            with np.errstate(invalid="ignore"):                 # (rows without a rejected candidate: -inf - -inf, not used)
                gap = np.where(has, np.minimum(gap, (kth - rej).astype(np.float64)), gap)
        par, tok = sel // V, sel % V
        take = lambda x: np.take_along_axis(x.reshape(B, K * V), sel, 1)     # noqa: E731
        nfin = np.take_along_axis(fin, par, 1) | (tok == end_token)
        toks = np.take_along_axis(toks, par[:, :, None], 1)
        toks[:, :, t] = np.where(filled, tok, pad_token)
        phi = np.where(filled, take(cphi), ninf).astype(dtype)
        G = np.where(filled, take(cG), ninf).astype(dtype)
        r = np.where(filled, take(cr), 0).astype(dtype)
        h = np.where(filled, take(hc), np.uint64(0))
        last, fin, live = np.where(filled, tok, 0), nfin & filled, filled
        toks[~filled] = pad_token
    ends = toks == end_token
    lengths = np.where(ends.any(2), ends.argmax(2) + 1, max_len)
    lengths = np.where(live, lengths, 0).astype(np.int32)
    return dict(tokens=toks, log_probs=phi, perturbed=G, lengths=lengths, threshold=threshold, gap=gap)


def brute_force(lp: np.ndarray, V: int, max_len: int, seed: int, b: int = 0, end_token: int = 2, pad_token: int = 0):
    """Every complete sequence of batch row b's chain with its log-probability and its perturbed value, by top-down Gumbel
    sampling over the WHOLE tree in Python floats, the contract's conditioning formula as written:
    G_c = -log(exp(-G_S) - exp(-Z) + exp(-Gp_c)).  lp: [V, V] fp64 step terms of the row (lp[c, v]).
    -> list of (tokens tuple of max_len, phi, G), G descending."""
    out = []

    def g_of(hh):
        return -math.log(-math.log(((hh >> 40) + 0.5) * 2.0 ** -24))

    def visit(prefix, phi, G, hh):
        if len(prefix) == max_len or (prefix and prefix[-1] == end_token):
            out.append((tuple(prefix) + (pad_token,) * (max_len - len(prefix)), phi, G))
            return
        c = prefix[-1] if prefix else 0
        hs = [mix64_int((hh + v + 1) & M64) for v in range(V)]
        Gp = [phi + lp[c, v] + g_of(hs[v]) for v in range(V)]
        Z = max(Gp)
        for v in range(V):
            Gc = G if Gp[v] == Z else -math.log(math.exp(-G) - math.exp(-Z) + math.exp(-Gp[v]))
            visit(prefix + [v], phi + lp[c, v], Gc, hs[v])

    visit([], 0.0, 0.0, mix64_int((seed & M64) ^ ((b << 32) & M64)))
    return sorted(out, key=lambda s: -s[2])


def sequence_probs(lp: np.ndarray, V: int, max_len: int, end_token: int = 2, pad_token: int = 0):
    """{tokens tuple: probability} of every complete sequence of one row's chain (lp [V, V] fp64)."""
    return {s: math.exp(phi) for s, phi, _ in brute_force(lp, V, max_len, 0, 0, end_token, pad_token)}
