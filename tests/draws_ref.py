"""NumPy restatement of N independent draws per batch row over a dense decoder table (the contract of include/arcvae_hip.h
arcvae_dec_sample_draws; test infrastructure, built on tests/topkp_ref.py).

The lists are those of arcvae_dec_sample_chain_trunc (tests/trunc_ref.py); what is new is the key of draw d of batch row b and the
pad mode.  The walk is replayed from materialised rows -- the kernels' own -- with the generator in Python ints: bit-exact."""
from __future__ import annotations

import numpy as np

import topkp_ref as T

DRAW_MUL = 0xD1B54A32D192ED03


def row_key(seed: int, b: int) -> int:
    """The common contract's key of batch row b: mix64(seed ^ (b << 32))."""
    return T.mix64((seed & T.M64) ^ ((b << 32) & T.M64))


def draw_key(seed: int, b: int, d: int) -> int:
    """key(b, 0) = the row key; key(b, d) = mix64(row key ^ (0xD1B54A32D192ED03 * d)) in 64-bit wrapping arithmetic."""
    k = row_key(seed, b)
    return k if d == 0 else T.mix64(k ^ ((DRAW_MUL * d) & T.M64))


def u24(key: int, t: int) -> int:
    """The 24 uniform bits of step t of the draw with this key: mix64(key + t) >> 40."""
    return T.mix64((key + t) & T.M64) >> 40


def walk(materialised_plain, materialised_banned, B: int, N: int, V: int, max_len: int, min_len: int, seed: int,
         end_token: int = 2, pad_token: int = -1):
    """Replay arcvae_dec_sample_draws from materialised table rows: materialised_*(r) -> (count, tokens [V], cum [V]) of table row
    r, the banned ones (built with ban_token = end_token) read by the steps t < min_len.  -> tokens [B, N, max_len] int32,
    first_end [B, N] int32.  pad_token >= 0: the positions after the first end hold it and the draw stops."""
    tokens = np.zeros((B, N, max_len), dtype=np.int32)
    first_end = np.full((B, N), max_len, dtype=np.int32)
    for b in range(B):
        for d in range(N):
            key, cur = draw_key(seed, b, d), 0
            for t in range(max_len):
                n, tok, cum = (materialised_banned if t < min_len else materialised_plain)(b * V + cur)
                cur = min(int(tok[T.pick(int(n), cum, u24(key, t))]), V - 1)
                tokens[b, d, t] = cur
                if cur == end_token and first_end[b, d] == max_len:
                    first_end[b, d] = t
                    if pad_token >= 0:
                        tokens[b, d, t + 1:] = pad_token
                        break
    return tokens, first_end
