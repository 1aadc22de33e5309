"""NumPy restatement of the exact expectations over a dense decoder table's outcomes (the contract of include/arcvae_hip.h
arcvae_dec_row_costs / arcvae_dec_chain_expect; test infrastructure, like chain_ref.py): entropy, cross-entropy, expected token
counts and the mass a max_len cuts off, in fp64 on top of chain_ref.marginals, and the same quantities by enumeration of every
outcome for tiny V.

Step terms lp come from beam_ref.step_terms: [B*V, V], row b*V + c = batch row b after token c.  Whatever their dtype the
arithmetic here is fp64: over fp32 step terms only expf, the products and the sums differ from the kernels'."""
from __future__ import annotations

import itertools

import numpy as np

import chain_ref


def row_costs(lp_p: np.ndarray, lp_q: np.ndarray):
    """-> (r, a), each [rows]: r = -sum_v p lq with p = exp(lp_p), a = the same sum with every term in absolute value.  A term
    whose p is 0 contributes 0, also where lq is -inf."""
    lp_p, lp_q = np.asarray(lp_p, dtype=np.float64), np.asarray(lp_q, dtype=np.float64)
    p = np.exp(lp_p)
    with np.errstate(invalid="ignore"):
        term = np.where(p > 0, p * lp_q, 0.0)
    return -term.sum(axis=1), np.abs(term).sum(axis=1)


def expectations(lp_p: np.ndarray, lp_q: np.ndarray, B: int, V: int, max_len: int, end_token: int = 2) -> dict:
    """fp64: H [B] the entropy of row b's outcome distribution, CE [B] the cross-entropy -E_P[log Q] (lp_q = lp_p: CE = H),
    A_H / A_CE the same sums with every term in absolute value (the magnitude a rounding bound scales with), visits [B, V],
    open_mass [B] and cont [B, V].  total_r = r[b, 0] + sum over v != end of r[b, v] * cont[b, v]."""
    alive = chain_ref.marginals(np.asarray(lp_p), B, V, max_len, end_token, np.float64)
    visits = alive.sum(axis=1)
    open_mass = np.delete(alive[:, -1, :], end_token, axis=1).sum(axis=1)
    cont = alive[:, :max_len - 1, :].sum(axis=1)
    cont[:, end_token] = 0.0
    out = dict(visits=visits, open_mass=open_mass, cont=cont)
    for name, lq in (("H", lp_p), ("CE", lp_q)):
        r, a = row_costs(lp_p, lq)
        r, a = r.reshape(B, V), a.reshape(B, V)
        with np.errstate(invalid="ignore"):
            out[name] = r[:, 0] + np.where(cont > 0, r * cont, 0.0).sum(axis=1)
            out["A_" + name] = a[:, 0] + np.where(cont > 0, a * cont, 0.0).sum(axis=1)
    return out


def outcomes(V: int, max_len: int, end_token: int):
    """Every outcome at max_len: the sequences that end with their first end_token at length n <= max_len, then the max_len
    tokens without one.  -> an iterator of (tokens, ended)."""
    others = [v for v in range(V) if v != end_token]
    for n in range(1, max_len + 1):
        for body in itertools.product(others, repeat=n - 1):
            yield body + (end_token,), True
            if n == max_len:
                for v in others:
                    yield body + (v,), False


def enumerate_outcomes(lp_p: np.ndarray, lp_q: np.ndarray, B: int, V: int, max_len: int, end_token: int = 2) -> dict:
    """The same quantities by enumeration, fp64: mass [B] (1 up to the rows' normalisation), H, CE, length [B] = the expected
    number of tokens, visits [B, V], open_mass [B]."""
    lp_p, lp_q = np.asarray(lp_p, dtype=np.float64), np.asarray(lp_q, dtype=np.float64)
    out = dict(mass=np.zeros(B), H=np.zeros(B), CE=np.zeros(B), length=np.zeros(B), visits=np.zeros((B, V)),
               open_mass=np.zeros(B))
    for b in range(B):
        Mp, Mq = lp_p[b * V:(b + 1) * V], lp_q[b * V:(b + 1) * V]
        for seq, ended in outcomes(V, max_len, end_token):
            logp = logq = 0.0
            c = 0
            for x in seq:
                logp += Mp[c, x]
                logq += Mq[c, x]
                c = x
            pr = np.exp(logp)
            if pr == 0.0:
                continue
            out["mass"][b] += pr
            out["H"][b] -= pr * logp
            out["CE"][b] -= pr * logq
            out["length"][b] += pr * len(seq)
            for x in seq:
                out["visits"][b, x] += pr
            if not ended:
                out["open_mass"][b] += pr
    return out
