"""Sampling without replacement, the parts that need no GPU: the NumPy restatement (tests/swor_ref.py) against a brute-force
evaluation of the contract over the whole tree of a 7-sequence chain, its statistics against Plackett-Luce, and the two entry
points declared in include/arcvae_hip.h, bound with the header's types, defined in csrc/swor.hip and built."""
import os
import re

import numpy as np

import swor_ref as R
from test_abi import ROOT, _ctype_of, _declared_args

END, PAD = 2, 0
V, T = 3, 2                                                     # 7 sequences: (2, pad), (0, x), (1, x)
NAMES = ("arcvae_dec_swor_ws_bytes", "arcvae_dec_swor")


def _chain(B, seed=11, same=False):
    """-> (table [B*V, V] f32, lse [B*V] f32, lp [B, V, V] f64): B rows of a V = 3 chain (one chain repeated if `same`)."""
    rs = np.random.RandomState(seed)
    table = rs.standard_normal((1 if same else B, V, V)).astype(np.float32)
    table = np.ascontiguousarray(np.broadcast_to(table, (B, V, V))).reshape(B * V, V)
    x = table.astype(np.float64)
    m = x.max(1)
    lse = (m + np.log(np.exp(x - m[:, None]).sum(1))).astype(np.float32)
    return table, lse, R.step_terms(table, lse, 1.0, np.float64).reshape(B, V, V)


def test_restatement_is_the_brute_force_top_k():
    """For every K the walk returns the K sequences of largest perturbed value of the WHOLE tree (values from the contract's
    formula as written), in order, with their log-probabilities, and the threshold is the (K+1)-th value."""
    B, seed = 16, 5
    table, lse, lp = _chain(B)
    for K in (1, 2, 4, 6):
        out = R.swor(table, lse, B, V, K, T, seed, END, PAD)
        for b in range(B):
            full = R.brute_force(lp[b], V, T, seed, b, END, PAD)
            assert len(full) == 7
            for k in range(K):
                assert tuple(out["tokens"][b, k]) == full[k][0], (K, b, k)
                assert abs(out["log_probs"][b, k] - full[k][1]) <= 1e-12
                assert abs(out["perturbed"][b, k] - full[k][2]) <= 1e-9
            assert abs(out["threshold"][b] - full[K][2]) <= 1e-9
            assert out["gap"][b] > 0
            assert list(out["lengths"][b]) == [1 if s[0] == END else T for s, _, _ in full[:K]]


def test_exhaustion_returns_every_sequence_once():
    B, seed = 8, 9
    table, lse, lp = _chain(B)
    out = R.swor(table, lse, B, V, 7, T, seed, END, PAD)
    for b in range(B):
        assert {tuple(s) for s in out["tokens"][b]} == set(R.sequence_probs(lp[b], V, T, END, PAD))
    assert np.all(np.isneginf(out["threshold"])) and np.all(np.isinf(out["gap"]))
    np.testing.assert_allclose(np.exp(out["log_probs"]).sum(1), 1.0, atol=1e-12)
    out = R.swor(table, lse, B, V, 9, T, seed, END, PAD)
    assert np.all(np.isneginf(out["log_probs"][:, 7:])) and np.all(np.isneginf(out["perturbed"][:, 7:]))
    assert np.all(out["lengths"][:, 7:] == 0) and np.all(out["tokens"][:, 7:] == PAD)
    assert np.all(np.isfinite(out["log_probs"][:, :7])) and np.all(np.diff(out["perturbed"][:, :7], axis=1) <= 0)
    for b in range(B):
        assert len({tuple(s) for s in out["tokens"][b, :7]}) == 7


def pair_z_scores(tokens, probs):
    """|z| of every ordered pair (rank 0, rank 1) with expected count >= 50 against Plackett-Luce, p_i p_j / (1 - p_i), over
    the rows of tokens [B, 2, T] drawn from one chain with sequence probabilities `probs` {tuple: p} -> (max |z|, cells)."""
    B = tokens.shape[0]
    seqs = sorted(probs)
    idx = {s: i for i, s in enumerate(seqs)}
    counts = np.zeros((len(seqs), len(seqs)))
    for b in range(B):
        counts[idx[tuple(tokens[b, 0])], idx[tuple(tokens[b, 1])]] += 1
    worst, cells = 0.0, 0
    for i, si in enumerate(seqs):
        for j, sj in enumerate(seqs):
            q = 0.0 if i == j else probs[si] * probs[sj] / (1.0 - probs[si])
            if B * q >= 50:
                worst = max(worst, abs(counts[i, j] - B * q) / np.sqrt(B * q * (1 - q)))
                cells += 1
            if i == j:
                assert counts[i, j] == 0
    return worst, cells


def test_ordered_pairs_follow_plackett_luce():
    B = 20000
    table, lse, lp = _chain(B, seed=3, same=True)
    out = R.swor(table, lse, B, V, 2, T, 2024, END, PAD)
    worst, cells = pair_z_scores(out["tokens"], R.sequence_probs(lp[0], V, T, END, PAD))
    print("max |z| =", worst, "over", cells, "cells")
    assert cells >= 20 and worst <= 5.0, (worst, cells)


def test_float32_restatement_stays_near_float64():
    """The float32 switch performs the same walk: same sets at a clear boundary, values within fp32 rounding of a short walk."""
    B, seed = 64, 21
    table, lse, _ = _chain(B)
    a = R.swor(table, lse, B, V, 3, T, seed, END, PAD, dtype=np.float64)
    c = R.swor(table, lse, B, V, 3, T, seed, END, PAD, dtype=np.float32)
    assert c["perturbed"].dtype == np.float32 and c["log_probs"].dtype == np.float32
    clear = a["gap"] >= 1e-3
    assert clear.sum() >= B // 2
    np.testing.assert_array_equal(a["tokens"][clear], c["tokens"][clear])
    assert np.abs(a["perturbed"][clear] - c["perturbed"][clear]).max() <= 1e-5
    assert np.abs(a["threshold"][clear] - c["threshold"][clear]).max() <= 1e-5


def test_declared_bound_and_defined():
    from arcvae_hip import _lib
    csrc = os.path.join(ROOT, "mlx-vae_amd", "csrc")
    decl = _declared_args()
    src = open(os.path.join(csrc, "swor.hip")).read()
    assert re.search(r"^SRCS\s*:=.*\bswor\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    for name in NAMES:
        assert name in decl, name
        assert re.search(r'extern "C"\s+int\s+' + name + r"\s*\(", src), name
        assert _lib.SIGNATURES[name] == [_ctype_of(d) for d in decl[name]], name
        assert hasattr(_lib.load(), name)
    assert "const unsigned long long* seed" in " ".join(decl["arcvae_dec_swor"])      # a device word, not a value


def test_weights_average_to_one_only_with_the_conditioning_taken_out():
    """The walk starts the root at G = 0: its perturbed values are drawn given that the row's largest is 0.  The estimator's
    weights (f = 1: their sum must average 1) are unbiased with `unconditioned` thresholds and visibly too small without."""
    import torch
    from models.decoder_sampling import importance_weights, unconditioned
    B, K, seed = 40000, 3, 1
    table, lse, _ = _chain(B, seed=3, same=True)
    out = R.swor(table, lse, B, V, K, T, seed, END, PAD)
    phi, G = torch.tensor(out["log_probs"]), torch.tensor(out["perturbed"])
    for kappa, biased in ((unconditioned(G[:, K - 1], seed), False), (G[:, K - 1], True)):
        s = importance_weights(phi, kappa)[:, :K - 1].sum(1).numpy()
        z = (s.mean() - 1.0) / (s.std(ddof=1) / np.sqrt(B))
        assert (z < -20) if biased else (abs(z) <= 5), (biased, s.mean(), z)
    free = unconditioned(G, seed).numpy()
    assert np.all(np.diff(free, axis=1) <= 0) and np.all(np.isfinite(free))
