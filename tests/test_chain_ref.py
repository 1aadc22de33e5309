"""The NumPy restatement of exact MAP decoding and of the chain marginals (tests/chain_ref.py) against brute force, against the
beam restatement and against fp64 -- on the CPU: what tests/test_chain_gpu.py then holds the kernels to, bit for bit."""
import numpy as np
import pytest

import beam_ref as R
import chain_ref as X

END, PAD = 2, 0
U = 2.0 ** -24


def _terms(seed, B, V, kind, temp, dtype=np.float32, lower=4.0):
    table = X.make_table(np.random.RandomState(seed), B, V, kind, END, lower)
    lse = R.row_lse(table, temp).astype(np.float32)
    return R.step_terms(table, lse, temp, dtype)


@pytest.mark.parametrize("kind", ["q8", "normal"])
@pytest.mark.parametrize("temp", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("V,T,min_len", [(4, 6, 0), (5, 5, 2), (4, 7, 7), (6, 4, 0)])
def test_viterbi_is_the_enumerated_maximum(V, T, min_len, temp, kind):
    """fp32, 4 rows: the score is BIT-equal to the maximum over every admissible sequence, and it is the left-to-right fp32
    log-likelihood of the returned tokens.  END = 2 < V; the q8 tables tie often inside a row."""
    B = 4
    lp = _terms(V * 100 + T, B, V, kind, temp)
    tok, sc, ln = X.viterbi(lp, B, V, T, min_len, END, PAD)
    for b in range(B):
        ref = X.brute_force(lp, b, V, T, min_len, END)
        assert sc[b].view(np.uint32) == np.float32(ref).view(np.uint32), (b, sc[b], ref)
    again = R.sequence_logprob(lp, tok, V, END)
    np.testing.assert_array_equal(again.view(np.uint32), sc.view(np.uint32))
    _check_admissible(tok, ln, V, T, min_len)


def _check_admissible(tok, ln, V, T, min_len):
    for row, n in zip(tok, ln):
        assert 1 <= n <= T and np.all(row[n:] == PAD) and np.all((row[:n] >= 0) & (row[:n] < V))
        assert not np.any(row[:n - 1] == END)
        if row[n - 1] == END:
            assert n - 1 >= min_len
        else:
            assert n == T


def test_exact_ties_take_the_earliest_end_then_the_lowest_token():
    """A flat table (every step term equal): every sequence of a given length ties.  min_len 0: the one-token sequence `end`
    (the earliest-ending candidate); min_len = max_len: no end allowed, the lowest tokens all the way (0 is not the end token)."""
    B, V, T = 2, 5, 6
    lp = np.full((B * V, V), -np.log(V), dtype=np.float32)
    tok, sc, ln = X.viterbi(lp, B, V, T, 0, END, PAD)
    assert np.all(ln == 1) and np.all(tok[:, 0] == END) and np.all(tok[:, 1:] == PAD)
    tok, sc, ln = X.viterbi(lp, B, V, T, T, END, 7)
    assert np.all(ln == T) and np.all(tok == 0)
    tok, sc, ln = X.viterbi(lp, B, V, T, 3, END, 7)                 # fewer additions never lose: -k log V decreases in k
    assert np.all(ln == 4) and np.all(tok[:, :3] == 0) and np.all(tok[:, 3] == END) and np.all(tok[:, 4:] == 7)


@pytest.mark.parametrize("V,T,min_len,kind", [(80, 64, 5, "normal"), (80, 64, 5, "q8"), (256, 48, 2, "q8"), (256, 48, 2, "normal")])
def test_map_score_is_never_below_the_beam(V, T, min_len, kind):
    B = 6
    lp = _terms(V * 1000 + T, B, V, kind, 1.0)
    tok, sc, ln = X.viterbi(lp, B, V, T, min_len, END, PAD)
    _check_admissible(tok, ln, V, T, min_len)
    np.testing.assert_array_equal(R.sequence_logprob(lp, tok, V, END).view(np.uint32), sc.view(np.uint32))
    for K in (1, 4, 32):
        _, bsc, _ = R.beam_search(lp, B, V, K, T, min_len, END, PAD)
        assert np.all(sc >= bsc[:, 0]), (K, sc, bsc[:, 0])
        if K == 1 and V == 80 and kind == "normal":
            assert np.any(sc > bsc[:, 0])                           # (not vacuous: greedy misses the optimum)


@pytest.mark.parametrize("V,T,kind", [(80, 128, "q8-lowered-end"), (12, 40, "normal-lowered-end"), (256, 16, "normal-lowered-end")])
@pytest.mark.parametrize("lower", [4.0, None])
def test_long_sequences_run_to_max_len(V, T, kind, lower):
    """With the end column lowered far enough the optimum does not end: the unfinished branch and back-traces of max_len steps.
    Lowered by 4 (every check but the length: at about 2 nats per step the optimum still ends after a few tokens, measured
    lengths 1 to 3 at V 80) and by 4 * max_len (None), where at least half the rows must run to max_len."""
    B = 6
    lp = _terms(V * 1000 + T, B, V, kind, 1.0, lower=4.0 * T if lower is None else lower)
    tok, sc, ln = X.viterbi(lp, B, V, T, 0, END, PAD)
    if lower is None:
        assert np.sum(ln == T) >= B // 2, ln
    _check_admissible(tok, ln, V, T, 0)
    np.testing.assert_array_equal(R.sequence_logprob(lp, tok, V, END).view(np.uint32), sc.view(np.uint32))
    _, bsc, _ = R.beam_search(lp, B, V, 4, T, 0, END, PAD)
    assert np.all(sc >= bsc[:, 0])


@pytest.mark.parametrize("V,T,temp", [(12, 16, 1.0), (12, 24, 0.7), (80, 12, 1.0)])
def test_marginals_fp32_against_fp64(V, T, temp):
    """Both recursions run over the same fp32 step terms, so only exp, the products and the sums differ: per step at most
    (V + 8) * 2^-24 relative for any order of V non-negative products.  The fp64 total mass (length distribution + survival) is
    1 to 1e-5: the fp32 lse normalises a row only to about 1e-7 * |lse|."""
    B = 4
    lp = _terms(V * 10 + T, B, V, "normal", temp)
    ref = X.marginals(lp, B, V, T, END, np.float64)
    got = X.marginals(lp, B, V, T, END, np.float32).astype(np.float64)
    bound = (np.arange(T) + 1)[None, :, None] * (V + 8) * U
    ok = ref >= 1e-30
    rel = np.abs(got / np.where(ok, ref, 1.0) - 1.0)
    assert np.all(rel[ok] <= np.broadcast_to(bound, rel.shape)[ok]), (rel / bound)[ok].max()
    total = X.length_distribution(ref, END).sum(axis=1)
    assert np.all(np.abs(total - 1.0) <= 1e-5), total
    # alive is a sub-distribution that only loses mass: what is alive at t either ends or stays alive at t + 1
    alive_mass = np.delete(ref, END, axis=2).sum(axis=2)
    assert np.all(np.diff(alive_mass, axis=1) <= 1e-6)
