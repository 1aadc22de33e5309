"""The NumPy restatement of exact K-best decoding (tests/kbest_ref.py) against brute-force enumeration, against the Viterbi and the
beam restatements and against the sequence log-likelihood -- on the CPU: what tests/test_kbest_gpu.py then holds the kernel to,
bit for bit.  Also the entry points' presence in the header and the binding (the checks of tests/test_abi.py cover their types)."""
import numpy as np
import pytest

import beam_ref as R
import chain_ref as X
import kbest_ref as KB

PAD = 0
B = 6

# (V, max_len, K, min_len, temperature, kind).  The end token is 2, or 1 at V 2.  "q8d": exact sums, ties everywhere; the two
# first cases must tie between adjacent returned scores in every row.  (3, 3, 32): 1 + 2 + 4 + 8 = 15 admissible sequences, fewer
# than K (none ends at min_len 3: 8).  min_len 0, in the middle and = max_len (the end token never allowed).
TIE_CASES = [(5, 5, 16, 2, 1.0, "q8d"), (4, 6, 32, 0, 1.0, "q8d")]
CASES = TIE_CASES + [
    (3, 3, 32, 0, 1.0, "q8d"), (3, 3, 32, 3, 1.0, "q8"), (2, 6, 8, 0, 1.0, "normal"), (2, 5, 4, 5, 1.0, "q8"),
    (2, 6, 32, 3, 1.0, "q8d"), (5, 6, 1, 0, 1.0, "normal"), (5, 6, 4, 3, 0.7, "normal"), (4, 6, 8, 6, 1.0, "q8"),
    (5, 5, 32, 0, 1.0, "q8-lowered-end"), (4, 5, 2, 2, 1.3, "q8-lowered-end"), (5, 4, 16, 4, 1.0, "normal"),
    (5, 6, 32, 1, 1.0, "q8"), (4, 4, 3, 0, 1.0, "q8d"), (5, 3, 5, 0, 0.7, "q8-lowered-end")]


def _end(V):
    return min(2, V - 1)


_cache = {}


def _case(V, T, K, min_len, temp, kind):
    """Step terms, the restatement's outputs and the enumerated scores of a case: computed once, shared, never modified."""
    key = (V, T, K, min_len, temp, kind)
    if key not in _cache:
        end = _end(V)
        table, lse = KB.make_table(np.random.RandomState(V * 1000 + T * 10 + K), B, V, kind, temp, end)
        lp = R.step_terms(table, lse, temp)
        out = KB.kbest(lp, B, V, K, T, min_len, end, PAD)
        brute = [KB.brute_force_scores(lp, b, V, T, min_len, end) for b in range(B)]
        for a in (lp,) + out:
            a.setflags(write=False)
        _cache[key] = (lp, out, brute)
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("V,T,K,min_len,temp,kind", CASES)
def test_scores_are_the_k_largest_enumerated(V, T, K, min_len, temp, kind):
    """fp32: the K scores are BIT-equal to the K largest contract scores over every admissible sequence (-inf in the slots that
    no sequence fills), and they descend."""
    lp, (tok, sc, ln), brute = _case(V, T, K, min_len, temp, kind)
    for b in range(B):
        np.testing.assert_array_equal(_bits(sc[b]), _bits(KB.top_scores(brute[b], K)))
        assert np.all(sc[b, :-1] >= sc[b, 1:])
        assert np.sum(sc[b] > -np.inf) == min(K, brute[b].size)
    if (V, T, K) == (3, 3, 32):
        assert np.all(np.isneginf(sc[:, -1]))                        # (the case with fewer than K admissible sequences)


@pytest.mark.parametrize("V,T,K,min_len,temp,kind", CASES)
def test_sequences_are_distinct_admissible_and_scored(V, T, K, min_len, temp, kind):
    """Every returned sequence is admissible (min_len honoured, nothing after the first end, length as reported, padded), the K of
    a row are pairwise distinct, and the left-to-right fp32 log-likelihood of each is BIT-equal to its score; an unfilled slot has
    length 0 and pad tokens only."""
    end = _end(V)
    lp, (tok, sc, ln), _ = _case(V, T, K, min_len, temp, kind)
    for b in range(B):
        seen = set()
        for j in range(K):
            row, n = tok[b, j], int(ln[b, j])
            if not sc[b, j] > -np.inf:
                assert n == 0 and np.all(row == PAD)
                continue
            assert 1 <= n <= T and np.all(row[n:] == PAD) and np.all((row[:n] >= 0) & (row[:n] < V))
            assert not np.any(row[:n - 1] == end)
            if row[n - 1] == end:
                assert n - 1 >= min_len
            else:
                assert n == T
            seen.add(tuple(row[:n]))
        assert len(seen) == int(np.sum(sc[b] > -np.inf))
    filled = sc.reshape(-1) > -np.inf
    again = R.sequence_logprob(lp, tok.reshape(B * K, T)[filled], V, end, batch=np.repeat(np.arange(B), K)[filled])
    np.testing.assert_array_equal(_bits(again), _bits(sc.reshape(-1)[filled]))


@pytest.mark.parametrize("V,T,K,min_len,temp,kind", CASES)
def test_k1_is_viterbi_and_no_rank_is_below_the_beam(V, T, K, min_len, temp, kind):
    end = _end(V)
    lp, (tok, sc, ln), _ = _case(V, T, K, min_len, temp, kind)
    tok1, sc1, ln1 = KB.kbest(lp, B, V, 1, T, min_len, end, PAD)
    vtok, vsc, vln = X.viterbi(lp, B, V, T, min_len, end, PAD)
    np.testing.assert_array_equal(tok1[:, 0], vtok)
    np.testing.assert_array_equal(ln1[:, 0], vln)
    np.testing.assert_array_equal(_bits(sc1[:, 0]), _bits(vsc))
    np.testing.assert_array_equal(tok[:, 0], vtok)                   # rank 0 of any K is the same sequence
    np.testing.assert_array_equal(_bits(sc[:, 0]), _bits(vsc))
    _, bsc, _ = R.beam_search(lp, B, V, K, T, min_len, end, PAD)
    assert np.all(sc >= bsc), (sc, bsc)


@pytest.mark.parametrize("V,T,K,min_len,temp,kind", TIE_CASES)
def test_tie_cases_tie_in_every_row(V, T, K, min_len, temp, kind):
    _, (tok, sc, ln), _ = _case(V, T, K, min_len, temp, kind)
    for b in range(B):
        s = sc[b][sc[b] > -np.inf]
        assert np.any(s[:-1] == s[1:]), (b, s)


def test_the_beam_misses_somewhere():
    """Not vacuous: over the cases without built-in ties, some rank of some row is STRICTLY above the beam's at the same K."""
    strictly = 0
    for case in CASES:
        if case[5] == "q8d" or case[2] == 1:
            continue
        V, T, K, min_len, temp, kind = case
        lp, (tok, sc, ln), _ = _case(*case)
        _, bsc, _ = R.beam_search(lp, B, V, K, T, min_len, _end(V), PAD)
        strictly += int(np.sum(np.any(sc > bsc, axis=1)))
    assert strictly > 0


def test_flat_table_tie_rules():
    """Every step term equal: all sequences of one length tie, shorter ones score higher.  The result order is then the
    contract's arrival order: the earlier end first, then (at max_len) the lower last token, then the lower rank -- and within a
    list (u asc, r' asc)."""
    V, T, K, end = 4, 3, 8, 2
    lp = np.full((V, V), -np.log(V), dtype=np.float32)
    tok, sc, ln = KB.kbest(lp, 1, V, K, T, 0, end, 9)
    assert ln[0].tolist() == [1, 2, 2, 2, 3, 3, 3, 3]
    assert tok[0, :5].tolist() == [[2, 9, 9], [0, 2, 9], [1, 2, 9], [3, 2, 9], [0, 0, 2]]
    assert tok[0, 5:].tolist() == [[1, 0, 2], [3, 0, 2], [0, 1, 2]]   # (u = 0 with its ranks r' = 0, 1, 2, then u = 1)
    tok, sc, ln = KB.kbest(lp, 1, V, K, T, T, end, 9)                  # no end: last token 0 first, its ranks by (u, r')
    assert np.all(ln == T)
    assert tok[0].tolist() == [[0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 1, 0], [1, 1, 0], [3, 1, 0], [0, 3, 0], [1, 3, 0]]


def test_first_k_stable_is_the_stable_argsort():
    rs = np.random.RandomState(0)
    for N, C, K in [(40, 7, 5), (12, 3, 12), (64, 5, 1), (30, 4, 29)]:
        cand = (np.round(rs.standard_normal((N, C)) * 2) / 2).astype(np.float32)       # many ties
        cand[rs.rand(N, C) < 0.3] = -np.inf
        want = np.argsort(-cand, axis=0, kind="stable")[:K]
        got = KB.first_k_stable(cand, K)
        fin = np.take_along_axis(cand, want, axis=0) > -np.inf          # (rows of -inf are empty: their order is immaterial)
        np.testing.assert_array_equal(got[fin], want[fin])
        np.testing.assert_array_equal(np.take_along_axis(cand, got, axis=0), np.take_along_axis(cand, want, axis=0))


def test_entry_points_are_declared_and_bound():
    import test_abi as A
    from arcvae_hip import _lib
    d = A._declared_args()
    for name, n in (("arcvae_dec_kbest_ws_bytes", 5), ("arcvae_dec_kbest", 16)):
        assert name in d and len(d[name]) == n and name in _lib.SIGNATURES
        assert [A._ctype_of(a) for a in d[name]] == list(_lib.SIGNATURES[name])
