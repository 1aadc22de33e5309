"""The NumPy restatement of length-normalised exact decoding (tests/length_norm_ref.py) against enumeration of every admissible
sequence, bit for bit in fp32, and against the un-normalised restatements -- on the CPU: what tests/test_length_norm_gpu.py then
holds the kernels to.  Also the three entry points' presence in the header and the binding (tests/test_abi.py covers their types)."""
import numpy as np
import pytest

import beam_ref as R
import chain_ref as X
import kbest_ref as KB
import length_norm_ref as LN

END, PAD = 2, 0
B = 3
KS = (1, 3, 7, 32)
ALPHAS = (0.0, 0.5, 1.0, 2.0)
KINDS = ("normal", "q8d", "normal-lowered-end")
TABLES = [(V, T, kind) for V in (3, 4, 5) for T in (4, 5, 6) for kind in KINDS]
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _table(V, T, kind):
    """Step terms and the enumeration of every row of a table: computed once, shared, never modified."""
    key = (V, T, kind)
    if key not in _cache:
        table, lse = KB.make_table(np.random.RandomState(V * 100 + T * 10 + KINDS.index(kind)), B, V, kind, 1.0, END)
        lp = R.step_terms(table, lse, 1.0)
        lp.setflags(write=False)
        _cache[key] = (lp, [LN.enumerate_all(lp, b, V, T, END) for b in range(B)])
    return _cache[key]


def _divisor_sets(T, kind):
    out = [(f"alpha {a}", LN.divisors(a, T)) for a in ALPHAS]
    if kind == "q8d":
        out.append(("ties", LN.tie_divisors(T)))
    return out


def test_divisors():
    np.testing.assert_array_equal(LN.tie_divisors(6), np.array([1, 2, 2, 4, 4, 8], dtype=np.float32))
    np.testing.assert_array_equal(LN.divisors(0.0, 5), np.ones(5, dtype=np.float32))
    np.testing.assert_array_equal(LN.divisors(1.0, 5), np.arange(1, 6, dtype=np.float32))
    assert LN.divisors(0.5, 4)[1] == np.float32(2.0 ** 0.5) and LN.divisors(0.5, 4).dtype == np.float32


@pytest.mark.parametrize("V,T,kind", TABLES)
def test_enumeration_is_the_sequence_logprob(V, T, kind):
    """The enumeration's counts, and its sums against beam_ref.sequence_logprob on the sequences the restatement returns (the
    enumeration keeps no tokens: its maximum per length is compared below, here that raw IS the log-likelihood of the tokens)."""
    lp, enum = _table(V, T, kind)
    raw, n, ended = enum[0]
    assert raw.size == sum((V - 1) ** k for k in range(T)) + (V - 1) ** T and raw.dtype == np.float32
    assert np.sum(~ended) == (V - 1) ** T and np.all(n[~ended] == T)
    for name, d in _divisor_sets(T, kind):
        for min_len in (0, 1, 2):
            tok, key, rw, ln, _, _ = LN.viterbi_norm(lp, B, V, T, min_len, END, PAD, d)
            np.testing.assert_array_equal(_bits(R.sequence_logprob(lp, tok, V, END)), _bits(rw), err_msg=name)
            np.testing.assert_array_equal(_bits(rw / d[ln - 1]), _bits(key), err_msg=name)
            for b in range(B):
                ends = np.flatnonzero(tok[b] == END)
                assert (ends.size and ends[0] + 1 == ln[b] and ends[0] >= min_len) or (not ends.size and ln[b] == T)
                assert np.all(tok[b, ln[b]:] == PAD)


@pytest.mark.parametrize("V,T,kind", TABLES)
def test_viterbi_norm_is_the_enumerated_maximum(V, T, kind):
    """fp32, bit for bit: the key is the maximum key over every admissible sequence; by_length[n-1] is the best enumerated raw
    score of the sequences that end at length n (whatever min_len is), open_score the best of those that do not end."""
    lp, enum = _table(V, T, kind)
    for name, d in _divisor_sets(T, kind):
        for min_len in (0, 1, 2):
            tok, key, rw, ln, by_length, opens = LN.viterbi_norm(lp, B, V, T, min_len, END, PAD, d)
            for b in range(B):
                raw, n, ended = enum[b]
                keys = LN.keys_of(raw, n, ended, min_len, d)
                assert _bits(key[b]) == _bits(keys[0]), (name, min_len, b)
                for m in range(1, T + 1):
                    assert _bits(by_length[b, m - 1]) == _bits(raw[ended & (n == m)].max()), (name, m)
                assert _bits(opens[b]) == _bits(raw[~ended].max())


@pytest.mark.parametrize("V,T,kind", TABLES)
def test_kbest_norm_keys_are_the_k_largest_enumerated(V, T, kind):
    """fp32, bit for bit: the K keys are the K largest keys over every admissible sequence, as a multiset (-inf in the slots no
    sequence fills), descending; the sequences are pairwise distinct; each raw score is the log-likelihood of its tokens and each
    key its raw score over its length's divisor; K = 1 is the Viterbi restatement."""
    lp, enum = _table(V, T, kind)
    for name, d in _divisor_sets(T, kind):
        for min_len in (0, 1, 2):
            vit = LN.viterbi_norm(lp, B, V, T, min_len, END, PAD, d)
            for K in KS:
                tok, key, rw, ln = LN.kbest_norm(lp, B, V, K, T, min_len, END, PAD, d)
                for b in range(B):
                    keys = LN.keys_of(*enum[b], min_len, d)
                    np.testing.assert_array_equal(_bits(key[b]), _bits(LN.top(keys, K)), err_msg=f"{name} {min_len} {K} {b}")
                    assert np.all(key[b, :-1] >= key[b, 1:])
                    full = ln[b] > 0
                    assert np.sum(full) == min(K, keys.size) and np.all(full[:np.sum(full)])
                    assert len({tuple(s) for s in tok[b, full]}) == np.sum(full)
                    np.testing.assert_array_equal(_bits(R.sequence_logprob(lp, tok[b, full], V, END, batch=[b] * np.sum(full))),
                                                  _bits(rw[b, full]))
                    np.testing.assert_array_equal(_bits(rw[b, full] / d[ln[b, full] - 1]), _bits(key[b, full]))
                if K == 1:
                    np.testing.assert_array_equal(tok[:, 0], vit[0])
                    np.testing.assert_array_equal(_bits(key[:, 0]), _bits(vit[1]))
                    np.testing.assert_array_equal(_bits(rw[:, 0]), _bits(vit[2]))
                    np.testing.assert_array_equal(ln[:, 0], vit[3])


@pytest.mark.parametrize("V,T,kind", TABLES)
def test_alpha_zero_is_the_unnormalised_restatement(V, T, kind):
    """Divisors of one (alpha = 0, or none given) return chain_ref.viterbi's and kbest_ref.kbest's tokens, lengths and score bits."""
    lp, _ = _table(V, T, kind)
    for d in (LN.divisors(0.0, T), None):
        for min_len in (0, 1, 2, T):
            tok, key, rw, ln, _, _ = LN.viterbi_norm(lp, B, V, T, min_len, END, PAD, d)
            vtok, vsc, vln = X.viterbi(lp, B, V, T, min_len, END, PAD)
            np.testing.assert_array_equal(tok, vtok)
            np.testing.assert_array_equal(ln, vln)
            np.testing.assert_array_equal(_bits(key), _bits(vsc))
            np.testing.assert_array_equal(_bits(rw), _bits(vsc))
            for K in KS:
                tok, key, rw, ln = LN.kbest_norm(lp, B, V, K, T, min_len, END, PAD, d)
                ktok, ksc, kln = KB.kbest(lp, B, V, K, T, min_len, END, PAD)
                np.testing.assert_array_equal(tok, ktok)
                np.testing.assert_array_equal(ln, kln)
                np.testing.assert_array_equal(_bits(key), _bits(ksc))
                np.testing.assert_array_equal(_bits(rw), _bits(ksc))


def test_the_earliest_end_wins_a_tie_across_lengths():
    """On "q8d" tables with the divisors [1, 2, 2, 4, 4, 8] every key is exact, and in some of the 48 rows per table the best key IS
    attained at more than one length (asserted: otherwise the rule is not exercised).  The restatement then returns the SHORTEST of
    the tying end candidates, the open candidate only when it is strictly better than every end candidate, and the key is the
    enumerated maximum all the same."""
    rows, ties = 48, 0
    for V in (3, 4, 5):
        for T in (4, 5, 6):
            table, lse = KB.make_table(np.random.RandomState(V * 100 + T), rows, V, "q8d", 1.0, END)
            lp = R.step_terms(table, lse, 1.0)
            d = LN.tie_divisors(T)
            for min_len in (0, 1, 2):
                tok, key, rw, ln, by_length, opens = LN.viterbi_norm(lp, rows, V, T, min_len, END, PAD, d)
                for b in range(rows):
                    cand = by_length[b] / d                                  # exact: multiples of 1/8 over powers of two
                    cand[:min_len] = -np.inf
                    open_key = opens[b] / d[T - 1]
                    best = max(cand.max(), open_key)
                    assert key[b] == best
                    at = np.flatnonzero(cand == best)
                    if at.size:
                        assert ln[b] == at[0] + 1 and tok[b, at[0]] == END   # the earliest end, even if the open one ties
                    else:
                        assert ln[b] == T and END not in tok[b]
                    if at.size + (open_key == best) > 1:
                        ties += 1
                        assert _bits(key[b]) == _bits(LN.keys_of(*LN.enumerate_all(lp, b, V, T, END), min_len, d)[0])
    print("rows whose best key ties across lengths:", ties)
    assert ties >= 1


def test_the_penalty_moves_the_chosen_lengths():
    """V 12, T 16, eight rows of the "normal" table: alpha = 0.5 does not choose alpha = 0's lengths (what the GPU test asserts of
    the kernel), and mixes early ends, late ends and open sequences."""
    V, T, rows = 12, 16, 8
    table, lse = KB.make_table(np.random.RandomState(V * 1000 + T), rows, V, "normal", 1.0, END)
    lp = R.step_terms(table, lse, 1.0)
    l0 = LN.viterbi_norm(lp, rows, V, T, 0, END, PAD, LN.divisors(0.0, T))[3]
    l5 = LN.viterbi_norm(lp, rows, V, T, 0, END, PAD, LN.divisors(0.5, T))[3]
    print("lengths at alpha 0:", l0.tolist(), "at alpha 0.5:", l5.tolist())
    assert not np.array_equal(l0, l5)
    assert len(set(l5.tolist())) >= 3 and T in l5 and l5.min() < 4                 # early ends, late ends or open ones, mixed


def test_trace_follows_the_pointers():
    """trace(n) returns, for every n, a sequence with its first end token at position n-1 and pads after, whose log-likelihood is
    by_length[n-1] bit for bit; n = 0 gives pads only; lengths are clamped into [0, max_len]."""
    V, T = 5, 6
    lp, _ = _table(V, T, "normal")
    by_length = LN.viterbi_norm(lp, B, V, T, 0, END, 7, None)[4]
    for n in range(1, T + 1):
        tok = LN.trace(lp, B, V, T, [n] * B, END, 7)
        assert np.all(tok[:, n - 1] == END) and not np.any(tok[:, :n - 1] == END) and np.all(tok[:, n:] == 7)
        np.testing.assert_array_equal(_bits(R.sequence_logprob(lp, tok, V, END)), _bits(by_length[:, n - 1]))
    assert np.all(LN.trace(lp, B, V, T, [0, -3, 0], END, 7) == 7)
    np.testing.assert_array_equal(LN.trace(lp, B, V, T, [T + 5] * B, END, 7), LN.trace(lp, B, V, T, [T] * B, END, 7))


def test_entry_points_are_declared_and_bound():
    import os
    import re
    from arcvae_hip import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "arcvae_hip.h")).read()
    for name, n in (("arcvae_dec_viterbi_norm", 19), ("arcvae_dec_viterbi_trace", 10), ("arcvae_dec_kbest_norm", 18)):
        assert re.search(rf"\bint\s+{name}\s*\(", header)
        assert len(_lib.SIGNATURES[name]) == n
