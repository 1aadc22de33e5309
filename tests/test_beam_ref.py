"""The NumPy restatement of beam search (tests/beam_ref.py) against brute force and its own contract -- CPU only; the GPU
kernels are held to this restatement in tests/test_beam_gpu.py."""
import itertools

import numpy as np
import pytest

import beam_ref as R

END, PAD = 2, 0


def _canonical(seq, min_len):
    """A sequence as a hypothesis: pad after the first EOS; None if EOS comes before min_len."""
    seq = list(seq)
    if END in seq:
        e = seq.index(END)
        if e < min_len:
            return None
        seq = seq[:e + 1] + [PAD] * (len(seq) - e - 1)
    return tuple(seq)


def _brute(lp, b, V, T, min_len):
    """Every distinct hypothesis of length T with its fp64 score, best first."""
    out = {}
    for seq in itertools.product(range(V), repeat=T):
        c = _canonical(seq, min_len)
        if c is None or c in out:
            continue
        out[c] = float(R.sequence_logprob(lp[b * V:(b + 1) * V], np.array([c]), V, END)[0])
    return sorted(out.items(), key=lambda kv: -kv[1])


@pytest.mark.parametrize("V,T,min_len", [(3, 3, 0), (4, 3, 1), (5, 2, 0), (5, 3, 2), (6, 2, 1), (3, 3, 3)])
def test_exhaustive_width_is_brute_force(V, T, min_len):
    """K >= V^(T-1) keeps every prefix, so the search is exhaustive: its K hypotheses are the K best sequences."""
    rs = np.random.RandomState(V * 10 + T)
    B = 2
    table = rs.standard_normal((B * V, V)) * 2.0
    lp = R.step_terms(table, R.row_lse(table, 1.0), 1.0, np.float64)
    K = min(32, V ** (T - 1))
    toks, scores, lengths = R.beam_search(lp, B, V, K, T, min_len, END, PAD)
    for b in range(B):
        every = _brute(lp, b, V, T, min_len)
        score_of = dict(every)
        got = [tuple(int(x) for x in toks[b, k]) for k in range(K) if scores[b, k] > -np.inf]
        assert len(got) == min(K, len(every)) and len(set(got)) == len(got)
        # the K best values; sequences compared through their scores (two orders of the same transitions tie exactly)
        np.testing.assert_allclose(scores[b, :len(got)], [s for _, s in every[:len(got)]], rtol=1e-12)
        np.testing.assert_allclose([score_of[c] for c in got], scores[b, :len(got)], rtol=1e-12)
        for k in range(len(got)):
            e = [i for i, x in enumerate(got[k]) if x == END]
            assert lengths[b, k] == (e[0] + 1 if e else T)
            assert not e or e[0] >= min_len


def test_width_one_is_the_first_argmax_walk():
    rs = np.random.RandomState(5)
    B, V, T = 4, 12, 20
    table = np.round(rs.standard_normal((B * V, V)) * 8) / 8        # ties: the first maximal index wins
    table[:, END] -= 1.0                                             # long walks
    lp = R.step_terms(table, R.row_lse(table, 1.0), 1.0)
    toks, scores, lengths = R.beam_search(lp, B, V, 1, T, 0, END, PAD)
    for b in range(B):
        c, walk = 0, []
        for t in range(T):
            c = int(np.argmax(table[b * V + c]))
            walk.append(c)
            if c == END:
                break
        n = len(walk)
        assert list(toks[b, 0, :n]) == walk and np.all(toks[b, 0, n:] == PAD)
        assert lengths[b, 0] == (n if walk[-1] == END else T)
        assert scores[b, 0] == R.sequence_logprob(lp[b * V:(b + 1) * V], toks[b:b + 1, 0], V, END)[0]


def test_min_length_absorbing_eos_and_padding():
    """EOS is the best token everywhere: with min_len 3 it first appears at t = 3; then the hypothesis pads and keeps its
    score; every returned score is the log-likelihood of its tokens."""
    rs = np.random.RandomState(1)
    B, V, K, T = 3, 7, 4, 9
    table = rs.standard_normal((B * V, V)).astype(np.float32)
    table[:, END] += 6.0
    lp = R.step_terms(table, R.row_lse(table, 1.0).astype(np.float32), 1.0)
    toks, scores, lengths = R.beam_search(lp, B, V, K, T, 3, END, PAD)
    for b in range(B):
        for k in range(K):
            e = np.flatnonzero(toks[b, k] == END)
            assert e.size and e[0] >= 3
            assert lengths[b, k] == e[0] + 1
            assert np.all(toks[b, k, e[0] + 1:] == PAD)
        assert np.all(np.diff(scores[b]) <= 0)
        np.testing.assert_array_equal(scores[b], R.sequence_logprob(lp, toks[b], V, END, batch=[b] * K))
    assert np.all(lengths[:, 0] == 4)                   # EOS as early as allowed is the best hypothesis here


def test_tie_order_on_integer_tables():
    """All-equal rows: every candidate ties, so the order is parent slot, then token: slot k after step 0 is token k, and
    after step 1 slot k extends parent 0 with token k."""
    B, V, K, T = 1, 6, 4, 3
    lp = R.step_terms(np.zeros((B * V, V), np.float32), R.row_lse(np.zeros((B * V, V)), 1.0).astype(np.float32), 1.0)
    toks, scores, lengths = R.beam_search(lp, B, V, K, T, 2, END, PAD)
    # t = 0: tokens 0, 1, 3, 4 (EOS excluded); t = 1 and 2: the first children of parent 0 (history 0, 0) win every tie
    assert toks[0, :, 0].tolist() == [0, 0, 0, 0]
    assert toks[0, :, 1].tolist() == [0, 0, 0, 0]
    assert toks[0, :, 2].tolist() == [0, 1, 2, 3]
    assert np.all(scores[0] == scores[0, 0])
    assert lengths[0].tolist() == [3, 3, 3, 3]


def test_fewer_candidates_than_slots_leave_empty_slots():
    B, V, K, T = 2, 3, 8, 2
    table = np.random.RandomState(2).standard_normal((B * V, V)).astype(np.float32)
    lp = R.step_terms(table, R.row_lse(table, 1.0).astype(np.float32), 1.0)
    toks, scores, lengths = R.beam_search(lp, B, V, K, T, 0, END, PAD)
    n = 3 * 2 + 1                                         # 2 live x 3 children + the finished EOS hypothesis's pad
    assert np.all(scores[:, :n] > -np.inf) and np.all(scores[:, n:] == -np.inf)
    assert np.all(lengths[:, n:] == 0) and np.all(toks[:, n:] == PAD)
