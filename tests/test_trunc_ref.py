"""tests/trunc_ref.py against brute-force set definitions, its reductions to tests/topkp_ref.py, and its walk (no GPU needed)."""
import numpy as np
import pytest

import topkp_ref as T
import trunc_ref as R


def _rows(V, n, seed):
    rs = np.random.RandomState(seed)
    rows = rs.standard_normal((n, V)).astype(np.float32) * 2
    rows[1, :] = 0.25                                                # flat
    rows[2, 1] = rows[2, 0]                                          # a tie
    if V > 3:
        rows[3, 3] = -200.0                                          # e underflows to 0
    return T.scaled(rows, 0.7)


@pytest.mark.parametrize("V", [3, 17, 80])
def test_min_p_set_is_the_brute_force_set(V):
    for s in _rows(V, 6, V):
        for k in (0, 2, 5, V + 3):
            for mp in (0.01, 0.1, 0.5):
                for p in (1.0, 0.9):
                    r = R.truncate(s, k, p, mp)
                    Kset, P = T.brute_force_sets(s, k, p)
                    s64 = s.astype(np.float64)
                    pr = np.exp(s64 - s64.max())
                    want = {i for i in P if pr[i] >= float(np.float32(mp)) * pr.max()} | {int(T.order(s)[0])}
                    assert set(r.tokens[:r.n].tolist()) == want, (k, mp, p)
                    assert set(r.tokens[:r.K].tolist()) == Kset


@pytest.mark.parametrize("V", [3, 17, 80])
def test_typical_set_and_entropy_by_enumeration(V):
    for s in _rows(V, 6, V + 1):
        for k in (0, 2, 5, V + 3):
            for tp in (0.2, 0.5, 0.9, 0.95):
                r = R.truncate(s, k, typical_p=tp)
                Kset, _ = T.brute_force_sets(s, k)
                so = T.order(s)
                pos = {int(t): i for i, t in enumerate(so)}
                s64 = s.astype(np.float64)
                mass = {i: np.exp(s64[i] - s64.max()) for i in Kset}
                M = sum(sorted(mass.values()))
                prob = {i: mass[i] / M for i in Kset}
                H = -sum(prob[i] * (s64[i] - s64.max() - np.log(M)) for i in Kset)
                np.testing.assert_allclose(r.H, H, rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(r.H, -sum(q * np.log(q) for q in prob.values() if q > 0), rtol=1e-9, atol=1e-12)
                d = {i: abs(s64[i] - s64.max() - np.log(M) + r.H) for i in Kset}
                kept = set()
                for i in Kset:
                    ahead = [j for j in Kset if (d[j], pos[j]) < (d[i], pos[i])]
                    if not ahead or sum(mass[j] for j in ahead) < float(np.float32(tp)) * r.C[-1]:
                        kept.add(i)
                assert set(r.tokens[:r.n].tolist()) == kept, (k, tp)
                assert sorted(r.tokens.tolist()) == list(range(V))
                np.testing.assert_array_equal(r.tokens[r.K:], so[r.K:])
                assert np.all(np.diff(r.d) >= 0)


def test_reductions_to_topkp_ref():
    for s in _rows(80, 6, 5):
        for k, p in ((0, 1.0), (5, 0.9), (0, 0.5), (100, 1.0)):
            o, K, e, C, n, before, thr = T.truncate(s, k, p)
            r = R.truncate(s, k, p, 0.0, 1.0)
            np.testing.assert_array_equal(r.tokens, o)
            assert (r.K, r.n, r.thr) == (K, n, thr)
            np.testing.assert_array_equal(r.e, e)
            np.testing.assert_array_equal(r.C, C)
            np.testing.assert_array_equal(R.truncated_probs(s, 1.0, k, p), T.truncated_probs(s, 1.0, k, p))


def test_banned_token_and_probabilities():
    V = 17
    for s in _rows(V, 6, 9):
        top = int(T.order(s)[0])
        for ban in (top, 2):
            for kw in (dict(), dict(min_p=0.1), dict(top_p=0.9, min_p=0.05), dict(typical_p=0.9), dict(top_k=V + 4, typical_p=0.5),
                       dict(top_k=V), dict(top_k=3)):
                r = R.truncate(s, ban=ban, **kw)
                assert ban not in r.tokens[:r.K] and r.tokens[-1] == ban
                assert r.K == min(kw.get("top_k") or V, V - 1)
                pr = R.truncated_probs(s, 1.0, ban=ban, **kw)
                assert pr[ban] == 0 and abs(pr.sum() - 1) < 1e-12 and (pr >= 0).all()
        for kw in (dict(min_p=0.3), dict(typical_p=0.3), dict(top_k=4, typical_p=0.9)):
            assert abs(R.truncated_probs(s, 0.7, **kw).sum() - 1) < 1e-12
    assert R.set_size(2, 0, ban=1) == 1 and R.set_size(80, 20, ban=2) == 20 and R.set_size(80, 0) == 80


def test_walk_masks_the_end_token_before_min_len():
    B, V, Tn, END = 5, 12, 16, 2
    rs = np.random.RandomState(3)
    table = T.scaled(rs.standard_normal((B * V, V)).astype(np.float32), 1.0)
    table[:, END] += 3.0                                             # the end token is likely: the mask shows

    def lists(ban):
        out = []
        for s in table:
            r = R.truncate(s, 0, 0.9, 0.05, ban=ban)
            cum = np.zeros(V, np.float32)
            cum[:r.K] = r.C
            out.append((r.n, r.tokens, cum))
        return out

    plain, banned = lists(-1), lists(END)
    for seed in (0, 7):
        want = T.walk(lambda r: plain[r], B, V, Tn, seed, END)
        got = R.walk(lambda r: plain[r], lambda r: banned[r], B, V, Tn, 0, seed, END)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert (want[1] < 6).any()
        for m in (6, Tn):
            tok, fe = R.walk(lambda r: plain[r], lambda r: banned[r], B, V, Tn, m, seed, END)
            assert (tok[:, :m] != END).all() and (fe >= m).all()
            if m == Tn:
                assert (fe == Tn).all()
