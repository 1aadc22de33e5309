"""The NumPy restatement of top-k / nucleus sampling (tests/topkp_ref.py) against brute-force enumeration of its sets and against
the published splitmix64 sequence (CPU only: the restatement is what the GPU tests hold the kernels to)."""
import numpy as np
import pytest

import topkp_ref as R


def test_mix64_is_splitmix64():
    # splitmix64 seeded with 0: its state advances by the golden gamma before each finalisation
    assert R.mix64(0) == 0xE220A8397B1DCDAF
    assert R.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert R.mix64(R.M64) < 1 << 64
    u = [R.u24(7, b, t) for b in range(4) for t in range(64)]
    assert all(0 <= x < 1 << 24 for x in u) and len(set(u)) == len(u)
    assert R.u24(7, 0, 0) == R.mix64(R.mix64(7)) >> 40
    assert R.u24(-1, 1, 0) == R.mix64(R.mix64(R.M64 ^ (1 << 32))) >> 40      # seeds are taken modulo 2^64


def _tables(V, rs):
    """random, quantised (ties everywhere), one dominant token, flat, and duplicated values at the k = 5 boundary"""
    rnd = rs.standard_normal((6, V)).astype(np.float32) * 2
    q = np.round(rnd * 2) / 2
    dom = rnd.copy()
    dom[:, rs.randint(V)] += 30
    flat = np.zeros((1, V), np.float32)
    dup = rnd.copy()
    for r in dup:
        o = R.order(r)
        if V > 6:
            r[o[5]] = r[o[4]]                            # tokens 5th and 6th in the order tie
            r[o[6]] = r[o[4]]
    return np.concatenate([rnd, q, dom, flat, dup]).astype(np.float32)


@pytest.mark.parametrize("V", [3, 12, 80, 256])
def test_sets_match_brute_force(V):
    rs = np.random.RandomState(V)
    tab = _tables(V, rs)
    ks = sorted({1, 2, 5, max(V - 1, 1), V, V + 7, 0})
    ps = [1e-6, 0.5, 0.9, 0.999, 1.0]
    checked = 0
    for temp in (1.0, 0.7):
        S = R.scaled(tab, temp)
        for s in (S if V <= 80 else S[::3]):
            for k in ks if V <= 80 else (1, 5, V - 1, 0):
                for p in ps:
                    o, K, e, C, n, before, thr = R.truncate(s, k, p)
                    Kset, P = R.brute_force_sets(s, k, p)
                    assert set(o[:K].tolist()) == Kset
                    assert 1 <= n <= K
                    if R.is_boundary(before, thr, 1e-12):
                        continue                          # (fp64 C - e against a direct sum: either side of the threshold)
                    assert set(o[:n].tolist()) == P, (k, p)
                    checked += 1
    assert checked > 0


def test_order_is_total_with_ties_to_the_lower_token():
    s = np.array([1.0, 3.0, 3.0, -0.0, 0.0, 3.0], np.float32)
    assert R.order(s).tolist() == [1, 2, 5, 0, 3, 4]
    o, K, e, C, n, _, _ = R.truncate(s, 2, 1.0)
    assert o[:K].tolist() == [1, 2] and n == 2


def test_limits():
    rs = np.random.RandomState(3)
    s = R.scaled(rs.standard_normal(80).astype(np.float32), 1.0)
    assert R.truncate(s, 1, 1.0)[4] == 1
    assert R.truncate(s, 0, 1e-9)[4] == 1
    assert R.truncate(s, 0, 1.0)[4] == 80
    assert R.truncate(s, 200, 1.0)[1] == 80
    p = R.truncated_probs(rs.standard_normal(80), 0.5, 5, 1.0)
    assert np.count_nonzero(p) == 5 and abs(p.sum() - 1) < 1e-12


def test_walk_replay_draws_the_truncated_distribution():
    """The walk's decision rule on exact cumulative masses draws position i with probability (C_i - C_{i-1}) / C_{n-1}: the
    first-step histogram of many rows over one materialised row matches the truncated distribution."""
    V, B = 6, 20000
    x = np.array([2.0, 1.0, 0.5, 0.25, -1.0, 0.0], np.float32)
    s = R.scaled(x, 1.0)
    o, K, e, C, n, _, _ = R.truncate(s, 4, 0.9)
    tok = np.zeros(V, np.int32)
    tok[:] = o
    cum = np.zeros(V, np.float32)
    cum[:K] = C
    first = np.array([tok[R.pick(n, cum, R.u24(5, b, 0))] for b in range(B)])
    want = np.zeros(V)
    want[o[:n]] = e[:n] / e[:n].sum()
    got = np.bincount(first, minlength=V) / B
    assert set(np.flatnonzero(got)) <= set(o[:n].tolist())
    assert 0.5 * np.abs(got - want).sum() < 0.02
    toks, fe = R.walk(lambda r: (n, tok, cum), 3, V, 10, 5)
    assert toks.shape == (3, 10) and set(np.unique(toks)) <= set(o[:n].tolist())
