"""The NumPy restatement of arcvae_dec_sample_draws (tests/draws_ref.py) against the restatement of the existing list walk
(tests/trunc_ref.py), and the properties of the contract that need no GPU: distinct keys, prefix stability in N, the pad mode,
and the first-position pick on a list whose cumulative masses step down by an ulp."""
import numpy as np

import draws_ref as D
import topkp_ref as T
import trunc_ref as R

END = 2


def _lists(V, B, seed, ban=-1):
    """Synthetic materialised lists of B*V table rows: (count [R], tokens [R, V], cum [R, V]) in the kernels' format, from the
    fp64 restatement rounded to fp32 (top_k 12, top_p 0.9)."""
    rs = np.random.RandomState(seed)
    table = (rs.standard_normal((B * V, V)) * 1.5).astype(np.float32)
    table[:, END] += 1.5
    cnt = np.zeros(B * V, np.int32)
    tok = np.zeros((B * V, V), np.int32)
    cum = np.zeros((B * V, V), np.float32)
    for i, s in enumerate(T.scaled(table, 1.0)):
        r = R.truncate(s, 12, 0.9, 0.0, 1.0, ban)
        cnt[i], tok[i] = r.n, r.tokens
        cum[i, :r.K] = r.C.astype(np.float32)
    return lambda r: (cnt[r], tok[r], cum[r])


def test_draw_zero_is_the_existing_walk():
    B, V, Tn = 5, 16, 24
    plain, banned = _lists(V, B, 1), _lists(V, B, 1, ban=END)
    for min_len in (0, 6):
        for seed in (0, 11, 2 ** 64 - 5):
            want_t, want_f = R.walk(plain, banned, B, V, Tn, min_len, seed, END)
            got_t, got_f = D.walk(plain, banned, B, 3, V, Tn, min_len, seed, END)
            np.testing.assert_array_equal(got_t[:, 0, :], want_t)
            np.testing.assert_array_equal(got_f[:, 0], want_f)
            assert (got_t[:, 1, :] != want_t).any()                  # the other draws are other molecules
        if min_len:
            assert (got_t[:, :, :min_len] != END).all() and (got_f >= min_len).all()
    assert all(D.u24(D.draw_key(7, b, 0), t) == T.u24(7, b, t) for b in range(4) for t in range(5))


def test_keys_are_pairwise_distinct():
    for seed in (0, 2 ** 63 + 17):
        keys = {D.draw_key(seed, b, d) for b in range(8) for d in range(4096)}
        assert len(keys) == 8 * 4096


def test_draws_are_a_prefix_of_a_larger_call():
    B, V, Tn = 2, 16, 20
    plain, banned = _lists(V, B, 2), _lists(V, B, 2, ban=END)
    t5, f5 = D.walk(plain, banned, B, 5, V, Tn, 3, 9, END)
    t9, f9 = D.walk(plain, banned, B, 9, V, Tn, 3, 9, END)
    np.testing.assert_array_equal(t5, t9[:, :5])
    np.testing.assert_array_equal(f5, f9[:, :5])


def test_pad_mode_agrees_up_to_the_first_end():
    B, V, Tn, N = 2, 16, 30, 24
    plain, banned = _lists(V, B, 3), _lists(V, B, 3, ban=END)
    t0, f0 = D.walk(plain, banned, B, N, V, Tn, 2, 4, END)
    t7, f7 = D.walk(plain, banned, B, N, V, Tn, 2, 4, END, pad_token=7)
    np.testing.assert_array_equal(f0, f7)
    assert (f0 < Tn - 1).any() and (f0 >= 2).all()
    for b in range(B):
        for d in range(N):
            e = f0[b, d]
            np.testing.assert_array_equal(t7[b, d, :e + 1], t0[b, d, :e + 1])
            assert (t7[b, d, e + 1:] == 7).all()


def test_the_pick_is_the_first_position_not_a_bisection():
    """cum steps down by one ulp at position 4 (a multiple of 4, where the pre-pass scan changes association order).  For a theta
    between the two values the first position above theta is 3; a bisection for the first C_i > theta, which assumes a
    non-decreasing C, probes position 4, finds it not above theta, and answers a later position."""
    c3 = np.float32(0.75)
    c4 = np.nextafter(c3, np.float32(0), dtype=np.float32)               # one ulp below
    cum = np.array([0.125, 0.25, 0.5, c3, c4, 0.8125, 0.875, 0.9375, 1.0], np.float32)
    n = len(cum)
    u = int(round(float(c4) * 2 ** 24))                                  # theta = fl(fl(u * 2^-24) * 1.0) = c4 exactly
    theta = np.float32(np.float32(u) * np.float32(2.0 ** -24)) * cum[n - 1]
    assert theta == c4 and cum[3] > theta and not cum[4] > theta
    assert T.pick(n, cum, u) == 3

    lo, hi = 0, n - 1                                                    # the bisection a monotone C would allow
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if cum[mid] > theta else (mid + 1, hi)
    assert lo == 5
    # and the walk applies exactly that pick: every first token of a replay over this list is T.pick of its own u24
    rows = lambda r: (n, np.arange(n), cum)                              # noqa: E731  (every table row is this list)
    tok, _ = D.walk(rows, rows, 1, 64, n, 1, 0, 0, end_token=n)
    assert [int(x) for x in tok[0, :, 0]] == [T.pick(n, cum, D.u24(D.draw_key(0, 0, d), 0)) for d in range(64)]
