"""The weight EMA's NumPy restatement (tests/ema_ref.py) against the fp64 recursion, and the decay warm-up (CPU).

Bound: after k updates the fp32 restatement is within k * 2^-23 * M of the fp64 recursion on the same fp32 omd, M the largest
|p| or |e| seen.  Derived, not measured: an update makes three roundings -- fl(p - e), fl(omd * .), fl(e + .) -- each at most
2^-24 relative of a quantity bounded by M (|p - e| <= M where the average follows the weights, as on these walks; omd <= 1; the
result lies between e and p), so an update adds at most 3 * 2^-24 * M < 2^-23 * M, and the error carried over from the earlier
updates is multiplied by 1 - omd <= 1."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ema_ref as R

N = 100_003


@pytest.mark.parametrize("decay,warmup,k", [(0.9, True, 6), (0.999, True, 200), (0.9999, False, 500), (0.5, False, 50)])
def test_fp32_restatement_stays_within_the_derived_bound(decay, warmup, k):
    rs = np.random.RandomState(11)
    p = rs.standard_normal(N).astype(np.float32)
    e32 = p.copy()
    e64 = p.astype(np.float64)
    M = float(np.abs(p).max())
    for t in range(k):
        p = (p + 0.01 * rs.standard_normal(N)).astype(np.float32)       # a random walk of the weights
        omd = R.omd32(1.0 - R.decay_at(decay, warmup, t))
        e32 = R.update32(e32, p, omd)
        e64 = R.update64(e64, p, omd)
        M = max(M, float(np.abs(p).max()), float(np.abs(e32).max()), float(np.abs(e64).max()))
    assert e32.dtype == np.float32
    err = float(np.abs(e32.astype(np.float64) - e64).max())
    bound = k * 2.0 ** -23 * M
    print(f"decay {decay} warmup {warmup} k {k}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_equal_inputs_are_an_exact_fixed_point():
    rs = np.random.RandomState(5)
    p = rs.standard_normal(4099).astype(np.float32)
    p[:3] = (0.0, np.float32(1e-42), np.float32(3e38))      # zero, a denormal, near the largest finite value
    for omd in (0.1, 1e-4, 1.0):
        assert np.array_equal(R.update32(p, p, omd).view(np.uint32), p.view(np.uint32))


def test_full_weight_copies_the_parameters():
    rs = np.random.RandomState(6)
    e, p = rs.standard_normal(1000).astype(np.float32), rs.standard_normal(1000).astype(np.float32)
    # omd = 1: e + (p - e), within one ulp of max(|e|, |p|) of p (not bitwise: the subtraction rounds)
    assert np.abs(R.update32(e, p, 1.0) - p).max() <= 2.0 ** -23 * max(np.abs(e).max(), np.abs(p).max())


def test_one_minus_decay_is_formed_in_double():
    """Why the ABI takes 1 - decay: formed in fp32 it is off by 1.7e-4 relative at decay 0.9999."""
    good = float(R.omd32(1.0 - 0.9999))
    bad = float(np.float32(1.0) - np.float32(0.9999))
    assert abs(good - 1e-4) / 1e-4 < 2.0 ** -24
    assert abs(bad - 1e-4) / 1e-4 > 1e-4


def test_warmup_schedule():
    assert R.decay_at(0.9, True, 0) == 0.1
    assert R.decay_at(0.9, False, 0) == 0.9 and R.decay_at(0.9, False, 10 ** 6) == 0.9
    for decay in (0.5, 0.9, 0.999, 0.9999):
        d = Fraction(str(decay))
        first = math.ceil((10 * d - 1) / (1 - d))                        # the first t with (1 + t) / (10 + t) >= decay, exactly
        seq = [R.decay_at(decay, True, t) for t in range(first + 50)]
        assert all(b >= a for a, b in zip(seq, seq[1:]))                 # non-decreasing
        reached = next(t for t, d in enumerate(seq) if d == decay)
        assert reached == first, (decay, reached, first)
        assert all(d < decay for d in seq[:first]) and all(d == decay for d in seq[first:])
    assert next(t for t in range(200) if R.decay_at(0.9, True, t) == 0.9) == 80


def test_module_schedule_matches_the_restatement():
    from arcvae_hip.ema import WeightEMA
    for decay, warm in ((0.9, True), (0.999, True), (0.9999, False)):
        ema = WeightEMA({}, decay, warmup=warm)
        assert ema.num_updates == 0
        for t in (0, 1, 5, 79, 80, 81, 10_000):
            assert ema.decay_at(t) == R.decay_at(decay, warm, t)
