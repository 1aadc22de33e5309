"""lr_schedule.LRSchedule: closed-form values of lr(s), its shape (warmup rises, decay never rises, last value held), that it is
a function of s alone (so a resumed run continues the curve), and every refusal.  No device, no torch.

Exact checks compare with the module's documented expressions written out here; the rest is held to 1e-12 relative."""
import math

import pytest

from lr_schedule import LRSchedule

BASE, W, N, R = 2e-4, 5, 45, 0.1
REL = 1e-12


def _close(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


def _expect(kind, s, base=BASE, w=W, n=N, r=R):
    if s < w:
        return base * (s + 1) / w
    q = min(1.0, (s - w) / max(1, n - w))
    if kind == "constant":
        return base
    if kind == "linear":
        return base * (r + (1.0 - r) * (1.0 - q))
    return base * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q)))


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_closed_form_points(kind):
    sch = LRSchedule(BASE, kind, warmup_steps=W, total_steps=N, min_lr_ratio=R)
    for s in (0, W - 1, W, N, N + 5):
        assert sch.lr(s) == _expect(kind, s), (kind, s)          # the same expressions, exactly
    assert sch.lr(0) == BASE * 1 / W
    assert sch.lr(W - 1) == BASE * W / W == BASE                 # the warmup ends ON the base rate
    assert _close(sch.lr(W), BASE)                               # q = 0: decay starts from the base rate
    last = BASE if kind == "constant" else BASE * R
    assert _close(sch.lr(N), last) and _close(sch.lr(N + 5), last)
    assert sch.lr(N + 5) == sch.lr(N)                            # held beyond N
    assert sch(7) == sch.lr(7)


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_midpoint(kind):
    sch = LRSchedule(BASE, kind, warmup_steps=W, total_steps=N, min_lr_ratio=R)
    mid = W + (N - W) // 2                                       # q = 20 / 40 = 1/2 exactly
    assert (mid - W) / (N - W) == 0.5
    assert _close(sch.lr(mid), BASE * (R + (1.0 - R) / 2))


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_shape(kind):
    sch = LRSchedule(BASE, kind, warmup_steps=W, total_steps=N, min_lr_ratio=R)
    vals = [sch.lr(s) for s in range(N + 10)]
    assert all(b > a for a, b in zip(vals[:W - 1], vals[1:W]))           # warmup rises strictly
    assert all(b <= a for a, b in zip(vals[W - 1:-1], vals[W:]))         # decay never rises
    assert all(0.0 <= v <= BASE for v in vals)
    if kind != "constant":
        assert all(b < a for a, b in zip(vals[W:N], vals[W + 1:N + 1]))  # ... and falls strictly until N


def test_no_warmup_and_short_runs():
    assert LRSchedule(BASE, "constant").lr(0) == BASE and LRSchedule(BASE, "constant").lr(10 ** 9) == BASE
    assert LRSchedule(BASE, "cosine", total_steps=10).lr(0) == BASE * (0.0 + 1.0 * 0.5 * (1.0 + math.cos(0.0)))
    # N <= W: the divisor is max(1, N - W) = 1, the decay is over one step after the warmup
    sch = LRSchedule(BASE, "linear", warmup_steps=4, total_steps=2, min_lr_ratio=0.5)
    assert sch.lr(3) == BASE and sch.lr(4) == BASE * (0.5 + 0.5 * 1.0) and sch.lr(5) == BASE * 0.5 == sch.lr(50)
    assert LRSchedule(0.0, "cosine", 3, 9).lr(1) == 0.0                  # a zero base rate is a valid rate
    assert _close(LRSchedule(BASE, "cosine", 0, 8, 1.0).lr(4), BASE)     # r = 1: no decay


def test_depends_on_s_alone():
    """Evaluation order, repetition and a rebuilt object (a resumed run) give the same numbers."""
    a = LRSchedule(BASE, "cosine", warmup_steps=W, total_steps=N, min_lr_ratio=R)
    fwd = [a.lr(s) for s in range(N + 3)]
    assert [a.lr(s) for s in reversed(range(N + 3))] == fwd[::-1]
    b = LRSchedule.from_state(a.state())
    assert [b.lr(s) for s in range(20, N + 3)] == fwd[20:]
    assert b.state() == a.state() == dict(base_lr=BASE, kind="cosine", warmup_steps=W, total_steps=N, min_lr_ratio=R)
    # total_steps left open and filled in later (the trainer does that) is the same schedule
    c = LRSchedule(BASE, "cosine", warmup_steps=W, min_lr_ratio=R)
    c.set_total_steps(N)
    assert [c.lr(s) for s in range(N + 3)] == fwd


def test_refusals():
    with pytest.raises(ValueError, match="kind"):
        LRSchedule(BASE, "exponential")
    with pytest.raises(ValueError, match="warmup_steps"):
        LRSchedule(BASE, "constant", warmup_steps=-1)
    for r in (-0.01, 1.01, math.nan, math.inf):
        with pytest.raises(ValueError, match="min_lr_ratio"):
            LRSchedule(BASE, "constant", min_lr_ratio=r)
    for base in (-1e-4, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="base_lr"):
            LRSchedule(base, "constant")
    for kind in ("linear", "cosine"):
        open_ended = LRSchedule(BASE, kind, warmup_steps=W)             # may be left open for the trainer to fill in ...
        with pytest.raises(ValueError, match="total_steps"):
            open_ended.lr(0)                                            # ... but has no value until then
        with pytest.raises(ValueError, match="total_steps"):
            open_ended.validate()
    with pytest.raises(ValueError, match="total_steps"):
        LRSchedule(BASE, "linear", total_steps=-3)
    with pytest.raises(ValueError, match="step count"):
        LRSchedule(BASE, "constant").lr(-1)
    assert LRSchedule(BASE, "constant", warmup_steps=W).validate().lr(W) == BASE      # constant needs no total_steps
