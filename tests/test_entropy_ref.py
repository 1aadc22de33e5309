"""The closed forms of the exact expectations (tests/entropy_ref.py; include/arcvae_hip.h arcvae_dec_row_costs /
arcvae_dec_chain_expect) against the enumeration of every outcome, on the CPU in fp64, and the two entry points' declarations."""
import os
import re

import numpy as np
import pytest

import beam_ref as R
import entropy_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(V, B, seed, temp_p, temp_q):
    rs = np.random.RandomState(seed)
    tp = rs.standard_normal((B * V, V)) * 2.0
    tq = rs.standard_normal((B * V, V)) * 2.0
    lp_p = R.step_terms(tp, R.row_lse(tp, temp_p), temp_p, dtype=np.float64)
    lp_q = R.step_terms(tq, R.row_lse(tq, temp_q), temp_q, dtype=np.float64)
    return lp_p, lp_q


@pytest.mark.parametrize("V,T,end", [(5, 5, 2), (4, 6, 0), (3, 1, 1)])
def test_recursion_equals_enumeration(V, T, end):
    """Two random tables at different temperatures, fp64 step terms: the rows are normalised to fp64 rounding, so the chain-rule
    totals and the enumeration agree to 1e-12."""
    B = 2
    lp_p, lp_q = _tables(V, B, 100 * V + T, 0.8, 1.3)
    rec = N.expectations(lp_p, lp_q, B, V, T, end)
    enu = N.enumerate_outcomes(lp_p, lp_q, B, V, T, end)
    tol = 1e-12
    assert np.all(np.abs(enu["mass"] - 1.0) <= tol)
    assert np.all(np.abs(rec["H"] - enu["H"]) <= tol), np.abs(rec["H"] - enu["H"]).max()
    assert np.all(np.abs(rec["CE"] - enu["CE"]) <= tol), np.abs(rec["CE"] - enu["CE"]).max()
    assert np.all(rec["CE"] - rec["H"] >= 0.0) and np.all(enu["CE"] - enu["H"] >= 0.0)        # KL >= 0
    assert np.all(rec["CE"] - rec["H"] > 1e-3)                                               # (and these tables do differ)
    assert np.all(np.abs(rec["visits"].sum(axis=1) - enu["length"]) <= tol)
    assert np.all(np.abs(rec["visits"] - enu["visits"]) <= tol)
    assert np.all(np.abs(rec["open_mass"] - enu["open_mass"]) <= tol)
    assert np.all(np.abs(rec["open_mass"] + rec["visits"][:, end] - 1.0) <= tol)
    assert np.all(rec["A_H"] >= np.abs(rec["H"])) and np.all(rec["A_CE"] >= np.abs(rec["CE"]))
    assert np.all(rec["H"] > 0.0) and np.all(enu["length"] >= 1.0 - tol) and np.all(enu["length"] <= T + tol)
    same = N.expectations(lp_p, lp_p, B, V, T, end)
    np.testing.assert_array_equal(same["CE"], same["H"])                                     # Q = P: KL exactly 0


def test_zero_probability_terms_contribute_nothing():
    """p = 0 with a logarithm of -inf: the guarded product, not 0 * inf."""
    V, T, end = 3, 3, 2
    p = np.array([[0.5, 0.0, 0.5], [0.25, 0.25, 0.5], [1.0, 0.0, 0.0]])
    with np.errstate(divide="ignore"):
        lp = np.log(p)
    rec = N.expectations(lp, lp, 1, V, T, end)
    enu = N.enumerate_outcomes(lp, lp, 1, V, T, end)
    assert np.all(np.isfinite(rec["H"])) and np.all(np.abs(rec["H"] - enu["H"]) <= 1e-12)
    assert np.all(np.abs(rec["visits"] - enu["visits"]) <= 1e-12) and rec["visits"][0, 1] == 0.0


def test_entry_points_are_declared_with_the_binding_arity():
    from arcvae_hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arcvae_hip.h")).read(), flags=re.S)
    for name in ("arcvae_dec_row_costs", "arcvae_dec_chain_expect"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/arcvae_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name])
