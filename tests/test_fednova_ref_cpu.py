"""tests/fednova_ref.py (which the GPU tests hold fh_fednova_rows to, bit for bit) against
hand-worked cases, exact fractions, the FedAvg restatement on inputs where every operation is
exact, and an fp64 evaluation; fedhip.ops.fednova_coefficients against the same fractions.
No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import fednova_ref as nr
from fedhip import ops

F = np.float32


def test_hand_cases_three_coordinates():
    """coef = [1/2, 1/4], tau_eff = 2, g = [1, 2, -1/2]:
       j=0: d = 1, -1    t = 1/2, -1/4   acc = 1/4   out = 1 + 1/2 = 3/2
       j=1: d = 0, 2     t = 0, 1/2      acc = 1/2   out = 2 + 1   = 3
       j=2: d = 1, 0     t = 1/2, 0      acc = 1/2   out = -1/2 + 1 = 1/2"""
    g = np.array([1.0, 2.0, -0.5], dtype=F)
    rows = np.array([[2.0, 2.0, 0.5], [0.0, 4.0, -0.5]], dtype=F)
    coef = [0.5, 0.25]
    acc = np.array([0.25, 0.5, 0.5], dtype=F)
    out = np.array([1.5, 3.0, 0.5], dtype=F)
    assert nr.same_bits(nr.fednova_rows(nr.PARTIAL, rows, coef, g), acc)
    assert nr.same_bits(nr.fednova_rows(nr.STEP, rows, coef, g, 2.0), out)
    assert nr.same_bits(nr.fednova_rows(nr.FINISH, acc[None], None, g, 2.0), out)
    assert nr.same_bits(nr.fednova_rows(nr.FINISH, acc, None, g, 2.0), out)


def test_hand_cases_rounding_and_nan():
    """j=0: x = 1 + 2^-23, g = 1, c = 1, tau = 1/2: acc = 2^-23, s = 2^-24, 1 + 2^-24 is a tie
       and rounds to even: out = 1 (a fused or wider evaluation would differ).
       j=1: x = g = +Inf: d = NaN, stored as 0x7FC00000 whatever NaN the hardware makes.
       j=2: x is a negative NaN with a payload: one NaN out."""
    one_ulp = np.array([0x3F800001], dtype=np.uint32).view(F)[0]
    neg_nan = np.array([0xFFA5A5A5], dtype=np.uint32).view(F)[0]
    g = np.array([1.0, np.inf, 3.0], dtype=F)
    rows = np.array([[one_ulp, np.inf, neg_nan]], dtype=F)
    out = nr.fednova_rows(nr.STEP, rows, [1.0], g, 0.5)
    assert out.view(np.uint32).tolist() == [0x3F800000, 0x7FC00000, 0x7FC00000]
    part = nr.fednova_rows(nr.PARTIAL, rows, [1.0], g)
    assert part.view(np.uint32).tolist() == [0x34000000, 0x7FC00000, 0x7FC00000]
    # denormals are kept: 2^-149 * 1 stays 2^-149
    tiny = np.array([1], dtype=np.uint32).view(F)
    got = nr.fednova_rows(nr.PARTIAL, tiny[None], [1.0], np.zeros(1, dtype=F))
    assert got.view(np.uint32).tolist() == [1]


CASES = [([0.5, 0.25, 0.25], [1, 5, 13]), ([0.1, 0.2, 0.3, 0.4], [131, 7, 3, 566]),
         ([8 / 148, 40 / 148, 100 / 148], [1, 5, 13]), ([1.0], [9])]


@pytest.mark.parametrize("helper", [ops.fednova_coefficients, nr.coefficients])
def test_coefficients_against_fractions(helper):
    for p, a in CASES:
        coef, tau = helper(p, a)
        assert isinstance(tau, float) and all(isinstance(c, float) for c in coef)
        exact_tau = sum(Fraction(pk) * ak for pk, ak in zip(p, a))
        for c, pk, ak in zip(coef, p, a):
            # one correctly rounded double division of the double p_k
            assert c == pk / ak
            assert abs(Fraction(c) - Fraction(pk) / ak) <= Fraction(pk) / ak * Fraction(1, 2 ** 53)
        # a plain sum in the given order: within len(p) roundings of the exact sum
        want = 0.0
        for pk, ak in zip(p, a):
            want = want + pk * ak
        assert tau == want
        assert abs(Fraction(tau) - exact_tau) <= exact_tau * Fraction(2 * len(p), 2 ** 53)
        # an explicit tau_eff replaces the weighted one and leaves the coefficients alone
        coef2, tau2 = helper(p, a, tau_eff=3)
        assert coef2 == coef and tau2 == 3.0 and isinstance(tau2, float)
    # numpy scalars and integers as they come out of a partition
    coef, tau = helper(np.array([0.5, 0.5], dtype=np.float64), np.array([2, 4]))
    assert coef == [0.25, 0.125] and tau == 3.0


@pytest.mark.parametrize("helper", [ops.fednova_coefficients, nr.coefficients])
def test_coefficients_empty_shard(helper):
    """a_k == 0 with p_k == 0 (the empty shard of D17): coefficient 0, nothing added to tau."""
    coef, tau = helper([0.25, 0.0, 0.75], [4, 0, 8])
    assert coef == [0.0625, 0.0, 0.09375] and tau == 7.0
    coef, tau = helper([0.0, 1.0], [0, 3])
    assert coef == [0.0, 1.0 / 3] and tau == 3.0


@pytest.mark.parametrize("helper", [ops.fednova_coefficients, nr.coefficients])
def test_coefficients_refusals(helper):
    for args, kw in ((([0.5, 0.5], [1, 0]), {}),          # no step but a weight
                     (([0.5, 0.5], [1, -2]), {}),         # negative steps
                     (([0.5, 0.5], [1, 2.5]), {}),        # not an integer
                     (([0.5, 0.5], [1]), {}),             # lengths
                     (([0.5], [1, 2]), {}),
                     (([1.0], [1]), {"tau_eff": "mean"}),
                     (([1.0], [1]), {"tau_eff": 0}),
                     (([1.0], [1]), {"tau_eff": -1.0}),
                     (([1.0], [1]), {"tau_eff": float("inf")}),
                     (([1.0], [1]), {"tau_eff": float("nan")}),
                     (([1.0], [1]), {"tau_eff": True})):
        with pytest.raises(ValueError):
            helper(*args, **kw)


def test_exact_identity_with_fedavg():
    """Small-integer rows and global, power-of-two weights, equal power-of-two a_k: every
    operation is exact, so FedNova IS FedAvg, bit for bit."""
    rng = np.random.default_rng(3)
    for w, a in (([0.25] * 4, 4), ([0.5, 0.25, 0.125, 0.125], 8), ([1.0], 2),
                 ([0.5, 0.5], 1)):
        C, P = len(w), 257
        rows = rng.integers(-64, 65, (C, P)).astype(F)
        g = rng.integers(-64, 65, P).astype(F)
        coef, tau = nr.coefficients(w, [a] * C)
        assert tau == float(a) and all(c == wk / a for c, wk in zip(coef, w))
        want = nr.weighted_sum(rows, w)
        assert nr.same_bits(nr.fednova_rows(nr.STEP, rows, coef, g, tau), want)
        part = nr.fednova_rows(nr.PARTIAL, rows, coef, g)
        assert nr.same_bits(nr.fednova_rows(nr.FINISH, part, None, g, tau), want)


@pytest.mark.parametrize("C", [1, 2, 5, 33])
def test_fp64_bound(C):
    """Against an fp64 evaluation with the already-rounded fp32 c_k and tau_eff.  Every input
    term passes through at most C+3 roundings on its way to out[j] (its subtract, its multiply,
    at most C-1 inexact adds, the tau multiply, the final add), each of relative size 2^-24,
    and |x - g| <= |x| + |g|; 1.01 covers the second-order terms of (1 + 2^-24)^(C+3)."""
    rng = np.random.default_rng(40 + C)
    P = 4001
    g = rng.standard_normal(P).astype(F)
    rows = (g + rng.standard_normal((C, P)) * 10.0 ** rng.uniform(-3, 1, (C, 1))).astype(F)
    p = rng.random(C) + 0.05
    p = (p / p.sum()).tolist()
    a = rng.integers(1, 600, C).tolist()
    coef, tau = nr.coefficients(p, a)
    c32, tau32 = np.asarray(coef, dtype=F), F(tau)
    got = nr.fednova_rows(nr.STEP, rows, c32, g, tau32).astype(np.float64)
    g64, r64, c64, t64 = g.astype(np.float64), rows.astype(np.float64), \
        c32.astype(np.float64), float(tau32)
    want = g64 + t64 * (c64[:, None] * (r64 - g64)).sum(0)
    bound = 1.01 * (C + 3) * 2.0 ** -24 * (
        np.abs(g64) + t64 * (np.abs(c64)[:, None] * (np.abs(r64) + np.abs(g64))).sum(0))
    err = np.abs(got - want)
    print(f"C={C}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
