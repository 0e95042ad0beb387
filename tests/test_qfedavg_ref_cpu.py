"""tests/qfedavg_ref.py (which the GPU tests hold fh_qfedavg_rows to) against the FedAvg
restatement on inputs where every operation is exact, hand-worked cases checked with exact
fractions on the paper's unsimplified Algorithm 2, and the edges of the coefficients;
fedhip.ops.qfedavg_coefficients against the reference copy.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import fednova_ref as nr
import qfedavg_ref as qr
from fedhip import ops

F = np.float32
D = np.float64


def test_q0_with_sample_weights_is_fedavg_bit_for_bit():
    """Small-integer rows and global, power-of-two weights that sum to 1: a = w, b = 0, den = 1,
    every operation is exact, so q-FedAvg with q = 0 IS FedAvg, bit for bit."""
    rng = np.random.default_rng(5)
    for w in ([0.25] * 4, [0.5, 0.25, 0.125, 0.125], [1.0], [0.5, 0.5]):
        C, P = len(w), 257
        rows = rng.integers(-64, 65, (C, P)).astype(F)
        g = rng.integers(-64, 65, P).astype(F)
        a, b = qr.coefficients(w, rng.random(C).tolist(), 0, 3.0)
        assert a == w and b == [0.0] * C
        want = nr.weighted_sum(rows, w)
        out, sq, den = qr.qfedavg_rows(qr.STEP, rows, a, b, g)
        assert den == 1.0 and qr.same_bits(out, want)
        assert sq.tolist() == [float(((r - g).astype(D) ** 2).sum()) for r in rows]
        part, _, den_p = qr.qfedavg_rows(qr.PARTIAL, rows, a, b, g)
        assert den_p == 1.0
        assert qr.same_bits(qr.qfedavg_rows(qr.FINISH, part, None, None, g, den=den_p)[0], want)


def algorithm2(pi, Fk, q, L, rows, g):
    """Li et al., Algorithm 2, unsimplified, in exact fractions (pi_k weighs both sums):
       dw_k = L * (g - x_k);  Delta_k = pi_k * F_k^q * dw_k;
       h_k = pi_k * (q * F_k^(q-1) * ||dw_k||^2 + L * F_k^q);  g_new = g - sum Delta / sum h."""
    fr = lambda v: [Fraction(float(x)) for x in v]
    g = fr(g)
    num, hs = [Fraction(0)] * len(g), Fraction(0)
    for p, f, x in zip(pi, Fk, rows):
        p, f, L_ = Fraction(p), Fraction(f), Fraction(L)
        dw = [L_ * (gj - xj) for gj, xj in zip(g, fr(x))]
        num = [n + p * f ** q * d for n, d in zip(num, dw)]
        hs += p * (q * f ** (q - 1) * sum(d * d for d in dw) + L_ * f ** q)
    return [gj - n / hs for gj, n in zip(g, num)], hs


HAND = [
    # q, L, F, a, b, rows, den, out          pi = [1/2, 1/2], g = [1, 2, -1]
    # q = 1: a = pi*F = [1/2, 3/2], b = pi*L = [1, 1]; d0 = [1,0,1] (2), d1 = [0,2,0] (4);
    #        den = (1*2 + 1/2) + (1*4 + 3/2) = 8; acc = [1/2, 3, 1/2]; out = g + acc/8
    (1, 2.0, [1.0, 3.0], [0.5, 1.5], [1.0, 1.0], [[2.0, 2.0, 0.0], [1.0, 4.0, -1.0]], 8.0,
     [1.0625, 2.375, -0.9375]),
    # q = 2: a = pi*F^2 = [1/2, 9/2], b = pi*2*L*F = [1, 3]; d0 = [1,0,1] (2), d1 = [1,1,1] (3);
    #        den = (1*2 + 1/2) + (3*3 + 9/2) = 16; acc = [5, 9/2, 5]; out = g + acc/16
    (2, 1.0, [1.0, 3.0], [0.5, 4.5], [1.0, 3.0], [[2.0, 2.0, 0.0], [2.0, 3.0, 0.0]], 16.0,
     [1.3125, 2.28125, -0.6875]),
]


@pytest.mark.parametrize("q,L,Fk,a,b,rows,den,out", HAND)
def test_hand_cases_against_algorithm_2(q, L, Fk, a, b, rows, den, out):
    pi = [0.5, 0.5]
    g = np.array([1.0, 2.0, -1.0], dtype=F)
    rows = np.array(rows, dtype=F)
    # the coefficients of the rule as fractions, from the losses themselves (no guard)
    assert [Fraction(p) * Fraction(f) ** q for p, f in zip(pi, Fk)] == [Fraction(x) for x in a]
    assert [Fraction(p) * q * Fraction(L) * Fraction(f) ** (q - 1) for p, f in zip(pi, Fk)] \
        == [Fraction(x) for x in b]
    want, hs = algorithm2(pi, Fk, q, L, rows, g)
    assert hs == Fraction(L) * Fraction(den)  # one L cancels against the numerator's
    assert want == [Fraction(x) for x in out]
    got, sq, got_den = qr.qfedavg_rows(qr.STEP, rows, a, b, g)
    assert got_den == den and qr.same_bits(got, np.array(out, dtype=F))
    part, sq2, den2 = qr.qfedavg_rows(qr.PARTIAL, rows, a, b, g)
    assert den2 == den and sq.tolist() == sq2.tolist()
    assert qr.same_bits(qr.qfedavg_rows(qr.FINISH, part, None, None, g, den=den2)[0], got)
    # the helpers, which add the authors' guard 1e-10 to the loss: within the roundings of a
    # double power and two or three double products (pow is not required to round correctly)
    for helper in (ops.qfedavg_coefficients, qr.coefficients):
        ha, hb = helper(pi, Fk, q, L)
        for k in range(2):
            f = Fraction(Fk[k] + 1e-10)
            ea = Fraction(pi[k]) * f ** q
            eb = Fraction(pi[k]) * q * Fraction(L) * f ** (q - 1)
            assert abs(Fraction(ha[k]) - ea) <= ea * Fraction(8, 2 ** 53)
            assert abs(Fraction(hb[k]) - eb) <= eb * Fraction(8, 2 ** 53)


def test_rounding_skip_and_nan():
    """j=0: x = 1 + 2^-23, g = 1, a = 1, den = 2: acc = 2^-23, s = 2^-24, 1 + 2^-24 is a tie and
    rounds to even: out = 1 (a fused or wider evaluation would differ).
    j=1: x = g = +Inf in the live row: d = NaN, stored as 0x7FC00000.
    Row 1 has a = -0: it is skipped although it holds NaN and Inf; its sqdist is NaN."""
    one_ulp = np.array([0x3F800001], dtype=np.uint32).view(F)[0]
    g = np.array([1.0, np.inf, 3.0], dtype=F)
    rows = np.array([[one_ulp, np.inf, 3.0], [np.nan, 1.0, np.inf]], dtype=F)
    a, b = [1.0, -0.0], [0.0, 5.0]
    part, sq, den = qr.qfedavg_rows(qr.PARTIAL, rows, a, b, g)
    assert part.view(np.uint32).tolist() == [0x34000000, 0x7FC00000, 0]
    assert math.isnan(sq[0]) and math.isnan(sq[1]) and math.isnan(den)  # b0 * NaN
    out = qr.finish(part, g, 2.0)
    assert out.view(np.uint32).tolist() == [0x3F800000, 0x7FC00000, 0x40400000]
    # denormals are kept: 2^-149 * 1 stays 2^-149
    tiny = np.array([1], dtype=np.uint32).view(F)
    got = qr.qfedavg_rows(qr.PARTIAL, tiny[None], [1.0], [0.0], np.zeros(1, dtype=F))[0]
    assert got.view(np.uint32).tolist() == [1]
    assert qr.denominator([0.0, -0.0], [1.0, 1.0], [np.nan, 3.0]) == (0.0, 0)


@pytest.mark.parametrize("den", [0.0, -0.0, -3.0, np.inf, -np.inf, np.nan, 1e46])
def test_bad_denominator_leaves_global(den):
    """den <= 0, a non-finite den, or one whose fp32 inverse is zero: out == g bitwise, also where
    g or acc hold NaN payloads (nothing is multiplied)."""
    g = np.array([0x3F800000, 0xFFA5A5A5, 0x00000001, 0x80000000], dtype=np.uint32).view(F)
    acc = np.array([1.0, 2.0, np.nan, np.inf], dtype=F)
    assert qr.inverse(den) == 0 and not np.signbit(qr.inverse(den))
    assert qr.same_bits(qr.finish(acc, g, den), g)
    assert qr.same_bits(qr.qfedavg_rows(qr.FINISH, acc, None, None, g, den=den)[0], g)


@pytest.mark.parametrize("helper", [ops.qfedavg_coefficients, qr.coefficients])
def test_coefficient_edges(helper):
    # a NaN, negative or infinite loss, or a weight that is not > 0: not live
    a, b = helper([0.2] * 4 + [0.0, -0.1], [1.0, float("nan"), -0.5, float("inf"), 1.0, 1.0],
                  1.5, 2.0)
    assert a[0] > 0 and b[0] > 0
    assert a[1:] == [0.0] * 5 and b[1:] == [0.0] * 5
    # loss 0 with q < 1 stays finite through the guard: F^(q-1) = (1e-10)^(-1/2) = 1e5
    a, b = helper([0.5, 0.5], [0.0, 1.0], 0.5, 1.0)
    assert all(math.isfinite(v) and v > 0 for v in a + b)
    assert a[0] == 0.5 * 1e-10 ** 0.5 and b[0] == ((0.5 * 0.5) * 1.0) * 1e-10 ** (-0.5)
    # q = 0 never evaluates F^(-1)
    assert helper([0.25, 0.75], [0.0, 0.0], 0, 7.0) == ([0.25, 0.75], [0.0, 0.0])
    assert helper([0.25, 0.75], [0.0, 0.0], 0.0, 7.0) == ([0.25, 0.75], [0.0, 0.0])
    # a higher loss gives a strictly larger a_k / pi_k for q > 0
    for q in (0.1, 1, 2, 5.5):
        losses = [0.0, 1e-3, 0.5, 0.5000001, 2.0, 40.0]
        pi = [0.3, 0.1, 0.2, 0.05, 0.25, 0.1]
        a, _ = helper(pi, losses, q, 1.0)
        ratio = [ak / pk for ak, pk in zip(a, pi)]
        assert all(x < y for x, y in zip(ratio, ratio[1:])), (q, ratio)
    # numpy scalars as they come out of a partition
    a, b = helper(np.array([0.5, 0.5]), np.array([2.0, 4.0], dtype=F), np.float64(1.0) * 1, 2)
    assert a == [0.5 * (2.0 + 1e-10), 0.5 * (4.0 + 1e-10)] and b == [1.0, 1.0]


@pytest.mark.parametrize("helper", [ops.qfedavg_coefficients, qr.coefficients])
def test_coefficient_refusals(helper):
    for args in (([0.5, 0.5], [1.0], 1, 1.0),                    # lengths
                 ([0.5], [1.0, 2.0], 1, 1.0),
                 ([1.0], [1.0], -1, 1.0),                        # q
                 ([1.0], [1.0], float("nan"), 1.0),
                 ([1.0], [1.0], float("inf"), 1.0),
                 ([1.0], [1.0], True, 1.0),
                 ([1.0], [1.0], 1, 0.0),                         # lipschitz
                 ([1.0], [1.0], 1, -2.0),
                 ([1.0], [1.0], 1, float("inf")),
                 ([1.0], [1.0], 1, float("nan")),
                 ([1.0], [1.0], 1, None),
                 ([float("inf")], [1.0], 1, 1.0),                # weight
                 ([0.5, 0.5], [float("nan"), -1.0], 1, 1.0),     # no live client
                 ([0.0, 0.0], [1.0, 1.0], 0, 1.0)):
        with pytest.raises(ValueError):
            helper(*args)
    # a rank of several may hold no live client
    assert helper([0.0, 0.5], [1.0, float("nan")], 1, 1.0, require_live=False) \
        == ([0.0, 0.0], [0.0, 0.0])


def test_ops_coefficients_equal_the_reference_copy():
    """A few hundred random draws, edge losses and weights mixed in: the same doubles."""
    rng = np.random.default_rng(11)
    edge_loss = [0.0, float("nan"), -1.0, float("inf"), 1e-12, 1e3]
    for trial in range(300):
        C = int(rng.integers(1, 9))
        w = rng.random(C)
        if trial % 3 == 0:
            w[rng.integers(0, C)] = 0.0
        w = (w / max(w.sum(), 1e-9)).tolist()
        losses = (rng.random(C) * 10.0 ** rng.uniform(-4, 2)).tolist()
        if trial % 4 == 0:
            losses[int(rng.integers(0, C))] = edge_loss[trial // 4 % len(edge_loss)]
        q = [0, 0.0, 0.5, 1, 2, 5.0, float(rng.uniform(0, 6))][trial % 7]
        L = float(10.0 ** rng.uniform(-2, 3))
        try:
            want = qr.coefficients(w, losses, q, L)
        except ValueError:
            with pytest.raises(ValueError):
                ops.qfedavg_coefficients(w, losses, q, L)
            continue
        got = ops.qfedavg_coefficients(w, losses, q, L)
        assert got == want
        assert all(isinstance(v, float) for v in got[0] + got[1])
