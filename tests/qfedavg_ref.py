"""Plain numpy reference for q-FedAvg (csrc/qfedavg.hip); no GPU.

qfedavg_rows is the definition of fh_qfedavg_rows (include/fedhip.h) on fp32 arrays, one rounded
operation per line, vectorised over the coordinates: numpy's float32 / float64 +, - and * are the
IEEE correctly rounded ones and keep denormals.  A NaN result of an arithmetic operation is
stored as the one quiet NaN 0x7FC00000.  sqdist sums fp64 squares of fp32 differences with
np.sum (pairwise): the kernel's order differs, so the GPU tests compare sqdist and den to a
summation-order tolerance and everything else bit for bit.  coefficients is a
pure-Python copy of fedhip.ops.qfedavg_coefficients.

tests/test_qfedavg_ref_cpu.py pins all of it against hand-worked cases and exact fractions.
"""
import math

import numpy as np

from robust_ref import QNAN_BITS, same_bits  # noqa: F401  (same_bits: re-exported)

STEP, PARTIAL, FINISH = range(3)
F = np.float32
D = np.float64
LOSS_GUARD = 1e-10


def canon(x):
    x = np.array(x, dtype=F)
    x.view(np.uint32)[np.isnan(x)] = QNAN_BITS
    return x


def weighted_delta_sum(rows, a, g):
    """acc = (((+0 + a0*(x0 - g)) + a1*(x1 - g)) + ...) over the k with a_k != 0, canonicalised."""
    rows, g = np.asarray(rows, dtype=F), np.asarray(g, dtype=F)
    a = np.asarray(a, dtype=F)
    assert rows.ndim == 2 and rows.shape[0] == a.shape[0] >= 1
    acc = np.zeros(g.shape[0], dtype=F)
    with np.errstate(all="ignore"):
        for x, c in zip(rows, a):
            if c == 0:  # +0 or -0: the row is skipped, whatever it holds
                continue
            d = x - g
            t = c * d
            acc = acc + t
            assert d.dtype == F and t.dtype == F and acc.dtype == F
    return canon(acc)


def sqdist(rows, g):
    """fp64 [C]: sum_j (double)fl32(x_kj - g_j)^2 for every k."""
    rows, g = np.asarray(rows, dtype=F), np.asarray(g, dtype=F)
    with np.errstate(all="ignore"):
        d = rows - g[None, :]
        assert d.dtype == F
        d = d.astype(D)
        return (d * d).sum(axis=1, dtype=D)


def denominator(a, b, sq):
    """(den, live): den = ((h_0 + h_1) + ...), h_k = a_k != 0 ? b_k * sq_k + (double)a_k : 0,
    all fp64, every operation on its own."""
    a = np.asarray(a, dtype=F)
    b, sq = np.asarray(b, dtype=D), np.asarray(sq, dtype=D)
    den, live = None, 0
    with np.errstate(all="ignore"):
        for ak, bk, sk in zip(a, b, sq):
            h = D(0.0)
            if ak != 0:
                m = bk * sk
                h = m + D(ak)
                live += 1
            den = h if den is None else den + h
    return D(den), live


def inverse(den):
    """fl32(1.0 / den) for a finite den > 0, else +0."""
    den = D(den)
    if not (np.isfinite(den) and den > 0):
        return F(0.0)
    with np.errstate(all="ignore"):
        return F(D(1.0) / den)


def finish(acc, g, den):
    """out = g + fl32(1/den) * acc; out = g, bit for bit, when the inverse is zero."""
    acc, g = np.asarray(acc, dtype=F), np.asarray(g, dtype=F)
    inv = inverse(den)
    if inv == 0:
        return g.copy()
    with np.errstate(all="ignore"):
        s = inv * acc
        out = g + s
        assert s.dtype == F and out.dtype == F
    return canon(out)


def qfedavg_rows(mode, rows, a, b, g, den=None):
    """(out fp32 [P], sqdist fp64 [C] or None, den).  STEP / PARTIAL: rows [C, P], a [C] (rounded
    to fp32 here), b [C] fp64.  FINISH: rows [1, P] (or [P]) is the sum itself, den is given."""
    g = np.asarray(g, dtype=F)
    if mode == FINISH:
        acc = np.asarray(rows, dtype=F).reshape(-1, g.shape[0])
        assert acc.shape[0] == 1 and den is not None
        return finish(acc[0], g, den), None, D(den)
    acc = weighted_delta_sum(rows, a, g)
    sq = sqdist(rows, g)
    den, _ = denominator(a, b, sq)
    if mode == PARTIAL:
        return acc, sq, den
    return finish(acc, g, den), sq, den


def coefficients(weights, losses, q, lipschitz, require_live=True):
    """(a, b) in Python double: F = loss + 1e-10, a_k = pi_k * F^q, b_k = pi_k * q * L * F^(q-1);
    a client whose weight is not > 0 or whose loss is negative or not finite gets a = b = 0;
    q == 0 gives a = pi, b = 0.  ValueError for bad arguments or no live client."""
    p = [float(w) for w in weights]
    loss = [float(x) for x in losses]
    if len(p) != len(loss):
        raise ValueError("lengths differ")
    for v, lo_ok in ((q, True), (lipschitz, False)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) \
                or v < 0 or (v == 0 and not lo_ok):
            raise ValueError(f"bad q or lipschitz {v!r}")
    q, L = float(q), float(lipschitz)
    a, b, live = [], [], 0
    for pk, lk in zip(p, loss):
        if math.isinf(pk):
            raise ValueError("infinite weight")
        if not (pk > 0.0 and math.isfinite(lk) and lk >= 0.0):
            a.append(0.0)
            b.append(0.0)
            continue
        live += 1
        if q == 0.0:
            a.append(pk)
            b.append(0.0)
            continue
        Fk = lk + LOSS_GUARD
        try:
            a.append(pk * Fk ** q)
            b.append(((pk * q) * L) * Fk ** (q - 1.0))
        except OverflowError as e:
            raise ValueError("overflow") from e
    if not live and require_live:
        raise ValueError("no live client")
    return a, b


def rule_fp64(rows, a, b, g):
    """The rule evaluated in fp64 throughout from the fp32 inputs (a tolerance reference)."""
    r64, g64 = np.asarray(rows, dtype=F).astype(D), np.asarray(g, dtype=F).astype(D)
    a64, b64 = np.asarray(a, dtype=F).astype(D), np.asarray(b, dtype=D)
    live = a64 != 0
    d = r64[live] - g64
    den = (b64[live] * (d * d).sum(1) + a64[live]).sum()
    return g64 + (a64[live, None] * d).sum(0) / den, den
