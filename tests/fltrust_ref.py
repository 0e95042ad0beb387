"""Plain numpy reference for FLTrust (csrc/fltrust.hip); no GPU.

The definition of fh_fltrust_rows (include/fedhip.h) on fp32 arrays, one rounded operation per
line: numpy's float32 / float64 +, -, *, / and sqrt are the IEEE correctly rounded ones and keep
denormals.  stats sums the exact fp64 products with np.sum (pairwise): the kernel's order
differs, so the GPU tests compare the sums to a summation-order tolerance.  coefficients is the
fp64 chain, left to right in k; the GPU tests feed it the kernel's OWN sums and compare what
follows.  step is the last line of the contract: center_ref's DELTA step around g, and g itself,
bit for bit, when every coefficient is zero.  rule_fp64 evaluates FLTrust in fp64 throughout (a
tolerance reference).

tests/test_fltrust_ref_cpu.py pins all of it against hand-worked cases and exact fractions.
"""
import numpy as np

import center_ref as cr
from robust_ref import same_bits  # noqa: F401  (re-exported)

SCORE, STEP = range(2)
STATE_DOUBLES = 4
F = np.float32
D = np.float64


def stats(rows, root, g):
    """(sq fp64 [C], dot fp64 [C], sq0): sums of exact fp64 products of the fp32 deltas."""
    rows, root, g = np.asarray(rows, dtype=F), np.asarray(root, dtype=F), np.asarray(g, dtype=F)
    with np.errstate(all="ignore"):
        d0 = root - g
        d = rows - g[None, :]
        assert d0.dtype == F and d.dtype == F
        d0, d = d0.astype(D), d.astype(D)
        return (d * d).sum(axis=1, dtype=D), (d * d0[None, :]).sum(axis=1, dtype=D), \
            D((d0 * d0).sum(dtype=D))


def coefficients(sq, dot, sq0):
    """(coef fp32 [C], trust fp64 [C], state fp64 [4]: S, live, trusted, n0) from the sums; all
    fp64, every operation on its own, S left to right."""
    sq, dot, sq0 = np.asarray(sq, dtype=D), np.asarray(dot, dtype=D), D(sq0)
    C = sq.shape[0]
    trust, nk = np.zeros(C, dtype=D), np.zeros(C, dtype=D)
    live = trusted = 0
    S = None
    with np.errstate(all="ignore"):
        n0 = np.sqrt(sq0)
        root_ok = bool(np.isfinite(sq0) and sq0 > 0)
        for k in range(C):
            ts = D(0.0)
            if np.isfinite(sq[k]) and sq[k] > 0 and np.isfinite(dot[k]):
                live += 1
                nk[k] = np.sqrt(sq[k])
                den = nk[k] * n0
                q = dot[k] / den
                ts = q if q > 0 else D(0.0)      # max(0, q); NaN gives 0
                ts = D(1.0) if ts > 1 else ts
            trusted += int(ts > 0)
            trust[k] = ts
            S = ts if S is None else S + ts
        coef = np.zeros(C, dtype=F)
        if root_ok and np.isfinite(S) and S > 0:
            for k in range(C):
                if trust[k] > 0:
                    scale = n0 / nk[k]
                    w = trust[k] * scale
                    coef[k] = F(w / S)
    return coef, trust, np.array([S, live, trusted, n0], dtype=D)


def step(rows, coef, g):
    """(out fp32 [P], sqdist_after fp64 [C]): g + sum_k coef_k * (x_k - g), center_ref's DELTA
    step; g itself, bit for bit, when every coefficient is zero."""
    rows, g = np.asarray(rows, dtype=F), np.asarray(g, dtype=F)
    coef = np.asarray(coef, dtype=F)
    if not np.any(coef != 0):
        return g.copy(), cr.sqdist(rows, g)
    return cr.center_iter(cr.DELTA, rows, coef, center=g)


def fltrust_rows(mode, rows, root, g):
    """(out or None, coef, trust, stats [2C + 1], state): the whole call."""
    sq, dot, sq0 = stats(rows, root, g)
    coef, trust, state = coefficients(sq, dot, sq0)
    out = step(rows, coef, g)[0] if mode == STEP else None
    return out, coef, trust, np.concatenate([sq, dot, [sq0]]), state


def rule_fp64(rows, root, g):
    """(out fp64 [P], trust fp64 [C], c fp64 [C]): FLTrust in fp64 throughout from the fp32
    inputs; non-finite rows and rows equal to g get score 0."""
    r64, g64 = np.asarray(rows, dtype=F).astype(D), np.asarray(g, dtype=F).astype(D)
    d0 = np.asarray(root, dtype=F).astype(D) - g64
    d = r64 - g64
    with np.errstate(all="ignore"):
        n0, nk = np.sqrt((d0 * d0).sum()), np.sqrt((d * d).sum(1))
        cos = (d * d0).sum(1) / (nk * n0)
        ts = np.where(np.isfinite(cos), np.clip(cos, 0.0, 1.0), 0.0)
        c = np.where(ts > 0, ts * (n0 / nk) / ts.sum(), 0.0)
    live = c != 0
    return g64 + (c[live, None] * d[live]).sum(0), ts, c
