"""Plain numpy reference for the geometric-median and centered-clipping kernels
(csrc/center.hip) and the two rules built on them; no GPU.

center_iter   the definition of fh_center_iter (include/fedhip.h) on fp32 arrays, one rounded
              operation per line, vectorised over the coordinates: numpy's float32 +, - and * are
              the IEEE correctly rounded ones and keep denormals.  A client whose coefficient is
              +-0 is skipped.  A NaN result is stored as the one quiet NaN 0x7FC00000.  The
              squared distances are fp32 differences, squared and summed in fp64 (np.sum: the
              order differs from the device's, which is why the GPU tests compare them within the
              summation-order bound, or exactly where every sum is exact).
center_coef   the definition of fh_center_coef in Python doubles (math.sqrt, / and * are IEEE
              correctly rounded), sums left to right.
geometric_median, centered_clip   the two rules as src/aggregation/robust.py sequences them.
              `replay` (a list of per-pass sqdist arrays, e.g. the device's last_sqdist) replaces
              the reference's own distances as the input of every coefficient step, so the fp32
              side can be compared bit for bit although fp64 sums differ in the last bit.

tests/test_center_ref_cpu.py pins all of it against hand-worked cases.
"""
import math

import numpy as np

from robust_ref import QNAN_BITS, median, same_bits  # noqa: F401  (same_bits: re-exported)

MEAN, DELTA = 0, 1
GEOMED, CCLIP = 0, 1
STATE_DOUBLES = 4
F = np.float32


def canon(x):
    x = np.array(x, dtype=F)
    x.view(np.uint32)[np.isnan(x)] = QNAN_BITS
    return x


def sqdist(rows, v):
    """fp64 [C]: sum_j ((double)fl32(x_kj - v_j))^2."""
    rows, v = np.asarray(rows, dtype=F), np.asarray(v, dtype=F)
    out = np.zeros(rows.shape[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for k, x in enumerate(rows):
            d = x - v
            assert d.dtype == F
            d = d.astype(np.float64)
            out[k] = np.sum(d * d)
    return out


def center_iter(mode, rows, coef, center=None):
    """(out fp32 [P], sqdist fp64 [C]).  rows [C, P], coef [C]; center [P] in DELTA."""
    rows = np.asarray(rows, dtype=F)
    coef = np.asarray(coef, dtype=F)
    assert rows.ndim == 2 and rows.shape[0] == coef.shape[0] >= 1
    P = rows.shape[1]
    acc = np.zeros(P, dtype=F)
    g = None if mode == MEAN else np.asarray(center, dtype=F)
    with np.errstate(all="ignore"):
        for x, c in zip(rows, coef):
            if c == 0:  # +0.0 and -0.0: the row is not multiplied in
                continue
            if mode == MEAN:
                t = c * x
            else:
                d = x - g
                assert d.dtype == F
                t = c * d
            acc = acc + t
            assert t.dtype == F and acc.dtype == F
        out = acc if mode == MEAN else g + acc
        assert out.dtype == F
    out = canon(out)
    return out, sqdist(rows, out)


def center_coef(rule, sq, alpha, param):
    """(coef fp32 [C], state fp64 [STATE_DOUBLES]) from the squared distances."""
    sq = [float(s) for s in sq]
    alpha = [float(a) for a in alpha]
    assert len(sq) == len(alpha) >= 1 and param > 0 and math.isfinite(param)
    C = len(sq)
    d = [math.sqrt(s) if s == s and s >= 0 else float("nan") for s in sq]
    live = [math.isfinite(s) and a > 0 for s, a in zip(sq, alpha)]
    coef = np.zeros(C, dtype=F)
    total = 0.0
    if rule == GEOMED:
        b = [a / max(param, dk) if lv else 0.0 for a, dk, lv in zip(alpha, d, live)]
        for k, bk in enumerate(b):
            total = bk if k == 0 else total + bk
        if total != 0.0:
            with np.errstate(all="ignore"):
                for k, bk in enumerate(b):
                    coef[k] = F(np.float64(bk) / np.float64(total))
    else:
        for k in range(C):
            if live[k]:
                coef[k] = F(alpha[k] * (param / d[k] if d[k] > param else 1.0))
            total = float(coef[k]) if k == 0 else total + float(coef[k])
    obj = 0.0
    for k in range(C):
        o = alpha[k] * d[k] if live[k] else 0.0
        obj = o if k == 0 else obj + o
    state = np.array([float(sum(live)), obj, total, float(param)], dtype=np.float64)
    return coef, state


def _run(rule, mode, rows, alpha, param, iters, v0, replay):
    rows = np.asarray(rows, dtype=F)
    dists = [sqdist(rows, v0)]
    use = (lambda i: np.asarray(replay[i], dtype=np.float64)) if replay is not None \
        else (lambda i: dists[i])
    coefs, states = [], []
    c, s = center_coef(rule, use(0), alpha, param)
    coefs.append(c)
    states.append(s)
    out = np.asarray(v0, dtype=F)
    for i in range(iters):
        out, sq = center_iter(mode, rows, coefs[i], center=out)
        dists.append(sq)
        c, s = center_coef(rule, use(i + 1), alpha, param)
        coefs.append(c)
        states.append(s)
    last = coefs[iters - 1]
    return out, {"sqdist": dists, "coef": coefs, "state": states, "last_coef": last,
                 "rejected": [k for k, ck in enumerate(last) if ck == 0],
                 "objective": float(states[iters][1]),
                 "live": min(float(s[0]) for s in states)}


def sample_weights(num_samples):
    """alpha_k = n_k / sum n in Python double (1/C each when the sum is 0)."""
    total = sum(num_samples)
    if total == 0:
        return [1.0 / len(num_samples)] * len(num_samples)
    return [n / total for n in num_samples]


def geometric_median(rows, alpha, nu=1e-6, iters=3, center=None, replay=None):
    """(out, info): `iters` smoothed Weiszfeld steps from `center` (default: the coordinate-wise
    median).  info: per-pass sqdist / coef / state, the last coefficients, the rejected
    positions, the objective at the result and the smallest live count of any pass."""
    rows = np.asarray(rows, dtype=F)
    v0 = median(rows) if center is None else np.asarray(center, dtype=F)
    return _run(GEOMED, MEAN, rows, alpha, nu, iters, v0, replay)


def centered_clip(rows, alpha, tau, iters=1, center=None, replay=None):
    """(out, info): `iters` clipping steps from the required `center`."""
    assert center is not None
    return _run(CCLIP, DELTA, rows, alpha, tau, iters, np.asarray(center, dtype=F), replay)
