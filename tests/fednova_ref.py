"""Plain numpy reference for FedNova (csrc/fednova.hip); no GPU.

fednova_rows is the definition of fh_fednova_rows (include/fedhip.h) on fp32 arrays, one rounded
operation per line, vectorised over the coordinates: numpy's float32 +, - and * are the IEEE
correctly rounded ones and keep denormals.  A NaN result is stored as the one quiet NaN
0x7FC00000.  coefficients is a pure-Python copy of fedhip.ops.fednova_coefficients.

tests/test_fednova_ref_cpu.py pins both against hand-worked cases and exact fractions.
"""
import math

import numpy as np

from robust_ref import QNAN_BITS, same_bits  # noqa: F401  (same_bits: re-exported)

STEP, PARTIAL, FINISH = range(3)
F = np.float32


def canon(x):
    x = np.array(x, dtype=F)
    x.view(np.uint32)[np.isnan(x)] = QNAN_BITS
    return x


def weighted_sum(rows, weights):
    """(((0 + w0*x0) + w1*x1) + ...): fh_fedavg_weighted_sum with accumulate = 0."""
    rows = np.asarray(rows, dtype=F)
    acc = np.zeros(rows.shape[1], dtype=F)
    for x, w in zip(rows, np.asarray(weights, dtype=F)):
        p = w * x
        acc = acc + p
    return acc


def normalised_sum(rows, coef, g):
    """acc = (((+0 + c0*(x0 - g)) + c1*(x1 - g)) + ...), not canonicalised."""
    rows, g = np.asarray(rows, dtype=F), np.asarray(g, dtype=F)
    coef = np.asarray(coef, dtype=F)
    assert rows.ndim == 2 and rows.shape[0] == coef.shape[0] >= 1
    acc = np.zeros(g.shape[0], dtype=F)
    with np.errstate(all="ignore"):
        for x, c in zip(rows, coef):
            d = x - g
            t = c * d
            acc = acc + t
            assert d.dtype == F and t.dtype == F and acc.dtype == F
    return acc


def fednova_rows(mode, rows, coef, g, tau_eff=0.0):
    """out fp32 [P].  STEP / PARTIAL: rows [C, P], coef [C].  FINISH: rows [1, P] (or [P]) is
    the sum itself, coef is ignored."""
    g = np.asarray(g, dtype=F)
    tau = F(tau_eff)
    with np.errstate(all="ignore"):
        if mode == FINISH:
            acc = np.asarray(rows, dtype=F).reshape(-1, g.shape[0])
            assert acc.shape[0] == 1
            acc = acc[0]
        else:
            acc = normalised_sum(rows, coef, g)
        if mode == PARTIAL:
            return canon(acc)
        s = tau * acc
        out = g + s
        assert s.dtype == F and out.dtype == F
    return canon(out)


def coefficients(weights, local_steps, tau_eff="weighted"):
    """(coef, tau_eff) in Python double: c_k = p_k / a_k, tau_eff = sum_k p_k * a_k summed in
    the given order, or the explicit finite positive tau_eff.  a_k == 0 needs p_k == 0 and gives
    c_k = 0.  ValueError otherwise."""
    p = [float(w) for w in weights]
    a = list(local_steps)
    if len(p) != len(a):
        raise ValueError("lengths differ")
    coef, tau = [], 0.0
    for pk, ak in zip(p, a):
        if isinstance(ak, bool) or int(ak) != ak or ak < 0:
            raise ValueError(f"bad step count {ak!r}")
        if ak == 0:
            if pk != 0.0:
                raise ValueError("no step but a weight")
            coef.append(0.0)
        else:
            coef.append(pk / int(ak))
            tau = tau + pk * int(ak)
    if tau_eff != "weighted":
        if isinstance(tau_eff, (str, bool)) or not math.isfinite(tau_eff) or tau_eff <= 0:
            raise ValueError(f"bad tau_eff {tau_eff!r}")
        tau = float(tau_eff)
    return coef, tau


def local_steps(sizes, batch, epochs=1):
    return [epochs * math.ceil(n / batch) for n in sizes]
