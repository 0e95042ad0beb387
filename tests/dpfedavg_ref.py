"""Plain numpy reference for central DP-FedAvg (csrc/dpfedavg.hip) — TEST HELPER (not a test):
no GPU, no project code.

It restates the arithmetic of DESIGN.md §5 "Central DP-FedAvg" with every fp32 rounding
explicit: numpy's float32 -, * and + are the IEEE correctly rounded ones and keep denormals.
The norm is the exact sum (math.fsum), the Gaussian comes from philox_ref.  A NaN result is
stored as the one quiet NaN 0x7FC00000.

tests/test_dpfedavg_ref_cpu.py pins it against a hand-computed case and an independent fp64
formulation.  The keyword argument `wrong` exists for that file only: it builds deliberately
WRONG variants, to prove that a comparison against this reference would notice each of those
defects.  The GPU tests never pass it.
"""
import math

import numpy as np

import philox_ref as pr
from robust_ref import QNAN_BITS, same_bits  # noqa: F401  (same_bits: re-exported)

F = np.float32
STREAM_NOISE = (1 << 64) - 1   # the Philox stream word (ctr_hi) of the aggregate's noise
STREAM_BIT = (1 << 64) - 2     # ... of the noise on the clipped-bit count
MASK64 = (1 << 64) - 1


def round_key(dp_seed, seed, round_index):
    return (dp_seed * 6364136223846793005 + seed * 1442695040888963407 + round_index) & MASK64


def canon(x):
    x = np.array(x, dtype=F)
    x.view(np.uint32)[np.isnan(x)] = QNAN_BITS
    return x


def deltas(rows, g):
    """d_kj = fl32(x_kj - g_j); g None: the rows are deltas."""
    rows = np.asarray(rows, dtype=F)
    with np.errstate(all="ignore"):
        return rows if g is None else rows - np.asarray(g, dtype=F)[None, :]


def sqnorms(rows, g=None):
    """float64 [C]: the exactly rounded sum over the whole row of (double)d^2 (each square is
    exact in fp64: a 24-bit significand squared has 48 bits)."""
    d = deltas(rows, g).astype(np.float64)
    return np.array([math.fsum((r * r).tolist()) for r in d], dtype=np.float64)


def clip_coef(sq, clip, m):
    """(bits int32 [C], scale fp32 [C]) at the clip norm `clip` (fp64) for a round of m clients:
    b = n <= C, c = fl32(min(1, C/n)) with the division in fp64 and n = 0 giving 1,
    s = fl32(c * fl32(1/m))."""
    n = np.sqrt(np.asarray(sq, dtype=np.float64))
    clip = float(clip)
    bits = (n <= clip).astype(np.int32)
    with np.errstate(all="ignore"):
        c = np.where(n > clip, clip / np.where(n > clip, n, 1.0), 1.0).astype(F)
    w = F(1.0) / F(m)
    s = c * w
    assert s.dtype == F
    return bits, s


def z_delta(z, clip_lr, sigma_b):
    """The multiplier left for the deltas: z when the clip norm is fixed, else
    (z^-2 - (2 sigma_b)^-2)^(-1/2); 2 sigma_b <= z is refused."""
    if clip_lr == 0 or z == 0:
        return float(z)
    if 2.0 * sigma_b <= z:
        raise ValueError("2 * sigma_b must exceed z")
    return (z ** -2 - (2.0 * sigma_b) ** -2) ** -0.5


def sigma_avg(zd, clip, m):
    """fl32(z_delta * C_t / m), fp64, left to right."""
    return F(float(zd) * float(clip) / float(m))


def gauss(seed, P):
    """float64 [P]: the server's N(0, 1) stream, element j = lane j % 4 of counter j // 4."""
    return pr.gauss_row(seed, STREAM_NOISE, P)


def clipped_sum(rows, scale, g=None, noise=None, rows_are_deltas=False, add_global=True,
                wrong=None):
    """out fp32 [P]:  acc = (((0 + s_0*d_0) + s_1*d_1) + ...) in row order, one rounded multiply
    and one rounded add each;  t = acc + noise when noise is given (no noise: no add);
    out = g + t when g is given and add_global, else t."""
    rows = np.asarray(rows, dtype=F)
    scale = np.asarray(scale, dtype=F)
    with np.errstate(all="ignore"):
        d = rows if (rows_are_deltas or g is None) else deltas(rows, g)
        acc = np.zeros(rows.shape[1], dtype=F)
        order = range(len(rows))
        if wrong == "reverse":
            order = reversed(order)
        for k in order:
            if wrong == "fma":  # one rounding of s*d + acc
                acc = (scale[k].astype(np.float64) * d[k].astype(np.float64)
                       + acc.astype(np.float64)).astype(F)
                continue
            p = scale[k] * d[k]
            acc = acc + p
        if noise is not None:
            noise = np.asarray(noise, dtype=F)
        if wrong == "noise_first" and g is not None and add_global and noise is not None:
            return canon((np.asarray(g, dtype=F) + noise) + acc)
        t = acc if noise is None else acc + noise
        out = np.asarray(g, dtype=F) + t if (g is not None and add_global) else t
        assert out.dtype == F
        return canon(out)


def clip_after_weight_sum(rows, c, m, g):
    """A deliberately WRONG variant: c * (w * d) instead of (c * w) * d."""
    d = deltas(rows, g)
    w = F(1.0) / F(m)
    acc = np.zeros(d.shape[1], dtype=F)
    for k in range(len(d)):
        acc = acc + np.asarray(c, dtype=F)[k] * (w * d[k])
    return canon(np.asarray(g, dtype=F) + acc)


def clip_update(clip, bit_sum, m, gamma, eta, sigma_b, seed):
    """(bbar, C_{t+1}) in fp64: bbar = (sum b + sigma_b * xi) / m, C' = C * exp(-eta * (bbar -
    gamma)); xi = lane 0 of the Box-Muller on Philox(seed, STREAM_BIT, 0).  eta = 0: no draw,
    C' = C."""
    if eta == 0:
        return float(bit_sum) / m, float(clip)
    xi = float(pr.gauss4(seed, STREAM_BIT, 0)[0])
    bbar = (float(bit_sum) + float(sigma_b) * xi) / m
    return bbar, float(clip) * math.exp(-eta * (bbar - gamma))


def step(rows, g, clip, m, z, gamma, eta, sigma_b, seed, noise=None, scale=None):
    """One fused round.  Returns dict(sq, bits, scale, sigma, out, bbar, clip_next).  noise
    None and z > 0: sigma_avg * the Philox stream rounded to fp32 per factor is NOT formed here
    (the fp32 Box-Muller is the device's): pass the noise, or compare out within GAUSS_TOL.
    scale: use these coefficients instead of the reference's own."""
    sq = sqnorms(rows, g)
    bits, s = clip_coef(sq, clip, m)
    zd = z_delta(z, eta, sigma_b)
    out = clipped_sum(rows, s if scale is None else scale, g, noise=noise)
    bbar, nxt = clip_update(clip, int(bits.sum()), m, gamma, eta, sigma_b, seed)
    return dict(sq=sq, bits=bits, scale=s, sigma=sigma_avg(zd, clip, m), out=out, bbar=bbar,
                clip_next=nxt)


def gaussian_epsilon(z, T, delta):
    """T/(2 z^2) + sqrt(2 T ln(1/delta)) / z."""
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / delta)) / z
