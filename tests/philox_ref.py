"""Host reference of the Philox streams — TEST HELPER (not a test): numpy only, no GPU, no
project code.

Every random decision of the HIP path is `Philox::gen(seed, hi, lo)` of csrc/fh_common.h (and
`u01` / `gauss4` on top of it), restated here from its specification:

    philox4x32_10   counter words (lo & 2^32-1, lo >> 32, hi & 2^32-1, hi >> 32), key words
                    (seed & 2^32-1, seed >> 32); 10 rounds of
                        hi0:lo0 = 0xD2511F53 * c0,  hi1:lo1 = 0xCD9E8D57 * c2
                        c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
                    with the key bumped by (0x9E3779B9, 0xBB67AE85) after each round
                    (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
    u01(x)          ((x >> 8) + 1) / 2^24: exact, in (0, 1]
    gauss4          Box-Muller on one block: ra = sqrt(-2 ln u01(r0)), rb = sqrt(-2 ln u01(r2)),
                    lanes (ra cos t1, ra sin t1, rb cos t3, rb sin t3), t = 2 pi u01(r1 / r3);
                    element j of a row is lane j % 4 of counter lo = j // 4
    keep_mask       element e is kept when u01(r0(seed, row, e)) <= 1 - p (1 - p in fp32)
    crop_flip       span = 2 pad + 1: i = (r0 * span) >> 32, j = (r1 * span) >> 32, flip = r2 >> 31
    row_key         the device key block is {step key, n_ids, id[0..)}: row z draws under id[z]
                    when n_ids != 0, else under z; the seed is seed_arg + block[0] mod 2^64

tests/test_philox_ref_cpu.py pins philox4x32_10 to the published Random123 known-answer
vectors.  The keyword arguments `rounds`, `swap_halves`, `lo_offset`, `lane_rot` and
`seed_bits` exist for that file only: they build deliberately WRONG generators, to prove that a
comparison against this reference would notice each of those defects.  The GPU tests never
pass them.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF

# ---- the tolerance of an fp32 Box-Muller draw against gauss4's fp64, per unit sigma -------
# |dg| <= r (|dtheta| + e_sincos) + |dr| + one rounding of the product r * cos / sin, with
#   r        <= sqrt(2 * 24 ln 2) = 5.77 (u01 >= 2^-24)
#   dtheta   <= 2 pi * 2 * 2^-24: the fp32 constant and the rounding of its product with u01
#   e_sincos <= 4 ulp of a value <= 1        (sinf / cosf / sincosf)
#   dr / r   <= 3 ulp (sqrtf) + 3 ulp / 2 (logf, halved by the root); the factor -2 is exact
# where ulp = 2^-23 relative.  The 3 / 4 / 3 ulp figures are the OpenCL specification's
# full-profile limits for log, sin / cos and sqrt; that the ROCm device library (OCML) behind
# HIP's logf, sincosf and sqrtf meets them is an assumption (ROCm ships no accuracy table).
# The derivation is spelled out in tests/test_philox_streams_gpu.py.
ULP32 = 2.0 ** -23
R_MAX = float(np.sqrt(2.0 * 24.0 * np.log(2.0)))
ULP_LOG, ULP_SINCOS, ULP_SQRT = 3.0, 4.0, 3.0
GAUSS_TOL = (R_MAX * (2.0 * np.pi * 2.0 * 2.0 ** -24 + ULP_SINCOS * ULP32)
             + R_MAX * (ULP_SQRT + ULP_LOG / 2.0) * ULP32
             + R_MAX * 2.0 ** -24)


def _u64(v):
    """Any integer scalar / array as uint64 (two's complement for negative values, as a C
    cast)."""
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) & MASK64)
    a = np.asarray(v)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object:
        return np.array([int(x) & MASK64 for x in a.ravel()], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def philox4x32_10(seed, hi, lo, rounds=10, swap_halves=False, lo_offset=0, lane_rot=0,
                  seed_bits=64):
    """(r0, r1, r2, r3) uint32 arrays of the broadcast shape of seed / hi / lo."""
    seed, hi, lo = np.broadcast_arrays(_u64(seed), _u64(hi), _u64(lo))
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    if seed_bits < 64:
        seed = seed & np.uint64((1 << seed_bits) - 1)
    if lo_offset:
        lo = lo + np.uint64(lo_offset)  # wraps mod 2^64
    if swap_halves:
        hi, lo = lo, hi
    c0, c1, c2, c3 = lo & m32, lo >> s32, hi & m32, hi >> s32
    k0, k1 = seed & m32, seed >> s32
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & m32, p1 >> s32, p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & m32
        k1 = (k1 + np.uint64(W1)) & m32
    r = [c.astype(np.uint32) for c in (c0, c1, c2, c3)]
    if lane_rot:
        r = r[lane_rot % 4:] + r[:lane_rot % 4]
    return tuple(r)


def u01(x):
    """uint32 -> float64 in (0, 1], exact."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / 2.0 ** 24


def gauss4(seed, hi, lo, lane_rot=0, **kw):
    """float64 [..., 4]: the four N(0, 1) draws of every counter."""
    r0, r1, r2, r3 = philox4x32_10(seed, hi, lo, **kw)
    ra = np.sqrt(-2.0 * np.log(u01(r0)))
    rb = np.sqrt(-2.0 * np.log(u01(r2)))
    ta, tb = 2.0 * np.pi * u01(r1), 2.0 * np.pi * u01(r3)
    g = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=-1)
    return np.roll(g, -lane_rot, axis=-1) if lane_rot else g


def gauss_row(seed, row, n, **kw):
    """float64 [n]: elements 0 .. n-1 of the row keyed `row`."""
    nq = (n + 3) // 4
    return gauss4(seed, row, np.arange(nq, dtype=np.uint64), **kw).reshape(-1)[:n]


def keep_mask(seed, row, n, p, **kw):
    """uint8 [n]: 1 where element e of the row keyed `row` is kept at drop probability p.
    The threshold is the kernels' fp32 keep probability 1.0f - (float)p (exact in fp64); for
    p = 0.5, 0.25, 0.3 it selects the same 2^-24 lattice values of u01 as the real 1 - p."""
    r0 = philox4x32_10(seed, row, np.arange(n, dtype=np.uint64), **kw)[0]
    return (u01(r0) <= float(np.float32(1.0) - np.float32(p))).astype(np.uint8)


def crop_flip(seed, row, b, pad, **kw):
    """uint8 [len(b), 3]: (crop row offset i, crop column offset j, flip) of batch slots b."""
    b = np.atleast_1d(_u64(b))
    r0, r1, r2, _ = philox4x32_10(seed, row, b, **kw)
    span = np.uint64(2 * pad + 1)
    i = (r0.astype(np.uint64) * span) >> np.uint64(32)
    j = (r1.astype(np.uint64) * span) >> np.uint64(32)
    return np.stack([i, j, (r2 >> np.uint32(31)).astype(np.uint64)], axis=-1).astype(np.uint8)


def key_block(step_key, ids=None):
    """The device key block {step key, n_ids, id[0..)} as a uint64 array."""
    ids = [] if ids is None else list(ids)
    return np.array([int(step_key) & MASK64, len(ids)] + [int(i) & MASK64 for i in ids],
                    dtype=np.uint64)


def row_key(block, z):
    """philox_row: the key of local row z under a key block (None: no block)."""
    if block is not None and int(block[1]) != 0:
        return int(block[2 + z])
    return int(z)


def effective_seed(seed_arg, block=None):
    """seed_arg + block[0] mod 2^64 with a key block, else seed_arg."""
    return ((int(seed_arg) & MASK64) + (0 if block is None else int(block[0]))) & MASK64
