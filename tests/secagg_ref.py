"""Host reference of secure aggregation (csrc/secagg.hip, src/aggregation/secure.py) — TEST
HELPER (not a test): numpy only, no GPU, no project code.  The Philox block function comes
from tests/philox_ref.py, which test_philox_ref_cpu.py pins to the published vectors.

    mask word        m(key, j) = word j % 4 of philox4x32_10(seed = key, hi = nonce, lo = j // 4)
    encode           v = fl32(w * x) (or x), r = rint(float64(v) * 2^frac_bits), NaN -> 0,
                     saturated to +-qmax (each counted as clipped), q = uint32(int32(r))
    encode_mask_rows out[z][j] = q + sum_t sign[z][t] * m(key[z][t], j)   mod 2^32
    sum_decode       acc[j] = sum_k masked[k][j] - sum_t sign[t] * m(key[t], j)   mod 2^32,
                     out[j] = float32(float64(int32(acc[j])) * 2^-frac_bits)
    pair_key(a, b)   r0 | r1 << 32 of philox4x32_10(seed = session seed, hi = a, lo = b), a < b
    self_key(a)      likewise from (hi = 2^64 - 1, lo = a)
    client a         adds the mask of pair (a, b) when a < b, subtracts it when a > b

The keyword arguments `lane_rot`, `lo_offset`, `drop_nonce` and `flip_signs` exist for
tests/test_secagg_ref_cpu.py only: they build deliberately WRONG maskers, to prove that a
comparison against this reference would notice each defect.  The GPU tests never pass them.
"""
import numpy as np

from philox_ref import MASK64, philox4x32_10


def masks(keys, nonce, P, lane_rot=0, lo_offset=0, drop_nonce=False):
    """uint32 [T, P]: row t holds m(keys[t], j) for j < P."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    nq = (P + 3) // 4
    if len(keys) == 0 or P == 0:
        return np.zeros((len(keys), P), dtype=np.uint32)
    r = philox4x32_10(keys[:, None], 0 if drop_nonce else int(nonce) & MASK64,
                      np.arange(nq, dtype=np.uint64)[None, :], lo_offset=lo_offset,
                      lane_rot=lane_rot)
    return np.stack(r, axis=-1).reshape(len(keys), 4 * nq)[:, :P]


def mask_sum(keys, signs, nonce, P, flip_signs=False, **defects):
    """uint32 [P]: sum_t sign[t] * m(key[t], .) mod 2^32; terms with sign 0 are skipped."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    signs = np.asarray(signs, dtype=np.int64).reshape(-1)
    if flip_signs:
        signs = -signs
    live = signs != 0
    m = masks(keys[live], nonce, P, **defects).astype(np.int64)
    return ((m * signs[live, None]).sum(axis=0) & 0xFFFFFFFF).astype(np.uint32)


def encode(rows, weights, frac_bits, qmax):
    """(q uint32 [C, P], clipped int64 [C]): the plain fixed-point codes."""
    x = np.asarray(rows, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = x if weights is None else \
            (np.asarray(weights, dtype=np.float32)[:, None] * x).astype(np.float32)
        r = np.rint(v.astype(np.float64) * 2.0 ** frac_bits)  # exact product, ties to even
    nan = np.isnan(r)
    hi, lo = r > qmax, r < -qmax  # both False for NaN
    r = np.where(nan, 0.0, np.where(hi, float(qmax), np.where(lo, -float(qmax), r)))
    clipped = (nan | hi | lo).sum(axis=1)
    return r.astype(np.int64).astype(np.int32).view(np.uint32), clipped


def encode_mask_rows(rows, weights, frac_bits, qmax, keys, signs, nonce, **defects):
    """(out uint32 [C, P], clipped [C]); keys / signs: [C, T] (or None: no terms)."""
    q, clipped = encode(rows, weights, frac_bits, qmax)
    out = q.copy()
    if keys is not None:
        for z in range(q.shape[0]):
            out[z] += mask_sum(keys[z], signs[z], nonce, q.shape[1], **defects)  # wraps mod 2^32
    return out, clipped


def decode(acc, frac_bits):
    """float32 [P]: the ring elements read as int32, times 2^-frac_bits, one rounding."""
    return (np.asarray(acc, dtype=np.uint32).view(np.int32).astype(np.float64)
            * 2.0 ** -frac_bits).astype(np.float32)


def sum_decode(masked, keys, signs, nonce, frac_bits, **defects):
    """(out float32 [P], acc uint32 [P]) over all rows of `masked` (uint32 [K, P])."""
    masked = np.asarray(masked, dtype=np.uint32)
    acc = (masked.astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if keys is not None and len(keys):
        acc = acc - mask_sum(keys, signs, nonce, masked.shape[1], **defects)
    return decode(acc, frac_bits), acc


# ------------------------------------------------------------------ the protocol's keys
def _key(seed, hi, lo):
    r = philox4x32_10(int(seed) & MASK64, int(hi) & MASK64, int(lo) & MASK64)
    return int(r[0]) | int(r[1]) << 32


def pair_key(seed, a, b):
    assert a < b
    return _key(seed, a, b)


def self_key(seed, a):
    return _key(seed, MASK64, a)


def client_terms(seed, ids, self_masks=False):
    """(keys uint64 [C, T], signs int32 [C, T]), T = max(1, C - 1 + self_masks); unused slots
    have sign 0."""
    C = len(ids)
    T = max(1, C - 1 + int(self_masks))
    keys = np.zeros((C, T), dtype=np.uint64)
    signs = np.zeros((C, T), dtype=np.int32)
    for i, a in enumerate(ids):
        t = 0
        for b in ids:
            if b != a:
                keys[i, t] = pair_key(seed, min(a, b), max(a, b))
                signs[i, t] = 1 if a < b else -1
                t += 1
        if self_masks:
            keys[i, t], signs[i, t] = self_key(seed, a), 1
    return keys, signs


def server_terms(seed, survivors, dropped, self_masks=False):
    """(keys uint64 [T], signs int32 [T]) left in the survivors' sum."""
    keys, signs = [], []
    for s in survivors:
        for d in dropped:
            keys.append(pair_key(seed, min(s, d), max(s, d)))
            signs.append(1 if s < d else -1)
        if self_masks:
            keys.append(self_key(seed, s))
            signs.append(1)
    return np.array(keys, dtype=np.uint64), np.array(signs, dtype=np.int32)


def fedavg_weights(num_samples):
    """FedAvg's n_k / N in Python doubles (rounded to fp32 where they multiply)."""
    total = sum(num_samples)
    return [n / total for n in num_samples]


def secure_fedavg(rows, num_samples, ids, seed, nonce, frac_bits, survivors=None,
                  self_masks=False):
    """What SecureAggregator computes: (decoded fp32 row, masked uint32 [C, P], clipped).
    `survivors` (ids; default all): the rest dropped after masking, and the survivors' sum is
    scaled once in fp32 by fl32(N / N_S)."""
    C = len(ids)
    qmax = (2 ** 31 - 1) // C
    keys, signs = client_terms(seed, ids, self_masks)
    masked, clipped = encode_mask_rows(rows, fedavg_weights(num_samples), frac_bits, qmax, keys,
                                       signs, nonce)
    survivors = list(ids) if survivors is None else list(survivors)
    dropped = [c for c in ids if c not in survivors]
    sk, ss = server_terms(seed, survivors, dropped, self_masks)
    out, _ = sum_decode(masked[[list(ids).index(s) for s in survivors]], sk, ss, nonce, frac_bits)
    if dropped:
        n_s = sum(num_samples[list(ids).index(s)] for s in survivors)
        out = (np.float32(sum(num_samples) / n_s) * out).astype(np.float32)
    return out, masked, clipped


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize == 4 and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))
