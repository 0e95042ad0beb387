"""Host restatement of csrc/efcomp.hip — TEST HELPER (not a test): numpy only, no GPU.

Error feedback and stochastic rounding for the update compressors, operation for operation in
np.float32 as include/fedhip.h states them (every fp32 operation rounded on its own):

    fold            v = fl32(fl32(x - base) + resid)
    topk_finish     d = keep ? v : +0;  x_out = fl32(base + d);  resid = keep ? +0 : v
    quant_finish    x_out = fl32(base + c);  resid = fl32(v - c)
    squant_segment  scale from max|v| (symmetric) or min / max (asymmetric), t = fl32(v / scale),
                    q = clamp(floor(t) + [(r >> 8) < (uint32)(fl32(t - floor t) * 2^24)]),
                    deq = fl32(q * scale) (+ lo); scale == 0 passes the segment through

The random words come from tests/philox_ref.py (word i & 3 of the block at counter
(id | 2^62, i >> 2)), the top-k keep rule and the deterministic quantiser from
oracle/compress_ref.py.  The upstream reference has none of this.

The row-level drivers take packed [C, W] arrays, a base of None / [1, W] (broadcast) / [C, W]
and the segment table, touch nothing outside [seg[0], seg[-1]) and return fresh arrays that
equal their inputs there.
"""
from __future__ import annotations

import numpy as np

import philox_ref
from oracle import compress_ref

F = np.float32
STREAM_BIT = 1 << 62  # FH_SQUANT_STREAM_BIT


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def base_row(base, z):
    return None if base is None else base[0 if base.shape[0] == 1 else z]


# ------------------------------------------------------------------ element definitions
def fold(x, base, resid):
    """v = fl32(fl32(x - base) + resid) (base None: fl32(x + resid))."""
    d = _f(x) if base is None else (_f(x) - _f(base)).astype(F)
    return (d + _f(resid)).astype(F)


def topk_keep(v, ratio):
    """uint8 keep mask of one segment: the k largest |v|, lowest indices among ties."""
    keep = np.zeros(v.size, np.uint8)
    keep[compress_ref.topk_indices(_f(v), compress_ref.topk_k(v.size, ratio))] = 1
    return keep


def topk_finish(base, v, keep):
    """(x_out, resid) of one segment."""
    k = keep.astype(bool)
    d = np.where(k, _f(v), F(0.0)).astype(F)
    x_out = d if base is None else (_f(base) + d).astype(F)
    return x_out, np.where(k, F(0.0), _f(v)).astype(F)


def quant_dense(v, bits, symmetric):
    """decompress(compress(v)) of the deterministic quantiser as fh_quantize_rows runs it: the
    reference's arithmetic, and a constant segment in asymmetric mode passes through."""
    v = _f(v)
    if not symmetric and v.min() == v.max():
        return v.copy()
    codes, scale, zp = compress_ref.quantize(v, bits, symmetric)
    return compress_ref.dequantize(codes, scale, zp).astype(F)


def quant_finish(base, v, c):
    x_out = _f(c) if base is None else (_f(base) + _f(c)).astype(F)
    return x_out, (_f(v) - _f(c)).astype(F)


def squant_words(key, cid, idx):
    """uint32 random words of the row elements idx of the client with global id cid."""
    idx = np.asarray(idx, dtype=np.uint64)
    r = philox_ref.philox4x32_10(int(key), int(cid) | STREAM_BIT, idx >> np.uint64(2))
    lane = (idx & np.uint64(3)).astype(np.int64)
    return np.choose(lane, [np.broadcast_to(w, idx.shape) for w in r]).astype(np.uint32)


def squant_segment(v, r, bits, symmetric):
    """One segment.  r: uint32 words.  Returns dict(deq, codes, q, t, scale, lo)."""
    v = _f(v)
    r = np.asarray(r, dtype=np.uint32)
    if symmetric:
        a = F(np.abs(v).max())
        qmax = F(2 ** (bits - 1) - 1)
        scale, lo = F(a / qmax), F(0.0)
        bot, top, bias = -qmax, qmax, int(qmax)
        u = v
    else:
        lo, hi = F(v.min()), F(v.max())
        top = F(2 ** bits - 1)
        scale = F(F(hi - lo) / top)
        bot, bias = F(0.0), 0
        u = (v - lo).astype(F)
    if not scale > 0:  # all zero / constant / one element: pass through
        z = np.zeros(v.size, np.int64)
        return {"deq": v.copy(), "codes": z.astype(np.uint8), "q": z, "t": np.zeros(v.size, F),
                "scale": scale, "lo": lo}
    t = (u / scale).astype(F)
    fl = np.floor(t).astype(F)
    f = (t - fl).astype(F)
    thr = (f * F(16777216.0)).astype(np.uint32)
    up = (r >> np.uint32(8)) < thr
    q = np.clip((fl + up.astype(F)).astype(F), bot, top).astype(F)
    d = (q * scale).astype(F)
    deq = d if symmetric else (lo + d).astype(F)
    qi = q.astype(np.int64)
    return {"deq": deq, "codes": ((qi + bias) & 0xFF).astype(np.uint8), "q": qi, "t": t,
            "scale": scale, "lo": lo}


# ------------------------------------------------------------------ packed rows
def _segments(seg):
    return list(zip(seg[:-1], seg[1:]))


def fold_rows(x, base, resid, seg):
    """resid with [seg[0], seg[-1]) of every row folded."""
    out = _f(resid).copy()
    a, e = seg[0], seg[-1]
    for z in range(x.shape[0]):
        b = base_row(base, z)
        out[z, a:e] = fold(x[z, a:e], None if b is None else b[a:e], resid[z, a:e])
    return out


def ef_topk_round(x, base, resid, seg, ratio):
    """One error-feedback top-k round: (x_out, resid_new, keep, v)."""
    v = fold_rows(x, base, resid, seg)
    x_out, r_new = _f(x).copy(), v.copy()
    keep = np.zeros(x.shape, np.uint8)
    for z in range(x.shape[0]):
        b = base_row(base, z)
        for a, e in _segments(seg):
            keep[z, a:e] = topk_keep(v[z, a:e], ratio)
            x_out[z, a:e], r_new[z, a:e] = topk_finish(None if b is None else b[a:e], v[z, a:e],
                                                       keep[z, a:e])
    return x_out, r_new, keep, v


def ef_quant_round(x, base, resid, seg, bits, symmetric):
    """One error-feedback round of the deterministic quantiser: (x_out, resid_new)."""
    v = fold_rows(x, base, resid, seg)
    x_out, r_new = _f(x).copy(), v.copy()
    for z in range(x.shape[0]):
        b = base_row(base, z)
        for a, e in _segments(seg):
            c = quant_dense(v[z, a:e], bits, symmetric)
            x_out[z, a:e], r_new[z, a:e] = quant_finish(None if b is None else b[a:e],
                                                        v[z, a:e], c)
    return x_out, r_new


def squant_round(x, base, resid, seg, bits, symmetric, key, ids, words=None):
    """fh_squant_rows on packed rows.  resid None: v = x - base; else v = fold(x, base, resid)
    (the fold and the quantiser, as compress_rows chains them).  Returns dict(out, codes,
    scale [C, nseg], lo [C, nseg], err = fl32(v - deq) (resid_out), resid (err, or None without
    resid), v)."""
    C = x.shape[0]
    v = _f(x).copy()
    a0, e0 = seg[0], seg[-1]
    if resid is not None:
        v = fold_rows(x, base, resid, seg)
    elif base is not None:
        for z in range(C):
            v[z, a0:e0] = (_f(x[z, a0:e0]) - _f(base_row(base, z)[a0:e0])).astype(F)
    out = _f(x).copy()
    err = v.copy()
    codes = np.zeros(x.shape, np.uint8)
    scale = np.zeros((C, len(seg) - 1), F)
    lo = np.zeros((C, len(seg) - 1), F)
    for z in range(C):
        b = base_row(base, z)
        for s, (a, e) in enumerate(_segments(seg)):
            r = words[z, a:e] if words is not None else squant_words(key, ids[z], np.arange(a, e))
            g = squant_segment(v[z, a:e], r, bits, symmetric)
            out[z, a:e] = g["deq"] if b is None else (_f(b[a:e]) + g["deq"]).astype(F)
            codes[z, a:e] = g["codes"]
            scale[z, s], lo[z, s] = g["scale"], g["lo"]
            err[z, a:e] = (v[z, a:e] - g["deq"]).astype(F)
    return {"out": out, "codes": codes, "scale": scale, "lo": lo, "err": err,
            "resid": None if resid is None else err, "v": v}


# ------------------------------------------------------------------ the unbiasedness check
# One vector, N distinct keys; the same on the CPU and on the device.
UNBIASED_N, UNBIASED_KEYS_N, UNBIASED_BITS, UNBIASED_ID = 4096, 256, 4, 5
UNBIASED_KEYS = [((k + 1) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1) for k in range(UNBIASED_KEYS_N)]


def unbiased_vector():
    rng = np.random.default_rng(20)
    return (rng.standard_normal(UNBIASED_N) * 0.05).astype(F)


def unbiased_bound(v, scale):
    """Hoeffding: every draw's error lies in an interval of width scale, so the mean of N draws
    is within scale * sqrt(ln(2 n / p) / (2 N)) of its expectation for all n elements at once
    with probability 1 - p, p = 1e-9 (= 0.241 scale at n = 4096, N = 256).  The expectation is
    within scale * 2^-24 of v (the threshold is truncated to 24 bits), and the fp32 roundings
    of t and q * scale move a value by at most one ulp of a = max|v|."""
    n, N = v.size, UNBIASED_KEYS_N
    h = float(np.sqrt(np.log(2.0 * n / 1e-9) / (2.0 * N)))
    assert h <= 0.241
    a = F(np.abs(v).max())
    ulp_a = float(np.spacing(a))
    return float(scale) * (h + 2.0 ** -24) + ulp_a
