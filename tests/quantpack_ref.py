"""Host restatement of csrc/quantpack.hip — TEST HELPER (not a test): numpy only, no GPU.

Packed quantised payloads as include/fedhip.h states them.  A code occupies cw bits (1, 2, 4, 8
for bits 1, 2, 3..4, 5..8); element j of segment s sits in byte boff[s] + (j * cw) // 8 of a
client's code row at bits [(j * cw) % 8, (j * cw) % 8 + cw), low bits first; boff is the exclusive
prefix sum of ceil(len_s * cw / 8) rounded up to 16.

    quantize_rows   what fh_quantize_rows writes: one code per element, scale, zp, dense out
    pack_rows       one code per byte -> code rows and passv
    validate        1 per (client, segment) with a code >= 2^bits, a bad scale or a bad passv
    dequant_rows    d = fl32(fl32((float)code - (float)zp) * (float)scale), pass-through rebuilt
    unpack_rows     out = fl32(base + d)
    quant_fedavg    acc = fl32(acc + fl32(fl32(w_k) * fl32(base + d_k))), sequential in k

The quantiser is oracle/compress_ref.py's (quantize / dequantize, imported), the sequential sum
oracle/fedavg_ref.py's.  The row-level drivers take packed [C, W] arrays, a base of None /
[1, W] (broadcast) / [C, W] and the segment table, and touch nothing outside [seg[0], seg[-1]).
"""
from __future__ import annotations

import numpy as np

from oracle import compress_ref, fedavg_ref

F = np.float32
INT64_MIN = -2 ** 63


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def base_row(base, z):
    return None if base is None else base[0 if base.shape[0] == 1 else z]


def code_width(bits):
    assert 1 <= bits <= 8
    return 1 if bits == 1 else 2 if bits == 2 else 4 if bits <= 4 else 8


def seg_bytes(seg, bits):
    cw = code_width(bits)
    return [((b - a) * cw + 7) // 8 for a, b in zip(seg[:-1], seg[1:])]


def boff(seg, bits):
    off = [0]
    for nb in seg_bytes(seg, bits):
        off.append(off[-1] + (nb + 15) // 16 * 16)
    return off


# ------------------------------------------------------------------ one segment
def pack_codes(codes, cw):
    """uint8 [ceil(n * cw / 8)]: codes (one per byte) cw bits each, low bits first; the unused
    high bits of the last byte are zero."""
    codes = np.asarray(codes, np.uint8)
    out = np.zeros((codes.size * cw + 7) // 8, np.uint8)
    bit = np.arange(codes.size) * cw
    np.bitwise_or.at(out, bit // 8,
                     ((codes.astype(np.uint32) & ((1 << cw) - 1)) << (bit % 8)).astype(np.uint8))
    return out


def unpack_codes(raw, cw, n):
    """uint8 [n]: the inverse of pack_codes."""
    raw = np.asarray(raw, np.uint8)
    j = np.arange(n) * cw
    return ((raw[j // 8].astype(np.uint32) >> (j % 8)) & ((1 << cw) - 1)).astype(np.uint8)


def dequant(codes, scale, zp, passv=F(0)):
    """d of one segment from its codes (one per byte).  zp == INT64_MIN: the segment was passed
    through, d = |passv| under the sign the code's bit 0 gives."""
    codes = np.asarray(codes, np.uint8)
    if zp == INT64_MIN:
        mag = np.asarray(passv, F).reshape(1).view(np.uint32)[0] & np.uint32(0x7FFFFFFF)
        return (mag | ((codes.astype(np.uint32) & 1) << np.uint32(31))).astype(np.uint32).view(F)
    with np.errstate(invalid="ignore", over="ignore"):
        return compress_ref.dequantize(codes, scale, zp).astype(F)


def quantize_segment(v, bits, symmetric):
    """(codes, scale, zp, passv, d) of one segment as fh_quantize_rows + the pack define them."""
    v = _f(v)
    if not symmetric and v.min() == v.max():  # the reference raises: passed through, flagged
        codes = (v.view(np.uint32) >> np.uint32(31)).astype(np.uint8)
        return codes, 0.0, INT64_MIN, v[0], dequant(codes, 0.0, INT64_MIN, v[0])
    codes, scale, zp = compress_ref.quantize(v, bits, symmetric)
    return codes, scale, zp, F(0), dequant(codes, scale, zp)


# ------------------------------------------------------------------ rows
def delta_rows(x, base, seg):
    v = _f(x).copy()
    a, e = seg[0], seg[-1]
    if base is not None:
        for z in range(x.shape[0]):
            v[z, a:e] = (_f(x[z, a:e]) - _f(base_row(base, z)[a:e])).astype(F)
    return v


def quantize_rows(x, base, seg, bits, symmetric):
    """dict(codes [C, W] uint8 one per element (0 outside the segments), scale [C, nseg] float64,
    zp [C, nseg] int64, passv [C, nseg] fp32, d [C, W] fp32)."""
    C, W = x.shape
    nseg = len(seg) - 1
    v = delta_rows(x, base, seg)
    r = dict(codes=np.zeros((C, W), np.uint8), scale=np.zeros((C, nseg), np.float64),
             zp=np.zeros((C, nseg), np.int64), passv=np.zeros((C, nseg), F),
             d=np.zeros((C, W), F), v=v)
    for z in range(C):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            codes, scale, zp, pv, d = quantize_segment(v[z, a:e], bits, symmetric)
            r["codes"][z, a:e], r["d"][z, a:e] = codes, d
            r["scale"][z, s], r["zp"][z, s], r["passv"][z, s] = scale, zp, pv
    return r


def pack_rows(codes, seg, bits, out=None):
    """uint8 [C, B]: the code rows.  out (optional) is updated in place: padding bytes keep what
    they held."""
    cw, bo, nb = code_width(bits), boff(seg, bits), seg_bytes(seg, bits)
    C = codes.shape[0]
    out = np.zeros((C, bo[-1]), np.uint8) if out is None else out
    for z in range(C):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            out[z, bo[s]:bo[s] + nb[s]] = pack_codes(codes[z, a:e], cw)
    return out


def unpack_code_rows(packed, seg, bits, W):
    """uint8 [C, W]: one code per element again."""
    cw, bo, nb = code_width(bits), boff(seg, bits), seg_bytes(seg, bits)
    out = np.zeros((packed.shape[0], W), np.uint8)
    for z in range(packed.shape[0]):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            out[z, a:e] = unpack_codes(packed[z, bo[s]:bo[s] + nb[s]], cw, e - a)
    return out


def validate(packed, scale, zp, passv, seg, bits):
    cw = code_width(bits)
    codes = unpack_code_rows(packed, seg, bits, seg[-1])
    C = packed.shape[0]
    bad = np.zeros((C, len(seg) - 1), np.int32)
    for z in range(C):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            b = bits < cw and bool((codes[z, a:e] >= 2 ** bits).any())
            b = b or not np.isfinite(scale[z, s]) or scale[z, s] < 0
            b = b or (zp[z, s] == INT64_MIN and not np.isfinite(passv[z, s]))
            bad[z, s] = int(b)
    return bad


def dequant_rows(packed, scale, zp, passv, seg, bits, W):
    codes = unpack_code_rows(packed, seg, bits, W)
    d = np.zeros((packed.shape[0], W), F)
    for z in range(packed.shape[0]):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            d[z, a:e] = dequant(codes[z, a:e], float(scale[z, s]), int(zp[z, s]), passv[z, s])
    return d


def unpack_rows(packed, scale, zp, passv, base, seg, bits, out):
    """out with [seg[0], seg[-1]) of every row replaced by fl32(base + d) (d without a base)."""
    out = _f(out).copy()
    d = dequant_rows(packed, scale, zp, passv, seg, bits, out.shape[1])
    a, e = seg[0], seg[-1]
    for z in range(packed.shape[0]):
        b = base_row(base, z)
        out[z, a:e] = d[z, a:e] if b is None else (_f(b[a:e]) + d[z, a:e]).astype(F)
    return out


def quant_fedavg(packed, scale, zp, passv, weights, base_row_, seg, bits, out, row_index=None,
                 accumulate=False):
    """out with [seg[0], seg[-1]) replaced by the sequential weighted sum of base + d_k."""
    out = _f(out).copy()
    a, e = seg[0], seg[-1]
    order = list(range(len(weights))) if row_index is None else list(row_index)
    d = dequant_rows(packed, scale, zp, passv, seg, bits, out.shape[0])
    rows = [d[r, a:e] if base_row_ is None else (_f(base_row_[a:e]) + d[r, a:e]).astype(F)
            for r in order]
    acc = out[a:e].copy() if accumulate else np.zeros(e - a, F)
    for r, w in zip(rows, weights):  # fedavg_ref.weighted_average's loop, from acc
        acc = (acc + (F(w) * r).astype(F)).astype(F)
    if not accumulate and rows:
        assert np.array_equal(acc.view(np.int32),
                              fedavg_ref.weighted_average(rows, weights).view(np.int32))
    out[a:e] = acc
    return out
