"""Host restatement of csrc/sparse.hip — TEST HELPER (not a test): numpy only, no GPU.

Sparse top-k payloads as include/fedhip.h states them.  koff is the exclusive prefix sum of the
segments' k; client z's payload is idx[z][0..K) (int32, segment-local, strictly ascending inside
a segment) and val[z][0..K) (fp32), segment s at [koff[s], koff[s+1]).

    pack_rows       ordered compaction of a keep mask: idx = i - seg[s], val = v = fl32(x - base)
    validate        1 per (client, segment) with an index < 0, >= len or a non-ascending pair
    unpack_rows     out = fl32(base + d), d = val at the named indices, +0.0 elsewhere
    sparse_fedavg   acc = fl32(acc + fl32(fl32(w_k) * fl32(base + d_k))), sequential in k

The keep rule is oracle/compress_ref.py's (through tests/efcomp_ref.py), the sequential sum
oracle/fedavg_ref.py's.  The row-level drivers take packed [C, W] arrays, a base of None /
[1, W] (broadcast) / [C, W] and the segment table, and touch nothing outside [seg[0], seg[-1]).
"""
from __future__ import annotations

import numpy as np

import efcomp_ref
from oracle import compress_ref, fedavg_ref

F = np.float32


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def seg_k(seg, ratio):
    return [compress_ref.topk_k(b - a, ratio) for a, b in zip(seg[:-1], seg[1:])]


def koff(seg, ratio):
    return np.concatenate([[0], np.cumsum(seg_k(seg, ratio))]).astype(np.int64).tolist()


def delta_rows(x, base, seg):
    """v = fl32(x - base) on [seg[0], seg[-1]) (x itself without a base), x elsewhere."""
    v = _f(x).copy()
    a, e = seg[0], seg[-1]
    if base is not None:
        for z in range(x.shape[0]):
            b = efcomp_ref.base_row(base, z)
            v[z, a:e] = (_f(x[z, a:e]) - _f(b[a:e])).astype(F)
    return v


def keep_rows(v, seg, ratio):
    """uint8 keep mask [C, W] of the rows v (zero outside the segments)."""
    keep = np.zeros(v.shape, np.uint8)
    for z in range(v.shape[0]):
        for a, e in zip(seg[:-1], seg[1:]):
            keep[z, a:e] = efcomp_ref.topk_keep(v[z, a:e], ratio)
    return keep


def pack_rows(x, base, keep, seg, ko, idx=None, val=None):
    """(idx, val, count): the kept elements in ascending index order.  idx / val (optional,
    [C, >= K]) are updated in place: slots beyond a segment's count keep what they held, kept
    elements beyond a segment's slots are counted and dropped."""
    C, K = x.shape[0], ko[-1]
    idx = np.zeros((C, K), np.int32) if idx is None else idx
    val = np.zeros((C, K), F) if val is None else val
    count = np.zeros((C, len(seg) - 1), np.int32)
    v = delta_rows(x, base, seg)
    for z in range(C):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            at = np.flatnonzero(keep[z, a:e])
            count[z, s] = at.size
            at = at[:ko[s + 1] - ko[s]]
            idx[z, ko[s]:ko[s] + at.size] = at
            val[z, ko[s]:ko[s] + at.size] = v[z, a + at]
    return idx, val, count


def topk_pack(x, base, seg, ratio):
    """keep mask of v = x - base, then pack: (idx, val, count, keep)."""
    keep = keep_rows(delta_rows(x, base, seg), seg, ratio)
    return pack_rows(x, base, keep, seg, koff(seg, ratio)) + (keep,)


def validate(idx, seg, ko):
    C = idx.shape[0]
    bad = np.zeros((C, len(seg) - 1), np.int32)
    for z in range(C):
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            i = idx[z, ko[s]:ko[s + 1]].astype(np.int64)
            bad[z, s] = int((i < 0).any() or (i >= e - a).any() or (np.diff(i) <= 0).any())
    return bad


def dense_rows(idx, val, seg, ko, W):
    """d [C, W]: val at the named indices, +0.0 elsewhere (_desparsify_tensor per segment)."""
    d = np.zeros((idx.shape[0], W), F)
    for z in range(idx.shape[0]):
        for s, a in enumerate(seg[:-1]):
            d[z, a + idx[z, ko[s]:ko[s + 1]].astype(np.int64)] = val[z, ko[s]:ko[s + 1]]
    return d


def unpack_rows(idx, val, base, seg, ko, out):
    """out with [seg[0], seg[-1]) of every row replaced by fl32(base + d) (d without a base)."""
    out = _f(out).copy()
    d = dense_rows(idx, val, seg, ko, out.shape[1])
    a, e = seg[0], seg[-1]
    for z in range(idx.shape[0]):
        b = efcomp_ref.base_row(base, z)
        out[z, a:e] = d[z, a:e] if b is None else (_f(b[a:e]) + d[z, a:e]).astype(F)
    return out


def sparse_fedavg(idx, val, weights, base_row, seg, ko, out, row_index=None, accumulate=False):
    """out with [seg[0], seg[-1]) replaced by the sequential weighted sum of base + d_k."""
    out = _f(out).copy()
    a, e = seg[0], seg[-1]
    order = list(range(len(weights))) if row_index is None else list(row_index)
    d = dense_rows(idx, val, seg, ko, out.shape[0])
    rows = [(_f(base_row[a:e]) + d[r, a:e]).astype(F) for r in order]
    acc = out[a:e].copy() if accumulate else np.zeros(e - a, F)
    for r, w in zip(rows, weights):  # fedavg_ref.weighted_average's loop, from acc
        acc = (acc + (F(w) * r).astype(F)).astype(F)
    if not accumulate and rows:
        assert np.array_equal(acc.view(np.int32),
                              fedavg_ref.weighted_average(rows, weights).view(np.int32))
    out[a:e] = acc
    return out


def sort_segment(indices, values):
    """The host step of wire.payloads_to_sparse: one layer's pairs in ascending index order."""
    order = np.argsort(np.asarray(indices, np.int64), kind="stable")
    return np.asarray(indices)[order], np.asarray(values)[order]
