"""tests/sparse_ref.py against the existing references, and against the reference compressor's
own encoding (tests/golden/sparse_topk.json).  No GPU; floats are compared by their int32 view."""
import json
import os

import numpy as np
import pytest
import torch

import efcomp_ref as er
import sparse_ref as sr
from fedhip.compress import CompressionConfig
from fedhip._lib import FedHipError
from fedhip.wire import sort_segment
from oracle import compress_ref, fedavg_ref

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_topk.json")

C = 3
LENS = [1, 7, 300, 40]
LEAD, TAIL = 5, 9
SEG = np.concatenate([[LEAD], LEAD + np.cumsum(LENS)]).tolist()
A, E = SEG[0], SEG[-1]
W = E + TAIL
RATIOS = [0.9, 0.5, 0.0, 1.0]


def i32(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    return np.array_equal(i32(a), i32(b))


def problem(seed, per_row):
    rng = np.random.default_rng(seed)
    base = (rng.integers(-256, 257, size=(C if per_row else 1, W)) * 2.0 ** -10).astype(F)
    base[:, A + 3] = F(-0.0)
    base[:, A + 20:A + 40:3] = F(-0.0)
    x = (base + (rng.standard_normal((C, W)) * 0.05).astype(F)).astype(F)
    x[0, A + 20:A + 40] = base[0, A + 20:A + 40]        # zero deltas over a -0.0 base
    return x, base


def topk_dense_rows(x, base, ratio):
    """What fh_topk_rows writes, from the existing references alone."""
    out = x.copy()
    for z in range(C):
        b = er.base_row(base, z)
        for a, e in zip(SEG[:-1], SEG[1:]):
            v = x[z, a:e] if b is None else (x[z, a:e] - b[a:e]).astype(F)
            d = compress_ref.topk_dense(v, ratio)
            out[z, a:e] = d if b is None else (b[a:e] + d).astype(F)
    return out


@pytest.mark.parametrize("per_row", [False, True, None], ids=["broadcast", "per_row", "nobase"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_unpack_of_pack_is_the_dense_topk(ratio, per_row):
    x, base = problem(1, bool(per_row))
    if per_row is None:
        base = None
    idx, val, count, keep = sr.topk_pack(x, base, SEG, ratio)
    ko = sr.koff(SEG, ratio)
    assert np.array_equal(count, np.tile(sr.seg_k(SEG, ratio), (C, 1)))
    assert not sr.validate(idx, SEG, ko).any()
    poison = np.full((C, W), np.nan, F)
    got = sr.unpack_rows(idx, val, base, SEG, ko, poison)
    want = topk_dense_rows(x, base, ratio)
    assert same(got[:, A:E], want[:, A:E])
    assert np.isnan(got[:, :A]).all() and np.isnan(got[:, E:]).all()
    if base is not None and ratio == 0.9:   # a dropped coordinate over a -0.0 base: +0.0
        z0 = (i32(base[0, A:E]) == i32(F(-0.0))) & (keep[0, A:E] == 0)
        assert z0.any() and not i32(got[0, A:E])[z0].any()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("ratio", [0.9, 0.0])
def test_sparse_fedavg_is_dense_fedavg_of_the_unpacked_rows(ratio, accumulate):
    x, base = problem(2, False)
    idx, val, _, _ = sr.topk_pack(x, base, SEG, ratio)
    ko = sr.koff(SEG, ratio)
    order = [2, 0, 1]
    w = [1.0 / 3.0, 0.1, 0.7]
    rows = sr.unpack_rows(idx, val, base, SEG, ko, np.zeros((C, W), F))
    start = np.full(W, np.nan, F)
    start[A:E] = np.linspace(-1, 1, E - A).astype(F)
    got = sr.sparse_fedavg(idx, val, w, base[0], SEG, ko, start, row_index=order,
                           accumulate=accumulate)
    want = fedavg_ref.weighted_average([rows[r, A:E] for r in order], w)
    if accumulate:
        want = start[A:E].copy()
        for r, wk in zip(order, w):
            want = (want + (F(wk) * rows[r, A:E]).astype(F)).astype(F)
    assert same(got[A:E], want)
    assert np.isnan(got[:A]).all() and np.isnan(got[E:]).all()


def test_validate_flags_each_kind_of_bad_payload():
    x, base = problem(3, False)
    idx, _, _, _ = sr.topk_pack(x, base, SEG, 0.5)
    ko = sr.koff(SEG, 0.5)
    s = 2
    a = ko[s]
    assert ko[s + 1] - a >= 4 and not sr.validate(idx, SEG, ko).any()

    def flagged(edit):
        bad_idx = idx.copy()
        edit(bad_idx[1])
        bad = sr.validate(bad_idx, SEG, ko)
        want = np.zeros_like(bad)
        want[1, s] = 1
        return np.array_equal(bad, want)

    def negative(r): r[a] = -1
    def too_large(r): r[ko[s + 1] - 1] = LENS[s]
    def equal(r): r[a + 1] = r[a]
    def descending(r): r[a], r[a + 1] = r[a + 1], r[a]
    for edit in (negative, too_large, equal, descending):
        assert flagged(edit), edit.__name__
    top = idx.copy()
    top[1, ko[s + 1] - 1] = LENS[s] - 1                  # the largest valid index passes
    assert not sr.validate(top, SEG, ko).any()


def test_config_refusals():
    assert CompressionConfig("topk", sparse=True).sparse
    assert not CompressionConfig().sparse
    with pytest.raises(FedHipError, match="sparse"):
        CompressionConfig("quantization", sparse=True)


# ------------------------------------------------------------------ the reference's encoding
with open(GOLDEN) as _fh:
    _G = json.load(_fh)


def _u32(bits):
    return np.array(bits, np.uint32).view(F)


@pytest.mark.parametrize("name", sorted(_G["cases"]))
def test_reference_encoding_decodes_to_the_same_dense_tensor(name):
    c = _G["cases"][name]
    n, ratio = c["numel"], c["sparsity_ratio"]
    x = _u32(_G["inputs_u32"][str(n)])
    assert np.unique(np.abs(x)).size == n                # tie-free: the selection is unique
    seg = [0, n]
    idx, val, count, _ = sr.topk_pack(x[None], None, seg, ratio)
    ko = sr.koff(seg, ratio)
    assert ko[-1] == c["k"] == count[0, 0]
    # the reference's pairs (magnitude order) through the host sorting step of payloads_to_sparse
    ri, rv = sort_segment(torch.tensor(c["indices"], dtype=torch.int64),
                          torch.from_numpy(_u32(c["values_u32"]).copy()))
    ni, nv = sr.sort_segment(c["indices"], _u32(c["values_u32"]))
    assert np.array_equal(ri.numpy(), ni) and same(rv.numpy(), nv)
    assert np.array_equal(ri.numpy(), idx[0]) and same(rv.numpy(), val[0])
    dense = sr.unpack_rows(ri.numpy()[None].astype(np.int32), rv.numpy()[None], None, seg, ko,
                           np.zeros((1, n), F))
    assert same(dense[0], _u32(c["dense_u32"]))
    assert same(dense[0], compress_ref.topk_dense(x, ratio))
