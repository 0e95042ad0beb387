"""csrc/sparse.hip on the device: fh_topk_pack_rows, fh_sparse_validate, fh_sparse_unpack_rows and
fh_sparse_fedavg, bit for bit against tests/sparse_ref.py and against the kernels they stand in
for (fh_topk_rows, fh_fedavg_weighted_sum), their chaining in compress_rows(sparse_out=), the
wire payloads of fedhip/wire.py and RankRound(compression=CompressionConfig(sparse=True)).

Shapes as tests/test_efcomp_gpu.py: 3 client rows, segments of 1, 7, 8191, 8193 and 300 elements
behind a lead of 5 and before a tail of 9; "aligned" rows (16-byte aligned, stride a multiple of
4) and "scalar" rows (stride W + 1 / K + 1, every pointer one element off); the base one
broadcast row or one row per client, with -0.0 in it.  Every buffer has a padding row and is
pre-filled with a NaN pattern (0xA5 for bytes); everything outside [seg_offsets[0],
seg_offsets[nseg]) of the parameter rows and outside [0, K) of the payload rows must keep it.
Inputs are finite.  Bad payloads only ever reach fh_sparse_validate and payloads_to_sparse.

No tolerances: floats are compared by their int32 view."""
import functools
import types

import numpy as np
import pytest
import torch

import efcomp_ref as er
import sparse_ref as sr
from fedhip import ops, wire
from fedhip._lib import FedHipError
from fedhip.compress import CompressionConfig, SegmentPlan, compress_rows, topk_rows
from fedhip.sparse import (SparsePlan, SparseUpdates, sparse_fedavg, sparse_unpack_rows,
                           sparse_validate, topk_pack_rows)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F = np.float32

C = 3
LEAD, TAIL = 5, 9
LENS = [1, 7, 8191, 8193, 300]
SEG = np.concatenate([[LEAD], LEAD + np.cumsum(LENS)]).tolist()
A, E = SEG[0], SEG[-1]
W = E + TAIL
NSEG = len(LENS)
BIG = 3                           # the 8193-element segment: two chunks
POISON_I32 = 0x7FC0BEEF          # a quiet NaN with a payload
POISON_U8 = 0xA5
VARIANTS = ["aligned", "scalar"]
MODES = ["broadcast", "per_row"]
RATIOS = [0.9, 0.5, 0.0, 1.0]
NEG0 = np.array([0x80000000], np.uint32).view(F)[0]


def i32(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    return np.array_equal(i32(a), i32(b))


class Buf:
    """[rows + 1, stride] device rows over one poisoned flat allocation; .view is
    [:rows, :width] and [lo, hi) of its rows is what a launch may write."""

    def __init__(self, variant, dtype=torch.float32, rows=C, width=W, lo=A, hi=E):
        self.dtype, self.rows, self.lo, self.hi = dtype, rows, lo, hi
        self.stride = (width + 3) // 4 * 4 + 4 if variant == "aligned" else width + 1
        self.off = 0 if variant == "aligned" else 1
        n = (rows + 1) * self.stride
        if dtype == torch.uint8:
            self.flat = torch.full((n + 16,), POISON_U8, dtype=dtype, device=DEV)
        else:
            self.flat = torch.full((n + 4,), POISON_I32, dtype=torch.int32, device=DEV)
            if dtype == torch.float32:
                self.flat = self.flat.view(torch.float32)
        self.full = self.flat[self.off:self.off + n].view(rows + 1, self.stride)
        self.view = self.full[:rows, :width]
        assert self.flat.data_ptr() % 16 == 0 and self.view.stride(0) == self.stride

    def put(self, arr):
        a = np.array(arr[:, self.lo:self.hi])        # a copy: the inputs are read-only
        self.view[:, self.lo:self.hi] = torch.from_numpy(a).to(DEV)
        return self

    def get(self):
        return self.view.cpu().numpy()[:, self.lo:self.hi]

    def assert_poison_outside(self):
        mask = torch.ones(self.flat.shape, dtype=torch.bool, device=DEV)
        n = self.full.numel()
        mask[self.off:self.off + n].view(self.full.shape)[:self.rows, self.lo:self.hi] = False
        flat = self.flat if self.dtype != torch.float32 else self.flat.view(torch.int32)
        assert bool((flat[mask] == (POISON_U8 if self.dtype == torch.uint8 else POISON_I32)).all())


class Base:
    def __init__(self, variant, arr):
        """arr: [1, W] (broadcast, stride 0) or [C, W]."""
        arr = np.array(arr, F)
        if arr.shape[0] == 1:
            off = 0 if variant == "aligned" else 1
            self.flat = torch.zeros(W + 4, device=DEV)
            self.flat[off:off + W] = torch.from_numpy(arr[0]).to(DEV)
            self.row = self.flat[off:off + W]
            self.view = self.row.view(1, W).expand(C, -1)
            assert self.view.stride(0) == 0
        else:
            b = Buf(variant, rows=arr.shape[0])
            b.full[:arr.shape[0], :W] = torch.from_numpy(arr).to(DEV)
            self.flat, self.view = b.flat, b.view
        self.before = self.flat.clone()

    def assert_unchanged(self):
        assert torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32))


@functools.lru_cache(maxsize=None)
def plan():
    p = SegmentPlan(SEG, DEV)
    assert p.chunk == 8192 and p.nchunks == NSEG + 1     # only the 8193 segment has two chunks
    return p


@functools.lru_cache(maxsize=None)
def splan(ratio):
    sp = SparsePlan(plan(), ratio)
    assert sp.koff_host == sr.koff(SEG, ratio) and sp.k == sr.seg_k(SEG, ratio)
    return sp


def payload_bufs(variant, ratio, rows=C):
    K = splan(ratio).K
    idx = Buf(variant, torch.int32, rows=rows, width=K, lo=0, hi=K)
    val = Buf(variant, torch.float32, rows=rows, width=K, lo=0, hi=K)
    return idx, val, SparseUpdates(idx.view, val.view, splan(ratio))


@functools.lru_cache(maxsize=None)
def make_base(mode):
    """Multiples of 2^-10 below 0.25, with -0.0 sprinkled in."""
    rng = np.random.default_rng(7 + (mode == "per_row"))
    b = (rng.integers(-256, 257, size=(1 if mode == "broadcast" else C, W)) * 2.0 ** -10).astype(F)
    b[:, A:E:5] = NEG0
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def problem(kind, ratio, mode, rows=C):
    """(x, base, reference pack) — "normal": Gaussian deltas; "ties": deltas on four magnitudes,
    exact over the grid base, so the k-th magnitude is shared by many elements."""
    rng = np.random.default_rng(int(ratio * 10) + 100 * (mode == "per_row") + 1000 * rows
                                + (kind == "ties"))
    base = make_base(mode)
    if rows != C:
        assert mode == "broadcast"
    if kind == "normal":
        delta = (rng.standard_normal((rows, W)) * 0.05).astype(F)
        delta[0, A + 40:A + 60] = 0.0                    # dropped coordinates over -0.0
    else:
        delta = (rng.integers(1, 5, size=(rows, W)) * rng.choice([-1.0, 1.0], size=(rows, W))
                 * 2.0 ** -6).astype(F)
        if ratio in (0.9, 0.5):
            # the two-chunk segment: k - 700 elements above T = 3 * 2^-6, 2000 elements at T all
            # over the segment (700 of them are kept), the rest below; the segment's last
            # element, alone in its chunk, is one of the tie
            a, e = SEG[BIG], SEG[BIG + 1]
            k = sr.seg_k(SEG, ratio)[BIG]
            for z in range(rows):
                order = rng.permutation(e - a - 1)
                mag = rng.integers(1, 3, size=e - a).astype(F)
                mag[order[:k - 700]] = 4.0
                mag[order[k - 700:k + 1300 - 1]] = 3.0
                mag[e - a - 1] = 3.0
                delta[z, a:e] = np.copysign(mag * F(2.0 ** -6), delta[z, a:e])
    x = (base + delta).astype(F)
    if kind == "ties":
        assert same((x - base)[:, A:E], delta[:, A:E])   # the grid base keeps the deltas exact
    x.setflags(write=False)
    ref = sr.topk_pack(x, base, SEG, ratio)
    if kind == "ties" and ratio in (0.9, 0.5):
        v, keep = sr.delta_rows(x, base, SEG), ref[3]
        a, e = SEG[BIG], SEG[BIG + 1]
        k = sr.seg_k(SEG, ratio)[BIG]
        for z in range(rows):                            # the tie is really there, and cut
            m = np.abs(v[z, a:e])
            T = np.sort(m)[::-1][k - 1]
            tie = np.flatnonzero(m == T)
            kept = tie[keep[z, a + tie] == 1]
            assert 0 < kept.size < tie.size and m[e - a - 1] == T
            assert len(set(kept // 64)) > 1 and len(set(kept // 256)) > 1   # waves, passes
            assert tie[-1] == 8192 and (tie < 8192).any()                   # both chunks
    return x, base, ref


def device_pack(variant, x_np, base_np, ratio, count=True):
    """topk_rows' keep mask and dense output, then the pack: everything the tests compare."""
    base = None if base_np is None else Base(variant, np.asarray(base_np))
    x = Buf(variant).put(x_np)
    keep = Buf(variant, torch.uint8)
    dense = Buf(variant)
    bview = None if base is None else base.view
    topk_rows(plan(), x.view, C, ratio, base=bview, out=dense.view, keep=keep.view)
    idx, val, upd = payload_bufs(variant, ratio)
    cnt = torch.full((C, NSEG), -7, dtype=torch.int32, device=DEV) if count else None
    topk_pack_rows(upd, x.view, keep.view, C, base=bview, count_out=cnt)
    torch.cuda.synchronize()
    for b in (keep, dense, idx, val):
        b.assert_poison_outside()
    x_before = Buf(variant).put(x_np)
    assert torch.equal(x.flat.view(torch.int32), x_before.flat.view(torch.int32))
    if base is not None:
        base.assert_unchanged()
    return types.SimpleNamespace(base=base, x=x, keep=keep, dense=dense, idx=idx, val=val,
                                 upd=upd, cnt=cnt)


# ------------------------------------------------------------------ pack, unpack
@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_pack_and_unpack(variant, ratio, mode, kind):
    x, base, (ridx, rval, rcount, rkeep) = problem(kind, ratio, mode)
    d = device_pack(variant, x, base, ratio)
    assert np.array_equal(d.keep.get(), rkeep[:, A:E])
    assert np.array_equal(d.idx.get(), ridx)
    assert same(d.val.get(), rval)
    assert np.array_equal(d.cnt.cpu().numpy(), rcount)
    assert np.array_equal(rcount, np.tile(sr.seg_k(SEG, ratio), (C, 1)))
    assert not sparse_validate(d.upd).cpu().numpy().any()
    # unpack: fh_topk_rows' own output is the yardstick
    out = Buf(variant)
    sparse_unpack_rows(d.upd, out.view, C, base=d.base.view)
    torch.cuda.synchronize()
    out.assert_poison_outside()
    d.base.assert_unchanged()
    assert same(out.get(), d.dense.get())
    assert same(out.get(), sr.unpack_rows(ridx, rval, base, SEG, sr.koff(SEG, ratio),
                                          np.zeros((C, W), F))[:, A:E])
    if ratio == 0.9:     # a dropped coordinate over a base of -0.0 comes out +0.0
        b0 = np.broadcast_to(base, (C, W))[:, A:E]
        z0 = (i32(b0) == i32(NEG0)) & (rkeep[:, A:E] == 0)
        assert z0.any() and not i32(out.get())[z0].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_pack_and_unpack_without_a_base(variant):
    x, _, _ = problem("normal", 0.9, "broadcast")
    ridx, rval, rcount, _ = sr.topk_pack(x, None, SEG, 0.9)
    d = device_pack(variant, x, None, 0.9, count=False)
    assert np.array_equal(d.idx.get(), ridx) and same(d.val.get(), rval)
    out = Buf(variant)
    sparse_unpack_rows(d.upd, out.view, C)
    torch.cuda.synchronize()
    out.assert_poison_outside()
    assert same(out.get(), d.dense.get())


def test_unpack_in_place_over_per_row_base():
    """out may be the base rows when every client has its own."""
    x, base, _ = problem("normal", 0.5, "per_row")
    d = device_pack("aligned", x, base, 0.5)
    sparse_unpack_rows(d.upd, d.base.view, C, base=d.base.view)
    torch.cuda.synchronize()
    assert same(d.base.view.cpu().numpy()[:, A:E], d.dense.get())
    with pytest.raises(FedHipError, match="alias"):
        row = torch.zeros(W, device=DEV)
        sparse_unpack_rows(d.upd, row.view(1, W), 1, base=row.view(1, W).expand(C, -1))


# ------------------------------------------------------------------ sparse FedAvg
@pytest.mark.parametrize("accumulate", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("ratio", [0.9, 0.0])
@pytest.mark.parametrize("nc", [1, 3, 17, 70])
def test_sparse_fedavg_equals_the_dense_sum(nc, ratio, accumulate):
    """fh_fedavg_weighted_sum over fh_topk_rows' output is the yardstick (70 clients: more than
    one batch of the slice search)."""
    variant = VARIANTS[(nc + accumulate) % 2]
    x, base_np, (ridx, rval, _, _) = problem("ties" if nc == 3 else "normal", ratio, "broadcast",
                                             rows=nc)
    rng = np.random.default_rng(nc)
    perm = np.roll(rng.permutation(nc), 1) if nc < 4 else rng.permutation(nc)
    assert nc == 1 or not np.array_equal(perm, np.arange(nc))
    w_np = (rng.random(nc) / nc + 1e-3).astype(F)
    assert any(float(F(w) * F(3)) != float(w) * 3 for w in w_np)      # not exact in fp32
    base = Base(variant, np.asarray(base_np))
    bview = base.row.view(1, W).expand(nc, -1)
    xs = torch.from_numpy(np.array(x)).to(DEV)
    dense = torch.zeros(nc, (W + 3) // 4 * 4, device=DEV)
    keep = torch.empty(nc, W, dtype=torch.uint8, device=DEV)
    topk_rows(plan(), xs, nc, ratio, base=bview, out=dense, keep=keep)
    idx, val, upd = payload_bufs(variant, ratio, rows=nc)
    topk_pack_rows(upd, xs, keep, nc, base=bview)
    w = torch.from_numpy(w_np).to(DEV)
    ri = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    start = (rng.standard_normal(W) * 0.1).astype(F)
    want = torch.from_numpy(start).to(DEV)
    ops.fedavg_weighted_sum(dense, w, want, row_index=ri, accumulate=accumulate, P=E)
    out = Buf(variant, rows=1)
    out.put(start[None])
    sparse_fedavg(upd, w, base.row, out.view[0], row_index=ri, accumulate=accumulate)
    torch.cuda.synchronize()
    out.assert_poison_outside()
    base.assert_unchanged()
    idx.assert_poison_outside()
    val.assert_poison_outside()
    assert same(out.get()[0], want.cpu().numpy()[A:E])
    ref = sr.sparse_fedavg(ridx, rval, w_np.tolist(), np.asarray(base_np)[0], SEG,
                           sr.koff(SEG, ratio), start, row_index=perm.tolist(),
                           accumulate=accumulate)
    assert same(out.get()[0], ref[A:E])
    if not accumulate and nc > 1:      # the order of the sum matters: another one, other bits
        sparse_fedavg(upd, w, base.row, out.view[0])
        torch.cuda.synchronize()
        assert not same(out.get()[0], ref[A:E])


# ------------------------------------------------------------------ validate, wire payloads
LAYOUT = types.SimpleNamespace(names=[f"layer{s}.weight" for s in range(NSEG)],
                               shapes=[(n,) for n in LENS])
BAD_S, BAD_Z = 2, 1


def _bad_edits(ko):
    a, b = ko[BAD_S], ko[BAD_S + 1]

    def negative(r): r[a + 2] = -1
    def too_large(r): r[b - 1] = LENS[BAD_S]
    def equal(r): r[a + 1] = r[a]
    def descending(r): r[a], r[a + 1] = r[a + 1].copy(), r[a].copy()
    return [negative, too_large, equal, descending]


@pytest.mark.parametrize("kind", ["negative", "too_large", "equal", "descending"])
def test_validate_flags_bad_payloads(kind):
    ratio = 0.9
    x, base, (ridx, rval, _, _) = problem("normal", ratio, "broadcast")
    ko = sr.koff(SEG, ratio)
    edit = {e.__name__: e for e in _bad_edits(ko)}[kind]
    bad_idx = ridx.copy()
    edit(bad_idx[BAD_Z])
    want = np.zeros((C, NSEG), np.int32)
    want[BAD_Z, BAD_S] = 1
    assert np.array_equal(sr.validate(bad_idx, SEG, ko), want)
    for variant in VARIANTS:
        idx, val, upd = payload_bufs(variant, ratio)
        idx.put(bad_idx)
        flags = torch.full((C, NSEG), -7, dtype=torch.int32, device=DEV)
        got = sparse_validate(upd, bad_out=flags)
        torch.cuda.synchronize()
        idx.assert_poison_outside()
        assert np.array_equal(got.cpu().numpy(), want)
    # the same payload as a coordinator would receive it
    good = SparseUpdates(torch.from_numpy(ridx).to(DEV), torch.from_numpy(rval).to(DEV),
                         splan(ratio))
    payloads = wire.sparse_to_payloads(good, LAYOUT, C)
    name = LAYOUT.names[BAD_S]
    seg = payloads[BAD_Z]["compressed_weights"][name]
    a, b = ko[BAD_S], ko[BAD_S + 1]
    seg["indices"] = torch.from_numpy(bad_idx[BAD_Z, a:b].astype(np.int64))
    if kind == "descending":   # any order is accepted: the host sort carries the values along
        edit_v = rval[BAD_Z].copy()
        edit(edit_v)
        seg["values"] = torch.from_numpy(edit_v[a:b])
        back = wire.payloads_to_sparse(payloads, LAYOUT, splan(ratio), DEV)
        assert np.array_equal(back.idx.cpu().numpy(), ridx) and same(back.val.cpu().numpy(), rval)
    else:
        with pytest.raises(FedHipError, match=f"client {BAD_Z}: layer {name}"):
            wire.payloads_to_sparse(payloads, LAYOUT, splan(ratio), DEV)


def test_wire_payloads_round_trip_and_refusals():
    ratio = 0.5
    x, base, (ridx, rval, _, _) = problem("normal", ratio, "broadcast")
    ko = sr.koff(SEG, ratio)
    good = SparseUpdates(torch.from_numpy(ridx).to(DEV), torch.from_numpy(rval).to(DEV),
                         splan(ratio))
    payloads = wire.sparse_to_payloads(good, LAYOUT, C)
    assert len(payloads) == C
    for z, p in enumerate(payloads):
        meta = p["metadata"]
        assert meta["algorithm"] == "topk_sparsification_0.5" and meta["sparsity_ratio"] == 0.5
        for s, n in enumerate(LAYOUT.names):
            e = p["compressed_weights"][n]
            assert e["indices"].dtype == torch.int64 and e["values"].dtype == torch.float32
            assert np.array_equal(e["indices"].numpy(), ridx[z, ko[s]:ko[s + 1]])
            assert same(e["values"].numpy(), rval[z, ko[s]:ko[s + 1]])
            sp = meta["sparsification_params"][n]
            assert sp == {"original_shape": torch.Size([LENS[s]]),
                          "original_dtype": "torch.float32", "sparsity_ratio": 0.5}
    # the reference's order: by magnitude.  Shuffled segments come back sorted, bit for bit.
    rng = np.random.default_rng(0)
    for p in payloads:
        for e in p["compressed_weights"].values():
            o = torch.from_numpy(rng.permutation(e["indices"].numel()))
            e["indices"], e["values"] = e["indices"][o], e["values"][o]
    back = wire.payloads_to_sparse(payloads, LAYOUT, splan(ratio), DEV)
    assert np.array_equal(back.idx.cpu().numpy(), ridx) and same(back.val.cpu().numpy(), rval)
    bare = [p["compressed_weights"] for p in payloads]       # the dict alone is accepted too
    back = wire.payloads_to_sparse(bare, LAYOUT, splan(ratio), DEV)
    assert np.array_equal(back.idx.cpu().numpy(), ridx)
    name = LAYOUT.names[4]
    e = bare[2][name]
    e["indices"], e["values"] = e["indices"][:-1], e["values"][:-1]
    with pytest.raises(FedHipError, match=f"client 2: layer {name}.*expected k"):
        wire.payloads_to_sparse(bare, LAYOUT, splan(ratio), DEV)
    del bare[2][name]
    with pytest.raises(FedHipError, match=f"client 2: layer {name} is missing"):
        wire.payloads_to_sparse(bare, LAYOUT, splan(ratio), DEV)


# ------------------------------------------------------------------ compress_rows(sparse_out=)
@pytest.mark.parametrize("variant", VARIANTS)
def test_compress_rows_error_feedback_with_a_payload(variant):
    """Two rounds: rows and resid as without sparse_out, and the payload holds the kept v."""
    ratio = 0.9
    cfg = CompressionConfig("topk", sparsity_ratio=ratio, error_feedback=True)
    base_np = make_base("broadcast")
    base = Base(variant, np.asarray(base_np))
    rng = np.random.default_rng(12)
    resid_a = Buf(variant).put(np.zeros((C, W), F))
    resid_b = Buf(variant).put(np.zeros((C, W), F))
    resid_np = np.zeros((C, W), F)
    ko = sr.koff(SEG, ratio)
    for t in range(2):
        x_np = (base_np + (rng.standard_normal((C, W)) * 0.05).astype(F)).astype(F)
        xa, xb = Buf(variant).put(x_np), Buf(variant).put(x_np)
        idx, val, upd = payload_bufs(variant, ratio)
        compress_rows(plan(), cfg, xa.view, C, base=base.view, resid=resid_a.view)
        compress_rows(plan(), cfg, xb.view, C, base=base.view, resid=resid_b.view,
                      sparse_out=upd)
        torch.cuda.synchronize()
        for b in (xb, resid_b, idx, val):
            b.assert_poison_outside()
        assert same(xb.get(), xa.get()) and same(resid_b.get(), resid_a.get()), t
        x_out, resid_np, keep, v = er.ef_topk_round(x_np, base_np, resid_np, SEG, ratio)
        assert same(xb.get(), x_out[:, A:E]) and same(resid_b.get(), resid_np[:, A:E]), t
        ridx, rval, _ = sr.pack_rows(v, None, keep, SEG, ko)
        assert np.array_equal(idx.get(), ridx) and same(val.get(), rval), t
        out = Buf(variant)                               # the payload rebuilds the rows
        sparse_unpack_rows(upd, out.view, C, base=base.view)
        torch.cuda.synchronize()
        assert same(out.get(), xb.get()), t


@pytest.mark.parametrize("rewrite", [True, False])
def test_compress_rows_plain_with_a_payload(rewrite):
    ratio = 0.9
    cfg = CompressionConfig("topk", sparsity_ratio=ratio)
    x_np, base_np, (ridx, rval, _, _) = problem("normal", ratio, "broadcast")
    base = Base("aligned", np.asarray(base_np))
    xa, xb = Buf("aligned").put(x_np), Buf("aligned").put(x_np)
    idx, val, upd = payload_bufs("aligned", ratio)
    compress_rows(plan(), cfg, xa.view, C, base=base.view)
    compress_rows(plan(), cfg, xb.view, C, base=base.view, sparse_out=upd, rewrite_rows=rewrite)
    torch.cuda.synchronize()
    xb.assert_poison_outside()
    assert np.array_equal(idx.get(), ridx) and same(val.get(), rval)
    assert same(xb.get(), xa.get() if rewrite else np.asarray(x_np)[:, A:E])


def test_refusals():
    with pytest.raises(FedHipError, match="sparse"):
        CompressionConfig("quantization", sparse=True)
    rows = torch.zeros(C, W, device=DEV)
    _, _, upd = payload_bufs("aligned", 0.9)
    with pytest.raises(FedHipError, match="sparse_out"):
        compress_rows(plan(), CompressionConfig("quantization"), rows, C, sparse_out=upd)
    with pytest.raises(FedHipError, match="another segment plan or ratio"):
        compress_rows(plan(), CompressionConfig("topk", sparsity_ratio=0.5), rows, C,
                      sparse_out=upd)
    with pytest.raises(FedHipError, match="idx must be"):
        SparseUpdates(upd.val, upd.val, upd.plan)
    with pytest.raises(FedHipError, match="alias"):
        sparse_fedavg(upd, torch.ones(1, device=DEV), rows[0], rows[0])
    torch.cuda.synchronize()
    assert not rows.any()


# ------------------------------------------------------------------ RankRound
SIZES = [40, 33, 32, 1]


def _central_noise(P, rnd):
    return (0.002 * np.random.default_rng(900 + rnd).standard_normal(P)).astype(F)


def _run_rounds(model_name, sparse, ef, make_kw, nrounds=2):
    """Two rounds of one RankRound; per round the bits of global_flat, global_bufs, residual,
    and the last payload."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    shape = (1, 28, 28) if model_name == "simple_cnn" else (3, 32, 32)
    model = hm.ModelFactory.create_model(model_name, dropout_rate=0.0).to(DEV)
    cfg = CompressionConfig("topk", sparsity_ratio=0.9, error_feedback=ef, sparse=sparse)
    rr = RankRound(model, SIZES, list(range(4)), epochs=1, batch=32, device=DEV, lanes=1,
                   compression=cfg, dp_seed=11, shuffle_seed=5, **make_kw())
    g = torch.Generator().manual_seed(3)
    total = sum(SIZES)
    data = torch.randn(total, *shape, generator=g).to(DEV)
    lab = torch.randint(0, 10, (total,), generator=g).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in rr.slots][:-1]).tolist()
    out = []
    for t in range(nrounds):
        if rr.central is not None:
            rr.central_noise = torch.from_numpy(_central_noise(rr.P, t)).to(DEV)
        g0 = rr.global_flat.clone()
        rr.run(data, lab, offs, "sgd", 0.01, seed=t + 1)
        torch.cuda.synchronize()
        out.append(dict(glob=rr.global_flat.cpu().numpy().copy(),
                        bufs=rr.global_bufs.cpu().numpy().copy(),
                        resid=None if rr.residual is None else rr.residual.cpu().numpy().copy(),
                        g0=g0))
    return rr, out


def _route_kw(route):
    from src.aggregation import dpfedavg, fedopt, robust
    return {
        "plain": lambda: {},
        "server_opt": lambda: {"server_opt": fedopt.FedAdam(0.01, device=DEV)},
        "robust": lambda: {"aggregator": robust.MedianAggregator()},
        "robust_server_opt": lambda: {"server_opt": fedopt.FedYogi(
            0.01, base=robust.MedianAggregator(), device=DEV)},
        "central_dp": lambda: {"central_dp": dpfedavg.CentralDPConfig(
            1.1, 0.05, target_quantile=0.5, clip_lr=0.3, bit_noise=1.0)},
        "central_dp_server_opt": lambda: {
            "central_dp": dpfedavg.CentralDPConfig(1.1, 0.05, target_quantile=0.5, clip_lr=0.3,
                                                   bit_noise=1.0),
            "server_opt": fedopt.FedAdam(0.01, device=DEV)},
    }[route]


def _check_same_rounds(model_name, ef, route):
    _, dense = _run_rounds(model_name, False, ef, _route_kw(route))
    rr, sparse = _run_rounds(model_name, True, ef, _route_kw(route))
    assert rr.last_sparse is not None
    for t, (a, b) in enumerate(zip(dense, sparse)):
        assert same(a["glob"], b["glob"]), (route, t)
        assert same(a["bufs"], b["bufs"]), (route, t)
        assert (a["resid"] is None) == (not ef)
        if ef:
            assert same(a["resid"], b["resid"]), (route, t)
    assert not same(dense[0]["glob"], dense[1]["glob"])
    return rr, sparse


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("route", ["plain", "server_opt", "robust", "robust_server_opt",
                                   "central_dp", "central_dp_server_opt"])
def test_rank_round_sparse_equals_dense_simple_cnn(route, ef):
    _check_same_rounds("simple_cnn", ef, route)


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_rank_round_sparse_equals_dense_cifar10_cnn_and_wire_round_trip(ef):
    rr, rounds = _check_same_rounds("cifar10_cnn", ef, "plain")
    assert rr.Q > 0                                      # BN running statistics are aggregated
    S, L = len(rr.slots), rr.trainer.layout
    upd = rr.last_sparse
    assert upd.nclients == S and not sparse_validate(upd).cpu().numpy().any()
    payloads = wire.sparse_to_payloads(upd, L, S)
    back = wire.payloads_to_sparse(payloads, L, upd.plan, DEV)
    K = upd.plan.K
    assert torch.equal(back.idx, upd.idx[:, :K])
    assert torch.equal(back.val.view(torch.int32), upd.val[:, :K].view(torch.int32))
    # the received payload aggregates to the round's global model
    out = torch.empty(rr.P, device=DEV)
    sparse_fedavg(back, rr.w32, rounds[-1]["g0"], out, row_index=rr.rows)
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), rounds[-1]["glob"])


def test_rank_round_exact_mode_on_a_one_rank_group(tmp_path):
    """exact=True needs a process group: one gloo rank in this process (no second process; the
    two-rank layouts are tests/test_multirank_gpu.py's).  The exact route rebuilds the rows from
    the payload and all-gathers them."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        kw = lambda: {"exact": True}    # noqa: E731
        _, dense = _run_rounds("simple_cnn", False, True, kw)
        rr, sparse = _run_rounds("simple_cnn", True, True, kw)
        assert rr.exact and not rr._sparse_sum()
        for a, b in zip(dense, sparse):
            assert same(a["glob"], b["glob"]) and same(a["bufs"], b["bufs"])
            assert same(a["resid"], b["resid"])
    finally:
        dist.destroy_process_group()
