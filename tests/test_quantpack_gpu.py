"""csrc/quantpack.hip on the device: fh_quant_pack_rows, fh_quant_validate, fh_quant_unpack_rows
and fh_quant_fedavg, bit for bit against tests/quantpack_ref.py and against the kernels they stand
in for (fh_quantize_rows, fh_fedavg_weighted_sum), their chaining in compress_rows(quant_out=),
the wire payloads of fedhip/wire.py and RankRound(compression=CompressionConfig(packed=True)).

Shapes as tests/test_sparse_gpu.py: 3 client rows, segments of 1, 7, 8191, 8193 and 300 elements
behind a lead of 5 and before a tail of 9 (a last byte partly filled at every code width below 8,
a segment spanning two chunks, and a one-element segment: the pass-through case of asymmetric
mode); "aligned" parameter rows (16-byte aligned, stride a multiple of 4) and "scalar" rows
(stride W + 1, every pointer one element off); no base, one broadcast base row or one row per
client, with -0.0 in it.  Code rows are always 16-byte aligned.  Every buffer has a padding row
and is pre-filled with a NaN pattern (0xA5 for bytes); everything outside [seg_offsets[0],
seg_offsets[nseg]) of the parameter rows and outside the segments' ceil(len * cw / 8) bytes of
the code rows (their padding up to the next 16-byte boundary included) must keep it.  Inputs are
finite.  Bad payloads only ever reach fh_quant_validate and payloads_to_quant.

No tolerances: floats are compared by their int32 view."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import quantpack_ref as qr
from fedhip import ops, wire
from fedhip._lib import FedHipError
from fedhip.compress import CompressionConfig, SegmentPlan, compress_rows, quantize_rows
from fedhip.quantpack import (QuantPlan, QuantUpdates, quant_fedavg, quant_pack_rows,
                              quant_unpack_rows, quant_validate)

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
POISON_I32 = 0x7FC0BEEF          # a quiet NaN with a payload
POISON_U8 = 0xA5
VARIANTS = ["aligned", "scalar"]
MODES = ["none", "broadcast", "per_row"]
BITS = [1, 2, 3, 4, 8]
SYM = [True, False]
NEG0 = np.array([0x80000000], np.uint32).view(F)[0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_codes.json")


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
            self.flat = torch.full((n + 4,), POISON_I32, dtype=torch.int32,
                                   device=DEV).view(torch.float32)
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
        flat = self.flat if self.dtype == torch.uint8 else self.flat.view(torch.int32)
        assert bool((flat[mask] == (POISON_U8 if self.dtype == torch.uint8 else POISON_I32)).all())


class Base:
    def __init__(self, variant, arr, rows=C):
        """arr: [1, W] (broadcast, stride 0) or [rows, W]."""
        arr = np.array(arr, F)
        if arr.shape[0] == 1:
            off = 0 if variant == "aligned" else 1
            self.flat = torch.zeros(W + 4, device=DEV)
            self.flat[off:off + W] = torch.from_numpy(arr[0]).to(DEV)
            self.row = self.flat[off:off + W]
            self.view = self.row.view(1, W).expand(rows, -1)
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
def qplan(bits):
    q = QuantPlan(plan(), bits)
    assert q.cw == qr.code_width(bits) and q.boff_host == qr.boff(SEG, bits)
    assert q.seg_bytes == qr.seg_bytes(SEG, bits) and q.B == q.boff_host[-1]
    assert q.boff.dtype == torch.int64 and q.boff.cpu().tolist() == q.boff_host
    return q


class Payload:
    """Poisoned, 16-byte aligned code rows (a padding row, stride B + 16) and the three header
    tensors; only the segments' own bytes of a code row may be written."""

    def __init__(self, bits, rows=C):
        self.q = q = qplan(bits)
        self.rows, self.stride = rows, q.B + 16
        self.flat = torch.full(((rows + 1) * self.stride,), POISON_U8, dtype=torch.uint8,
                               device=DEV)
        self.full = self.flat.view(rows + 1, self.stride)
        self.scale = torch.full((rows, NSEG), -7.0, dtype=torch.float64, device=DEV)
        self.zp = torch.full((rows, NSEG), -7, dtype=torch.int64, device=DEV)
        self.passv = torch.full((rows, NSEG), POISON_I32, dtype=torch.int32,
                                device=DEV).view(torch.float32)
        self.upd = QuantUpdates(self.full[:rows, :q.B], self.scale, self.zp, self.passv, q)
        assert self.upd.codes.data_ptr() % 16 == 0 and self.upd.codes.stride(0) % 16 == 0
        m = np.ones((rows + 1, self.stride), bool)
        for a, nb in zip(q.boff_host, q.seg_bytes):
            m[:rows, a:a + nb] = False
        self.outside = torch.from_numpy(m.reshape(-1)).to(DEV)

    def put(self, packed, scale, zp, passv):
        """The segments' own bytes only: the padding keeps its poison."""
        dev = torch.from_numpy(packed).to(DEV)
        for a, nb in zip(self.q.boff_host, self.q.seg_bytes):
            self.full[:self.rows, a:a + nb] = dev[:, a:a + nb]
        self.scale.copy_(torch.from_numpy(scale))
        self.zp.copy_(torch.from_numpy(zp))
        self.passv.copy_(torch.from_numpy(np.ascontiguousarray(passv, F)))
        return self

    def codes(self):
        return self.full[:self.rows, :self.q.B].cpu().numpy()

    def assert_poison_outside(self):
        assert bool((self.flat[self.outside] == POISON_U8).all())

    def assert_equals(self, ref):
        """Byte for byte inside the segments, header bit for bit."""
        got, want = self.codes(), qr.pack_rows(ref["codes"], SEG, self.q.bits)
        for a, nb in zip(self.q.boff_host, self.q.seg_bytes):
            assert np.array_equal(got[:, a:a + nb], want[:, a:a + nb])
        assert np.array_equal(self.zp.cpu().numpy(), ref["zp"])
        live = ref["zp"] != qr.INT64_MIN          # a passed-through segment's scale is a zero
        scale = self.scale.cpu().numpy()
        assert np.array_equal(scale.view(np.int64)[live], ref["scale"].view(np.int64)[live])
        assert not scale[~live].any()
        assert same(self.passv.cpu().numpy(), ref["passv"])


@functools.lru_cache(maxsize=None)
def make_base(mode, rows=C):
    """Multiples of 2^-10 below 0.25, with -0.0 sprinkled in; None without a base."""
    if mode == "none":
        return None
    rng = np.random.default_rng(7 + (mode == "per_row"))
    b = (rng.integers(-256, 257, size=(1 if mode == "broadcast" else rows, W)) * 2.0 ** -10)
    b = b.astype(F)
    b[:, A:E:5] = NEG0
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def problem(bits, symmetric, mode, rows=C):
    """(x, base, helper quantisation).  Client 0's 7-element segment has an all-zero delta (both
    zeros without a base): code 0 and d = -0.0 in symmetric mode, passed through in asymmetric
    mode.  The last client's 300-element segment has a non-zero constant delta."""
    rng = np.random.default_rng(bits + 10 * symmetric + 100 * MODES.index(mode) + 1000 * rows)
    base = make_base(mode, rows)
    delta = (rng.standard_normal((rows, W)) * 0.05).astype(F)
    delta[0, SEG[1]:SEG[2]] = 0.0
    if base is None:
        delta[0, SEG[1]:SEG[2]:2] = NEG0
    delta[rows - 1, SEG[4]:SEG[5]] = F(-0.375)
    x = delta if base is None else (base + delta).astype(F)
    x.setflags(write=False)
    ref = qr.quantize_rows(x, base, SEG, bits, symmetric)
    if not symmetric:
        flagged = ref["zp"] == qr.INT64_MIN
        assert flagged[:, 0].all() and flagged[0, 1] and not flagged[:, 2:4].any()
        assert flagged[rows - 1, 4]                     # exact over the grid base too
    else:
        assert same(ref["d"][0, SEG[1]:SEG[2]], np.full(7, NEG0 if bits > 1 else 0.0))
    return x, base, ref


def device_pack(variant, bits, symmetric, mode):
    """fh_quantize_rows' codes and dense output, then the pack: everything the tests compare."""
    x_np, base_np, ref = problem(bits, symmetric, mode)
    base = None if base_np is None else Base(variant, np.asarray(base_np))
    bview = None if base is None else base.view
    x = Buf(variant).put(x_np)
    codes = Buf(variant, torch.uint8)
    dense = Buf(variant)
    pay = Payload(bits)
    quantize_rows(plan(), x.view, C, bits, symmetric, base=bview, out=dense.view,
                  codes=codes.view, scale_out=pay.scale, zp_out=pay.zp)
    quant_pack_rows(pay.upd, x.view, codes.view, C, base=bview)
    torch.cuda.synchronize()
    for b in (codes, dense, pay):
        b.assert_poison_outside()
    x_before = Buf(variant).put(x_np)
    assert torch.equal(x.flat.view(torch.int32), x_before.flat.view(torch.int32))
    if base is not None:
        base.assert_unchanged()
    return types.SimpleNamespace(base=base, bview=bview, x=x, codes=codes, dense=dense, pay=pay,
                                 ref=ref, base_np=base_np)


# ------------------------------------------------------------------ pack, unpack, validate
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("symmetric", SYM, ids=["sym", "asym"])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_pack_unpack_validate(variant, bits, symmetric, mode):
    d = device_pack(variant, bits, symmetric, mode)
    ref = d.ref
    m = ~_flag_mask(ref)
    assert np.array_equal(d.codes.get()[m], ref["codes"][:, A:E][m])
    d.pay.assert_equals(ref)
    assert not quant_validate(d.pay.upd).cpu().numpy().any()
    d.pay.assert_poison_outside()
    # unpack: fh_quantize_rows' own output is the yardstick
    out = Buf(variant)
    quant_unpack_rows(d.pay.upd, out.view, C, base=d.bview)
    torch.cuda.synchronize()
    out.assert_poison_outside()
    d.pay.assert_poison_outside()
    if d.base is not None:
        d.base.assert_unchanged()
    assert same(out.get(), d.dense.get())
    packed = qr.pack_rows(ref["codes"], SEG, bits)
    want = qr.unpack_rows(packed, ref["scale"], ref["zp"], ref["passv"], d.base_np, SEG, bits,
                          np.zeros((C, W), F))
    assert same(out.get(), want[:, A:E])
    if mode == "none":     # d itself: -0.0 of the all-zero symmetric segment, both zeros passed
        assert same(out.get(), ref["d"][:, A:E])
        got = out.get()[0, SEG[1] - A:SEG[2] - A]
        if symmetric and bits > 1:
            assert same(got, np.full(7, NEG0))
        if not symmetric:
            assert same(got, np.asarray(problem(bits, symmetric, mode)[0])[0, SEG[1]:SEG[2]])
            assert (i32(got) < 0).any() and (i32(got) == 0).any()


def _flag_mask(ref):
    """[C, E - A] bool: elements of passed-through segments (their one-byte codes are the
    quantiser's business, the payload ships sign bits instead)."""
    m = np.zeros((ref["zp"].shape[0], E - A), bool)
    for s, (a, e) in enumerate(zip(SEG[:-1], SEG[1:])):
        m[ref["zp"][:, s] == qr.INT64_MIN, a - A:e - A] = True
    return m


def test_unpack_in_place_over_per_row_base():
    """out may be the base rows when every client has its own."""
    d = device_pack("aligned", 4, True, "per_row")
    quant_unpack_rows(d.pay.upd, d.base.view, C, base=d.base.view)
    torch.cuda.synchronize()
    assert same(d.base.view.cpu().numpy()[:, A:E], d.dense.get())
    with pytest.raises(FedHipError, match="alias"):
        row = torch.zeros(W, device=DEV)
        quant_unpack_rows(d.pay.upd, row.view(1, W), 1, base=row.view(1, W).expand(C, -1))


BAD_Z, BAD_S = 1, 2


@pytest.mark.parametrize("kind", ["code", "code_last", "scale_nan", "scale_inf", "scale_neg",
                                  "passv_inf", "passv_nan"])
def test_validate_flags_bad_payloads(kind):
    bits = 3
    x, base, ref = problem(bits, False, "none")
    q = qplan(bits)
    packed = qr.pack_rows(ref["codes"], SEG, bits)
    scale, zp, passv = ref["scale"].copy(), ref["zp"].copy(), ref["passv"].copy()
    # garbage where nobody may look: padding bits of last bytes, padding bytes (the poison) and
    # the passv of segments that were not passed through
    for s in range(NSEG):
        used = (LENS[s] * q.cw) % 8
        a, nb = q.boff_host[s], q.seg_bytes[s]
        if used:
            packed[:, a + nb - 1] |= (0xFF << used) & 0xFF
    passv[zp != qr.INT64_MIN] = np.nan
    want = np.zeros((C, NSEG), np.int32)
    assert np.array_equal(qr.validate(packed, scale, zp, passv, SEG, bits), want)
    pay = Payload(bits).put(packed, scale, zp, passv)
    assert np.array_equal(quant_validate(pay.upd).cpu().numpy(), want)   # garbage and all
    z, s = BAD_Z, BAD_S
    if kind == "code":
        packed[z, q.boff_host[s] + 1234] |= 0x08          # an even element: code 8..15
    elif kind == "code_last":
        packed[z, q.boff_host[s] + q.seg_bytes[s] - 1] |= 0x08   # element 8190, the last one
    elif kind.startswith("scale"):
        scale[z, s] = {"scale_nan": np.nan, "scale_inf": np.inf, "scale_neg": -1e-3}[kind]
    else:
        s = 0                                             # the one-element segment is flagged
        assert zp[z, s] == qr.INT64_MIN
        passv[z, s] = np.inf if kind == "passv_inf" else np.nan
    want[z, s] = 1
    assert np.array_equal(qr.validate(packed, scale, zp, passv, SEG, bits), want)
    pay = Payload(bits).put(packed, scale, zp, passv)
    flags = torch.full((C, NSEG), -7, dtype=torch.int32, device=DEV)
    got = quant_validate(pay.upd, bad_out=flags)
    torch.cuda.synchronize()
    pay.assert_poison_outside()
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------ FedAvg from the codes
@pytest.mark.parametrize("accumulate", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("symmetric", SYM, ids=["sym", "asym"])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("nc", [1, 3, 70])
def test_quant_fedavg_equals_the_dense_sum(nc, bits, symmetric, accumulate):
    """fh_fedavg_weighted_sum over the unpacked rows is the yardstick.  70 clients over 3 payload
    rows: the row index permutes and repeats, and the prefetch ring of the client loop wraps."""
    variant = VARIANTS[(nc + bits + accumulate) % 2]
    mode = "none" if (bits + symmetric + nc) % 3 == 0 else "broadcast"
    d = device_pack(variant, bits, symmetric, mode)
    rng = np.random.default_rng(nc + 7 * bits)
    perm = np.concatenate([[2, 0, 1]] + [rng.permutation(C) for _ in range(nc // C)])[:nc]
    assert nc == 1 or not np.array_equal(perm, np.arange(nc) % C)
    w_np = (rng.random(nc) / nc + 1e-3).astype(F)
    assert (w_np.view(np.uint32) & 0xFF).any()     # full mantissas: the products are rounded
    rows = torch.zeros(C, (W + 3) // 4 * 4, device=DEV)
    quant_unpack_rows(d.pay.upd, rows, C, base=d.bview)
    w = torch.from_numpy(w_np).to(DEV)
    ri = torch.from_numpy(perm.astype(np.int32)).to(DEV)
    start = (rng.standard_normal(W) * 0.1).astype(F)
    want = torch.from_numpy(start).to(DEV)
    ops.fedavg_weighted_sum(rows, w, want, row_index=ri, accumulate=accumulate, P=E)
    out = Buf(variant, rows=1)
    out.put(start[None])
    brow = None if d.base is None else d.base.row
    quant_fedavg(d.pay.upd, w, brow, out.view[0], row_index=ri, accumulate=accumulate)
    torch.cuda.synchronize()
    out.assert_poison_outside()
    d.pay.assert_poison_outside()
    if d.base is not None:
        d.base.assert_unchanged()
    assert same(out.get()[0], want.cpu().numpy()[A:E])
    ref = d.ref
    hb = None if d.base_np is None else np.asarray(d.base_np)[0]
    href = qr.quant_fedavg(qr.pack_rows(ref["codes"], SEG, bits), ref["scale"], ref["zp"],
                           ref["passv"], w_np.tolist(), hb, SEG, bits, start,
                           row_index=perm.tolist(), accumulate=accumulate)
    assert same(out.get()[0], href[A:E])
    if not accumulate and nc == 3 and bits == 8:   # the order matters: another one, other bits
        quant_fedavg(d.pay.upd, w, brow, out.view[0])
        torch.cuda.synchronize()
        assert not same(out.get()[0], href[A:E])


# ------------------------------------------------------------------ compress_rows(quant_out=)
@pytest.mark.parametrize("symmetric", SYM, ids=["sym", "asym"])
@pytest.mark.parametrize("bits", [8, 3])
@pytest.mark.parametrize("rewrite", [True, False])
def test_compress_rows_plain_with_a_payload(rewrite, bits, symmetric):
    cfg = CompressionConfig("quantization", bits=bits, symmetric=symmetric)
    x_np, base_np, ref = problem(bits, symmetric, "broadcast")
    base = Base("aligned", np.asarray(base_np))
    xa, xb = Buf("aligned").put(x_np), Buf("aligned").put(x_np)
    pay = Payload(bits)
    compress_rows(plan(), cfg, xa.view, C, base=base.view)
    compress_rows(plan(), cfg, xb.view, C, base=base.view, quant_out=pay.upd,
                  rewrite_rows=rewrite)
    torch.cuda.synchronize()
    xb.assert_poison_outside()
    pay.assert_poison_outside()
    pay.assert_equals(ref)
    assert pay.upd.symmetric is symmetric              # recorded for the upload's metadata
    assert same(xb.get(), xa.get() if rewrite else np.asarray(x_np)[:, A:E])
    out = Buf("aligned")                               # the payload rebuilds the compressed rows
    quant_unpack_rows(pay.upd, out.view, C, base=base.view)
    torch.cuda.synchronize()
    assert same(out.get(), xa.get())


@pytest.mark.parametrize("symmetric", SYM, ids=["sym", "asym"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_compress_rows_error_feedback_with_a_payload(variant, symmetric):
    """Two rounds: rows and resid as without quant_out, and rows == fl32(base + d)."""
    cfg = CompressionConfig("quantization", bits=4, symmetric=symmetric, error_feedback=True)
    base_np = make_base("broadcast")
    base = Base(variant, np.asarray(base_np))
    rng = np.random.default_rng(12)
    resid_a = Buf(variant).put(np.zeros((C, W), F))
    resid_b = Buf(variant).put(np.zeros((C, W), F))
    for t in range(2):
        x_np = (base_np + (rng.standard_normal((C, W)) * 0.05).astype(F)).astype(F)
        xa, xb = Buf(variant).put(x_np), Buf(variant).put(x_np)
        pay = Payload(4)
        compress_rows(plan(), cfg, xa.view, C, base=base.view, resid=resid_a.view)
        compress_rows(plan(), cfg, xb.view, C, base=base.view, resid=resid_b.view,
                      quant_out=pay.upd)
        torch.cuda.synchronize()
        for b in (xb, resid_b, pay):
            b.assert_poison_outside()
        assert same(xb.get(), xa.get()) and same(resid_b.get(), resid_a.get()), t
        assert t == 0 or resid_b.get().any()
        out = Buf(variant)
        quant_unpack_rows(pay.upd, out.view, C, base=base.view)
        torch.cuda.synchronize()
        assert same(out.get(), xb.get()), t
        assert not quant_validate(pay.upd).cpu().numpy().any()


def test_refusals():
    with pytest.raises(FedHipError, match="packed"):
        CompressionConfig("topk", packed=True)
    with pytest.raises(FedHipError, match="stochastic"):
        CompressionConfig("quantization", stochastic=True, packed=True)
    with pytest.raises(FedHipError, match="bits"):
        CompressionConfig("quantization", bits=9, packed=True)
    with pytest.raises(FedHipError, match="bits"):
        QuantPlan(plan(), 9)
    rows = torch.zeros(C, W, device=DEV)
    upd = Payload(8).upd
    with pytest.raises(FedHipError, match="quant_out"):
        compress_rows(plan(), CompressionConfig("topk"), rows, C, quant_out=upd)
    with pytest.raises(FedHipError, match="stochastic"):
        compress_rows(plan(), CompressionConfig("quantization", stochastic=True), rows, C,
                      key=1, row_ids=torch.zeros(C, dtype=torch.int64, device=DEV),
                      quant_out=upd)
    with pytest.raises(FedHipError, match="bits"):
        compress_rows(plan(), CompressionConfig("quantization", bits=9), rows, C, quant_out=upd)
    with pytest.raises(FedHipError, match="another segment plan or bit width"):
        compress_rows(plan(), CompressionConfig("quantization", bits=4), rows, C, quant_out=upd)
    other = QuantPlan(SegmentPlan(SEG, DEV), 8).empty(C)          # equal, but not this plan
    with pytest.raises(FedHipError, match="another segment plan or bit width"):
        compress_rows(plan(), CompressionConfig("quantization", bits=8), rows, C,
                      quant_out=other)
    with pytest.raises(FedHipError, match="codes must be"):
        QuantUpdates(upd.passv, upd.scale, upd.zp, upd.passv, upd.plan)
    # aligned 16-byte loads are the point of the layout: the entry points refuse anything else
    q = qplan(8)
    flat = torch.zeros((C + 1) * (q.B + 16) + 16, dtype=torch.uint8, device=DEV)
    off_ptr = flat[4:4 + C * (q.B + 16)].view(C, q.B + 16)[:, :q.B]
    off_stride = flat[:C * (q.B + 8)].view(C, q.B + 8)[:, :q.B]
    assert off_ptr.data_ptr() % 16 == 4 and off_stride.stride(0) % 16 == 8
    w = torch.ones(C, device=DEV)
    out = torch.zeros(W, device=DEV)
    codes = torch.zeros(C, W, dtype=torch.uint8, device=DEV)
    for bad in (off_ptr, off_stride):
        u = QuantUpdates(bad, upd.scale, upd.zp, upd.passv, q)
        for fn in (lambda: quant_pack_rows(u, rows, codes, C),
                   lambda: quant_validate(u),
                   lambda: quant_unpack_rows(u, rows, C),
                   lambda: quant_fedavg(u, w, None, out)):
            with pytest.raises(FedHipError, match="16"):
                fn()
    with pytest.raises(FedHipError, match="alias"):
        quant_fedavg(upd, w[:1], rows[0], rows[0])
    torch.cuda.synchronize()
    assert not rows.any() and not out.any() and not flat.any()


# ------------------------------------------------------------------ wire payloads
LAYOUT = types.SimpleNamespace(names=[f"layer{s}.weight" for s in range(NSEG)],
                               shapes=[(n,) if n != 300 else (3, 100) for n in LENS])


@pytest.mark.parametrize("bits", BITS)
def test_wire_payloads_round_trip(bits):
    d = device_pack("aligned", bits, True, "broadcast")
    ref = d.ref
    with pytest.raises(FedHipError, match="mode is not recorded"):   # never guessed from zp
        wire.quant_to_payloads(d.pay.upd, LAYOUT, C)
    payloads = wire.quant_to_payloads(d.pay.upd, LAYOUT, C, symmetric=True)
    assert len(payloads) == C
    for z, p in enumerate(payloads):
        meta = p["metadata"]
        assert meta["algorithm"] == f"quantization_{bits}bit" and meta["bits"] == bits
        assert meta["symmetric"] is True
        for s, n in enumerate(LAYOUT.names):
            t = p["compressed_weights"][n]
            assert t.dtype == torch.uint8 and tuple(t.shape) == tuple(LAYOUT.shapes[s])
            assert np.array_equal(t.reshape(-1).numpy(), ref["codes"][z, SEG[s]:SEG[s + 1]])
            assert meta["quantization_params"][n] == {
                "scale": float(ref["scale"][z, s]), "zero_point": int(ref["zp"][z, s]),
                "original_shape": torch.Size(LAYOUT.shapes[s]), "original_dtype": "torch.float32"}
    for form in (payloads, [{"compressed_weights": p["compressed_weights"],
                             "quantization_params": p["metadata"]["quantization_params"]}
                            for p in payloads]):
        back = wire.payloads_to_quant(form, LAYOUT, qplan(bits), DEV)
        assert back.codes.data_ptr() % 16 == 0
        assert back.symmetric is (True if form is payloads else None)   # the metadata's, or unknown
        got, want = back.codes.cpu().numpy(), d.pay.codes()
        for a, nb in zip(qplan(bits).boff_host, qplan(bits).seg_bytes):
            assert np.array_equal(got[:, a:a + nb], want[:, a:a + nb])
        assert torch.equal(back.scale.view(torch.int64), d.pay.scale.view(torch.int64))
        assert torch.equal(back.zp, d.pay.zp)
        out = Buf("aligned")
        quant_unpack_rows(back, out.view, C, base=d.bview)
        torch.cuda.synchronize()
        assert same(out.get(), d.dense.get())


def test_wire_refusals():
    bits = 3
    flagged = device_pack("aligned", bits, False, "broadcast")
    with pytest.raises(FedHipError, match=f"client 0: layer {LAYOUT.names[0]}"):
        wire.quant_to_payloads(flagged.pay.upd, LAYOUT, C, symmetric=False)
    d = device_pack("aligned", bits, True, "broadcast")
    q = qplan(bits)
    name = LAYOUT.names[4]

    def fresh():
        return wire.quant_to_payloads(d.pay.upd, LAYOUT, C, symmetric=True)
    p = fresh()
    p[2]["compressed_weights"][name] = p[2]["compressed_weights"][name].reshape(-1)
    with pytest.raises(FedHipError, match=f"client 2: layer {name} has shape"):
        wire.payloads_to_quant(p, LAYOUT, q, DEV)
    p = fresh()
    p[2]["compressed_weights"][name] = p[2]["compressed_weights"][name].to(torch.int16)
    with pytest.raises(FedHipError, match=f"client 2: layer {name} has dtype"):
        wire.payloads_to_quant(p, LAYOUT, q, DEV)
    p = fresh()
    del p[2]["compressed_weights"][name]
    with pytest.raises(FedHipError, match=f"client 2: layer {name} is missing"):
        wire.payloads_to_quant(p, LAYOUT, q, DEV)
    for code in (9, 200):            # what fh_quant_validate flags, and what no nibble holds
        p = fresh()
        p[1]["compressed_weights"][name][1, 7] = code
        with pytest.raises(FedHipError, match=f"client 1: layer {name} has a code >= 2\\^3"):
            wire.payloads_to_quant(p, LAYOUT, q, DEV)
    p = fresh()
    p[1]["metadata"]["quantization_params"][name]["scale"] = float("nan")
    with pytest.raises(FedHipError, match=f"client 1: layer {name}.*scale"):
        wire.payloads_to_quant(p, LAYOUT, q, DEV)


@pytest.mark.parametrize("bits", [5, 6, 7])
def test_codes_out_of_range_where_a_byte_holds_one_code(bits):
    """cw = 8 with bits < 8: no host check can see a code >= 2^bits, only fh_quant_validate."""
    q = QuantPlan(plan(), bits)
    assert q.cw == 8 and q.boff_host == qr.boff(SEG, bits)
    rng = np.random.default_rng(bits)
    x = (rng.standard_normal((C, W)) * 0.05).astype(F)
    ref = qr.quantize_rows(x, None, SEG, bits, True)
    assert 2 ** (bits - 1) < ref["codes"].max() < 2 ** bits
    packed = qr.pack_rows(ref["codes"], SEG, bits)

    def device(pk):
        codes = torch.full((C + 1, q.B + 16), POISON_U8, dtype=torch.uint8, device=DEV)
        dev = torch.from_numpy(pk).to(DEV)
        for a, nb in zip(q.boff_host, q.seg_bytes):      # the padding keeps its poison
            codes[:C, a:a + nb] = dev[:, a:a + nb]
        return QuantUpdates(codes[:C, :q.B], torch.from_numpy(ref["scale"]).to(DEV),
                            torch.from_numpy(ref["zp"]).to(DEV),
                            torch.from_numpy(ref["passv"]).to(DEV), q)
    assert not quant_validate(device(packed)).cpu().numpy().any()
    # the vector body, the byte tail behind it and the one-byte segment
    for z, s, at in [(1, 3, 4097), (2, 2, 8190), (0, 0, 0), (1, 4, 299)]:
        for code in (2 ** bits, 255):
            bad = packed.copy()
            bad[z, q.boff_host[s] + at] = code
            want = np.zeros((C, NSEG), np.int32)
            want[z, s] = 1
            assert np.array_equal(qr.validate(bad, ref["scale"], ref["zp"], ref["passv"], SEG,
                                              bits), want)
            assert np.array_equal(quant_validate(device(bad)).cpu().numpy(), want)
    good = device(packed)
    good.symmetric = True
    payloads = wire.quant_to_payloads(good, LAYOUT, C)
    assert wire.payloads_to_quant(payloads, LAYOUT, q, DEV).symmetric is True
    name = LAYOUT.names[3]
    payloads[2]["compressed_weights"][name][8192] = 2 ** bits
    with pytest.raises(FedHipError, match=f"client 2: layer {name} has a code >= 2\\^{bits}"):
        wire.payloads_to_quant(payloads, LAYOUT, q, DEV)


def test_wire_golden_cases_round_trip_to_the_references_bits():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["cases"]) == 25
    for name, c in sorted(g["cases"].items()):
        n, bits = c["numel"], c["bits"]
        layout = types.SimpleNamespace(names=["w"], shapes=[(n,)])
        q = QuantPlan(SegmentPlan([0, n], DEV), bits)
        payload = {"compressed_weights": {"w": torch.tensor(c["codes"], dtype=torch.uint8)},
                   "quantization_params": {"w": {"scale": float.fromhex(c["scale_hex"]),
                                                 "zero_point": c["zero_point"]}}}
        upd = wire.payloads_to_quant([payload], layout, q, DEV)
        out = torch.full((1, n + 4), float("nan"), device=DEV)
        quant_unpack_rows(upd, out, 1)
        acc = torch.zeros(n, device=DEV)
        quant_fedavg(upd, torch.ones(1, device=DEV), None, acc)
        torch.cuda.synchronize()
        want = np.array(c["dense_u32"], np.uint32)
        assert np.array_equal(out[0, :n].cpu().numpy().view(np.uint32), want), name
        assert bool(out[0, n:].isnan().all())
        # 1.0 * d added to +0.0: d, but for -0.0, which the sum's +0.0 start absorbs
        got = acc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.where(want == 0x80000000, 0, want)), name
        back = wire.quant_to_payloads(upd, layout, 1, symmetric=c["symmetric"])[0]
        assert back["compressed_weights"]["w"].tolist() == c["codes"]
        assert back["metadata"]["symmetric"] is c["symmetric"]
        assert back["metadata"]["quantization_params"]["w"]["scale"].hex() == c["scale_hex"]


# ------------------------------------------------------------------ RankRound
SIZES = [40, 33, 32, 1]


def _central_noise(P, rnd):
    return (0.002 * np.random.default_rng(900 + rnd).standard_normal(P)).astype(F)


def _run_rounds(packed, ef, make_kw, nrounds=2):
    """Two rounds of one RankRound; per round the bits of global_flat, global_bufs, residual, the
    rows after the round and the global model it started from."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn", dropout_rate=0.0).to(DEV)
    cfg = CompressionConfig("quantization", bits=8, error_feedback=ef, packed=packed)
    rr = RankRound(model, SIZES, list(range(4)), epochs=1, batch=32, device=DEV, lanes=1,
                   compression=cfg, dp_seed=11, shuffle_seed=5, **make_kw())
    g = torch.Generator().manual_seed(3)
    total = sum(SIZES)
    data = torch.randn(total, 1, 28, 28, generator=g).to(DEV)
    lab = torch.randint(0, 10, (total,), generator=g).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in rr.slots][:-1]).tolist()
    out = []
    for t in range(nrounds):
        if rr.central is not None:
            rr.central_noise = torch.from_numpy(_central_noise(rr.P, t)).to(DEV)
        g0 = rr.global_flat.clone()
        rr.run(data, lab, offs, "sgd", 0.01, seed=t + 1)
        torch.cuda.synchronize()
        S = len(rr.slots)
        out.append(dict(glob=rr.global_flat.cpu().numpy().copy(),
                        bufs=rr.global_bufs.cpu().numpy().copy(),
                        resid=None if rr.residual is None else rr.residual.cpu().numpy().copy(),
                        rows=rr.trainer.params[:S, :rr.P].cpu().numpy().copy(), g0=g0))
    return rr, out


def _route_kw(route):
    from src.aggregation import dpfedavg, fedopt, robust
    return {
        "plain": lambda: {},
        "server_opt": lambda: {"server_opt": fedopt.FedAdam(0.01, device=DEV)},
        "robust": lambda: {"aggregator": robust.MedianAggregator()},
        "central_dp": lambda: {"central_dp": dpfedavg.CentralDPConfig(
            1.1, 0.05, target_quantile=0.5, clip_lr=0.3, bit_noise=1.0)},
    }[route]


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("route", ["plain", "server_opt", "robust", "central_dp"])
def test_rank_round_packed_equals_unpacked(route, ef):
    _, dense = _run_rounds(False, ef, _route_kw(route))
    rr, packed = _run_rounds(True, ef, _route_kw(route))
    assert rr.last_quant is not None
    assert rr._quant_sum() == (route in ("plain", "server_opt"))
    for t, (a, b) in enumerate(zip(dense, packed)):
        assert same(a["glob"], b["glob"]), (route, t)
        assert same(a["bufs"], b["bufs"]), (route, t)
        assert (a["resid"] is None) == (not ef)
        if ef:
            assert same(a["resid"], b["resid"]), (route, t)
    assert not same(dense[0]["glob"], dense[1]["glob"])
    # the payload of the last round unpacks to the rows packed=False aggregated
    S = len(rr.slots)
    upd = rr.last_quant
    assert upd.nclients == S and not quant_validate(upd).cpu().numpy().any()
    g0 = packed[-1]["g0"]
    rows = torch.zeros(S, (rr.P + 3) // 4 * 4, device=DEV)
    quant_unpack_rows(upd, rows, S, base=g0.view(1, -1).expand(S, -1))
    torch.cuda.synchronize()
    assert same(rows[:, :rr.P].cpu().numpy(), dense[-1]["rows"])
    if rr._quant_sum() and not ef:      # the plain routes leave the rows as trained
        assert not same(packed[-1]["rows"], dense[-1]["rows"])
    if route == "plain":                # the uploads, received again, aggregate to the global
        L = rr.trainer.layout
        back = wire.payloads_to_quant(wire.quant_to_payloads(upd, L, S), L, upd.plan, DEV)
        out = torch.empty(rr.P, device=DEV)
        quant_fedavg(back, rr.w32, g0, out, row_index=rr.rows)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), packed[-1]["glob"])
