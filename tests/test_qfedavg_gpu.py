"""fh_qfedavg_rows (csrc/qfedavg.hip), QFedAvgAggregator and RankRound(qfedavg=) on the GPU,
against the numpy reference of tests/qfedavg_ref.py (pinned by test_qfedavg_ref_cpu.py).

What is fp32 is held bit for bit (uint32 views): PARTIAL's out is the reference sum; STEP's out is
the reference finish applied to the reference sum and the kernel's OWN reported den.  What is an
fp64 sum (sqdist, den) differs from numpy's only by the order of the additions and is held to a
derived bound: a sum of n non-negative fp64 terms in any order is within (n-1) * 2^-53 * sum of
the exact sum, the squares of fp32 differences are exact in fp64, so two orders differ by at most
2 * P * 2^-53 * sum (SQ_TOL); den adds per client one product, one sum and C - 1 additions of
non-negative terms: (2 * P + 2 * C + 4) * 2^-53 * den (DEN_TOL).  Neither was tuned on the GPU.

Shapes: client counts on both sides of every register-slot count and vector width (16 bytes up
to 16 clients, 8 bytes up to 32, scalar above); sizes below, at and above the vector width, the
256-thread tile and a workgroup's columns per tile (256 * 4, 256 * 2, 256), and one size of
several workgroups with a tail.
"""
import os
import queue
import time
from datetime import datetime

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fednova_ref as nr
import fedopt_ref as fr
import qfedavg_ref as qr
from fedhip import ops
from fedhip._lib import FedHipError, call, ptr, stream_handle
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgAggregator, FedAvgError
from src.aggregation.qfedavg import QFedAvgAggregator, QFedAvgConfig
from src.shared.models import GlobalModel, ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
F, D = np.float32, np.float64

CS = [1, 2, 3, 16, 17, 33, 64]
PS = [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3 * 1024 + 7]


def _np(t):
    return t.detach().cpu().numpy()


def _sq_tol(P, want):
    return 2 * P * 2.0 ** -53 * want


def _den_tol(C, P, want):
    return (2 * P + 2 * C + 4) * 2.0 ** -53 * want


def _data(C, P, seed, zeros=True):
    """(rows, a fp32, b fp64, g): rows around g at mixed magnitudes, some denormals in both;
    positive coefficients, with exact zeros (+0 and -0) among them when C allows."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 1, P)).astype(F)
    rows = (g + rng.standard_normal((C, P)) * 10.0 ** rng.uniform(-4, 0, (C, 1))).astype(F)
    den_bits = rng.integers(1, 1 << 22, size=P).astype(np.uint32).view(F)
    g[::11] = den_bits[::11]                           # denormal globals
    rows[rng.integers(C), ::5] = -den_bits[::5]        # a row with denormals
    a = (rng.uniform(0.05, 1.0, C) / C).astype(F)
    b = rng.uniform(0.0, 3.0, C).astype(D)
    if zeros and C >= 3:
        k = rng.permutation(C)[:2]
        a[k[0]], a[k[1]] = 0.0, -0.0
    return rows, a, b, g


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show)."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


def _window(P, offset, fill=None):
    buf = torch.full((P + 16,), SENTINEL, device=DEV)
    view = buf[offset:offset + P]
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return buf, view


def _intact(buf, offset, P):
    b = _np(buf)
    return (b[:offset] == SENTINEL).all() and (b[offset + P:] == SENTINEL).all()


def _run(mode, view, a, b, g, goff=0, ooff=4, row_index=None, alias=False, state=None):
    """One fh_qfedavg_rows into a sentinel window -> (out, sqdist, den, live) as numpy."""
    P = view.shape[1]
    a32 = None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(DEV)
    b64 = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=D)).to(DEV)
    gbuf, gd = _window(P, goff, fill=g)
    buf, out = (gbuf, gd) if alias else _window(P, ooff)
    got, sq, st = ops.qfedavg_rows(view, a32, b64, gd, out, mode, row_index=row_index,
                                   state=state)
    torch.cuda.synchronize()
    assert got is out and _intact(buf, goff if alias else ooff, P)
    if not alias:
        assert qr.same_bits(_np(gd), g) and _intact(gbuf, goff, P)
    st = _np(st)
    return _np(out).copy(), None if sq is None else _np(sq), st[0], st[1]


def _check(rows, a, b, g, view, tag, **kw):
    """PARTIAL and STEP on one layout against the reference; returns STEP's out."""
    C, P = rows.shape
    acc, sq, den = qr.qfedavg_rows(qr.PARTIAL, rows, a, b, g)
    live = int(np.count_nonzero(np.asarray(a, dtype=F)))
    p_out, p_sq, p_den, p_live = _run(qr.PARTIAL, view, a, b, g, **kw)
    assert qr.same_bits(p_out, acc), tag
    assert (np.abs(p_sq - sq) <= _sq_tol(P, sq)).all(), (tag, p_sq, sq)
    assert abs(p_den - den) <= _den_tol(C, P, den) and p_live == live, (tag, p_den, den)
    s_out, s_sq, s_den, s_live = _run(qr.STEP, view, a, b, g, **kw)
    assert (np.abs(s_sq - sq) <= _sq_tol(P, sq)).all(), (tag, s_sq, sq)
    assert abs(s_den - den) <= _den_tol(C, P, den) and s_live == live, (tag, s_den, den)
    if kw.get("ooff", 4) % 4 == 0:
        # acc goes to the workspace in STEP and to out in PARTIAL; with both 16-byte aligned
        # the two modes take the same path: the same launches, the same fp64 bits
        assert np.array_equal(s_sq.view(np.uint64), p_sq.view(np.uint64)), tag
        assert D(s_den).view(np.uint64) == D(p_den).view(np.uint64), tag
    assert qr.same_bits(s_out, qr.finish(acc, g, s_den)), tag
    return s_out


@pytest.mark.parametrize("C", CS)
def test_qfedavg_bits(C):
    for P in PS:
        rows, a, b, g = _data(C, P, 1000 * C + P)
        vec = _place(rows, (P + 3) // 4 * 4 + 4, 0)    # stride % 4 == 0, > P: vector + tail
        sca = _place(rows, (P + 2) | 1, 0)             # odd stride > P: scalar path
        outs = [_check(rows, a, b, g, v, (C, P, v.stride(0))) for v in (vec, sca)]
        assert qr.same_bits(outs[0], outs[1]), (C, P)  # vector and scalar paths: the same bits
    if C == 64:
        # The smallest shape with two tiles per workgroup: the 64-slot scalar instance (at most
        # 512 workgroups, one column per thread) over 512 * 256 + 257 columns is 514 tiles on 257
        # workgroups, the last tile partial.
        P = 512 * 256 + 257
        rows, a, b, g = _data(C, P, 1000 * C + P)
        _check(rows, a, b, g, _place(rows, (P + 2) | 1, 0), (C, P, "two tiles"))


@pytest.mark.parametrize("C", [1, 2, 5, 33])
def test_qfedavg_step_within_fp32_tolerance_of_fp64(C):
    """STEP against the rule evaluated in fp64 from the same fp32 inputs.  Every input term
    passes through at most C + 4 fp32 roundings on its way to out[j] (its subtract, its multiply,
    at most C - 1 inexact adds, the rounding of 1/den, the multiply by it, the final add), each
    of relative size 2^-24, and |x - g| <= |x| + |g|.  The contract's den sums squares of the
    ROUNDED fp32 differences where the fp64 evaluation squares exact ones: each square, and so
    the sum of these non-negative terms, is off by at most 2^-23 relative (beside DEN_TOL and a
    denormal-range term far below one ulp of den).  Through 1/den that is two more units of 2^-24
    on the step: C + 6; 1.01 covers the second-order terms.  The data hold denormals, and a
    result in the denormal range is rounded to a multiple of 2^-149 instead: an absolute error
    of up to 2^-150 per operation, which the second term covers."""
    P = 4001
    rows, a, b, g = _data(C, P, 40 + C, zeros=False)
    got, _, den, _ = _run(qr.STEP, _place(rows, 4004, 0), a, b, g)
    want, den64 = qr.rule_fp64(rows, a, b, g)
    assert abs(den - den64) <= 1.01 * 2.0 ** -23 * den64 + _den_tol(C, P, den64)
    r64, g64, a64 = rows.astype(D), g.astype(D), a.astype(D)
    bound = 1.01 * (C + 6) * 2.0 ** -24 * (
        np.abs(g64) + (a64[:, None] * (np.abs(r64) + np.abs(g64))).sum(0) / den64) \
        + (C + 4) * 2.0 ** -150
    err = np.abs(got.astype(D) - want)
    print(f"C={C}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("C", [3, 17, 33])
def test_row_index_misalignment_aliasing_and_replay(C):
    P, tall = 1001, C + 5
    rng = np.random.default_rng(C)
    rows, _, _, g = _data(tall, P, 77 + C)
    _, a, b, _ = _data(C, P, 78 + C)
    pick = rng.permutation(tall)[:C]               # a subset of a taller matrix, permuted
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    aligned = _place(rows, 1008, 0)
    want = _check(rows[pick], a, b, g, aligned, ("aligned", C), row_index=idx)
    # the same call again: the same bits, fp64 included
    o1, sq1, den1, _ = _run(qr.STEP, aligned, a, b, g, row_index=idx)
    o2, sq2, den2, _ = _run(qr.STEP, aligned, a, b, g, row_index=idx)
    assert qr.same_bits(o1, want) and qr.same_bits(o2, want)
    assert np.array_equal(sq1.view(np.uint64), sq2.view(np.uint64))
    assert D(den1).view(np.uint64) == D(den2).view(np.uint64)
    for view, kw in ((_place(rows, 1008, 1), {}),             # rows + 4 B: scalar path
                     (aligned, {"ooff": 1}),                   # out + 4 B
                     (aligned, {"goff": 3}),                   # global + 12 B
                     (_place(rows, 1003, 0), {})):             # odd stride
        got = _check(rows[pick], a, b, g, view, (C, kw), row_index=idx, **kw)
        assert qr.same_bits(got, want), (C, kw)
    # STEP with out aliased to global, on both apply paths: the bits of a separate out
    for off in (0, 1):
        got = _run(qr.STEP, aligned, a, b, g, row_index=idx, alias=True, goff=off)[0]
        assert qr.same_bits(got, want), off
    # the identity index against no index (the first C rows of the taller matrix)
    ident = torch.arange(C, dtype=torch.int32, device=DEV)
    w0 = _run(qr.STEP, aligned, a, b, g)[0]
    assert qr.same_bits(_run(qr.STEP, aligned, a, b, g, row_index=ident)[0], w0)


@pytest.mark.parametrize("C", [3, 17, 64])
def test_nan_row_with_zero_coefficient_and_all_zero(C):
    P = 1030
    rows, a, b, g = _data(C, P, 5 + C)
    dead = [int(k) for k in np.flatnonzero(a == 0)]
    bad = rows.copy()
    bad[dead[0], 7] = np.nan
    bad[dead[1], :] = np.inf
    bad[dead[1], ::2] = -np.inf
    for stride in (1032, 1031):    # the vector and the scalar path, each against itself
        clean = _run(qr.STEP, _place(rows, stride, 0), a, b, g)
        out, sq, den, live = _run(qr.STEP, _place(bad, stride, 0), a, b, g)
        assert qr.same_bits(out, clean[0])
        assert D(den).view(np.uint64) == D(clean[2]).view(np.uint64) and live == C - 2
        assert np.isnan(sq[dead[0]]) and not np.isfinite(sq[dead[1]])
        alive = np.ones(C, dtype=bool)
        alive[dead] = False
        assert np.array_equal(sq[alive].view(np.uint64), clean[1][alive].view(np.uint64))
    # all a = 0: out == g bitwise (NaN payloads in g included), no live client, den = 0
    g2 = g.copy()
    g2[:4] = np.array([0xFFA5A5A5, 0x7F800001, 0x80000000, 0x00000001], dtype=np.uint32).view(F)
    zero = np.zeros(C, dtype=F)
    zero[::2] = -0.0
    for alias in (False, True):
        out, sq, den, live = _run(qr.STEP, _place(bad, 1032, 0), zero, b, g2, alias=alias)
        assert qr.same_bits(out, g2) and den == 0.0 and live == 0


def test_partial_partial_finish_composition():
    """Two groups of clients as two ranks would hold them: the partial sums added in fp32, the
    dens in fp64, FINISH.  Bit for bit the reference run the same way (given the kernel's dens);
    against one STEP over all clients only to tolerance, the split changes the summation order."""
    C, P = 11, 2051
    rows, a, b, g = _data(C, P, 9)
    view = _place(rows, 2052, 0)
    groups = [[0, 3, 4, 9, 10], [1, 2, 5, 6, 7, 8]]
    parts, dens, ref_parts = [], [], []
    for grp in groups:
        idx = torch.tensor(grp, dtype=torch.int32, device=DEV)
        out, _, den, _ = _run(qr.PARTIAL, view, a[grp], b[grp], g, row_index=idx)
        ref = qr.qfedavg_rows(qr.PARTIAL, rows[grp], a[grp], b[grp], g)
        assert qr.same_bits(out, ref[0]) and abs(den - ref[2]) <= _den_tol(C, P, ref[2])
        parts.append(out), dens.append(den), ref_parts.append(ref[0])
    total, den = parts[0] + parts[1], D(dens[0]) + D(dens[1])
    assert total.dtype == F
    state = torch.tensor([den, 0.0], dtype=torch.float64, device=DEV)
    want = qr.qfedavg_rows(qr.FINISH, ref_parts[0] + ref_parts[1], None, None, g, den=den)[0]
    for stride, ooff in ((2052, 4), (2051, 1)):
        got = _run(qr.FINISH, _place(total[None], stride, 0), None, None, g, ooff=ooff,
                   state=state)
        assert got[1] is None and got[2] == den
        assert qr.same_bits(got[0], want)
    # FINISH in place: out is the global vector, or the row itself
    for which in ("global", "rows"):
        row = _place(total[None], 2052, 0)
        gd = torch.from_numpy(g).to(DEV)
        out = gd if which == "global" else row[0]
        ops.qfedavg_rows(row, None, None, gd, out, ops.QFA_FINISH, state=state)
        assert qr.same_bits(_np(out), want), which
    step, _, den_s, _ = _run(qr.STEP, view, a, b, g)
    assert abs(den_s - den) <= _den_tol(C, P, den_s)
    tol = 1.01 * (C + 4) * 2.0 ** -23 * (np.abs(g.astype(D)) + (
        a.astype(D)[:, None] * (np.abs(rows.astype(D)) + np.abs(g.astype(D)))).sum(0) / den_s) \
        + (C + 4) * 2.0 ** -149
    assert (np.abs(step.astype(D) - want.astype(D)) <= tol).all()  # both within the fp64 bound


def test_qfedavg_argument_errors():
    rows = torch.zeros(65, 8, device=DEV)
    g = torch.zeros(8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    sq = torch.full((65,), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.full((2,), SENTINEL, dtype=torch.float64, device=DEV)
    a = torch.ones(65, device=DEV)
    b = torch.ones(65, dtype=torch.float64, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def raw(C=3, P=8, mode=0, rows_p=ptr(rows), a_p=ptr(a), b_p=ptr(b), g_p=ptr(g),
            out_p=ptr(out), ws_p=ptr(ws), ws_n=1 << 16, sq_p=ptr(sq), st_p=ptr(st)):
        call("fh_qfedavg_rows", rows_p, 8, None, a_p, b_p, C, P, g_p, mode, out_p, ws_p, ws_n,
             sq_p, st_p, stream_handle())

    for kw, msg in ((dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(C=0), "outside"),
                    (dict(C=65), "outside"), (dict(C=2, mode=2), "FINISH"),
                    (dict(C=0, mode=2), "FINISH"), (dict(P=-1), "bad sizes"),
                    (dict(st_p=None), "null state"), (dict(st_p=None, mode=2, C=1), "null state"),
                    (dict(a_p=None), "null"), (dict(b_p=None), "null"), (dict(sq_p=None), "null"),
                    (dict(a_p=None, P=0), "null"), (dict(rows_p=None), "null"),
                    (dict(g_p=None), "null"), (dict(out_p=None), "null"),
                    (dict(rows_p=None, mode=2, C=1), "null"), (dict(g_p=None, mode=2, C=1), "null"),
                    (dict(out_p=None, mode=2, C=1), "null"), (dict(ws_n=8), "workspace"),
                    (dict(ws_p=None), "workspace"), (dict(ws_p=ptr(ws) + 4), "workspace"),
                    (dict(mode=1, ws_n=8), "workspace"), (dict(mode=1, out_p=ptr(g)), "PARTIAL")):
        with pytest.raises(FedHipError, match=msg):
            raw(**kw)
    with pytest.raises(FedHipError, match="outside"):
        ops.qfedavg_rows(rows, a, b, g, out, ops.QFA_STEP)
    with pytest.raises(FedHipError, match="HIP device"):
        ops.qfedavg_rows(torch.zeros(3, 8), a[:3], b[:3], g, out, ops.QFA_STEP)
    with pytest.raises(FedHipError, match="FINISH"):
        ops.qfedavg_rows(rows[:1], a[:1], None, g, out, ops.QFA_FINISH, state=st)
    with pytest.raises(FedHipError, match="ONE row"):
        ops.qfedavg_rows(rows[:2], None, None, g, out, ops.QFA_FINISH, state=st)
    assert ops.qfedavg_workspace(0, 8) == 0 and ops.qfedavg_workspace(65, 8) == 0
    assert ops.qfedavg_workspace(3, 0) == 0 and ops.qfedavg_workspace(3, 8) >= 8 * 4 + 3 * 8
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all() and (_np(sq) == SENTINEL).all()
    assert (_np(st) == SENTINEL).all()
    # P == 0: den from the a_k alone, zero distances, no out; FINISH with P == 0 is a no-op
    a3 = torch.tensor([0.5, 0.0, 0.25], device=DEV)
    _, z, s = ops.qfedavg_rows(rows[:3], a3, b[:3], g, out, ops.QFA_STEP, P=0, sqdist=sq[:3],
                               state=st)
    torch.cuda.synchronize()
    assert _np(z).tolist() == [0.0] * 3 and _np(s).tolist() == [0.75, 2.0]
    raw(C=1, P=0, mode=2)
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all()


# ------------------------------------------------------------------ the aggregator
SHAPES = {"conv.weight": (4, 1, 3, 3), "fc.bias": (5,)}


def _flat(weights):
    return np.concatenate([_np(weights[n]).reshape(-1) for n in SHAPES])


def test_aggregate_updates_and_packed_against_the_reference():
    gen = torch.Generator().manual_seed(4)
    prev_w = {name: 0.3 * torch.randn(*shape, generator=gen) for name, shape in SHAPES.items()}
    prev = GlobalModel(round_number=3, model_weights=prev_w, accuracy_metrics={},
                       participating_clients=[], convergence_score=0.0)
    ups, samples, train_loss, exact_loss = [], [10, 11, 12], [0.5, 2.0, 0.1], [0.7, 1.9, 0.4]
    for k in range(3):
        wts = {name: t + 0.05 * torch.randn(*t.shape, generator=gen)
               for name, t in prev_w.items()}
        ups.append(ModelUpdate(client_id=f"c{k}", round_number=4, model_weights=wts,
                               num_samples=samples[k], training_loss=train_loss[k],
                               privacy_budget_used=0.5, compression_ratio=0.8,
                               timestamp=datetime.now()))
    rows = np.stack([_flat(u.model_weights) for u in ups])
    g0 = _flat(prev_w)
    C, P = rows.shape
    L = 100.0

    def want(pi, losses, q, den):
        a, b = qr.coefficients(pi, losses, q, L)
        acc, _, ref_den = qr.qfedavg_rows(qr.PARTIAL, rows, a, b, g0)
        assert abs(den - ref_den) <= _den_tol(C, P, ref_den)
        return qr.finish(acc, g0, den)

    uniform, by_samples = [1.0 / 3] * 3, [n / 33 for n in samples]
    agg = QFedAvgAggregator(device=DEV, q=1.0, keep_stats=True)
    for losses, ref_losses in ((None, train_loss), ({"c2": 0.4, "c0": 0.7, "c1": 1.9, "x": 9.0},
                                                    exact_loss), (exact_loss, exact_loss)):
        gm = agg.aggregate_updates(ups, prev, L, losses=losses)
        assert gm.round_number == 4 and gm.participating_clients == ["c0", "c1", "c2"]
        assert [gm.model_weights[n].shape for n in SHAPES] == \
            [torch.Size(s) for s in SHAPES.values()]
        assert qr.same_bits(_flat(gm.model_weights), want(uniform, ref_losses, 1.0, agg.last_den))
        assert qr.same_bits(_flat(prev_w), g0)   # the global model is not stepped in place
        assert len(agg.last_sqdist) == 3
    assert agg.aggregation_history[-1]["client_samples"]["c2"] == 12
    # the default keeps no statistics: no device read
    quiet = QFedAvgAggregator(device=DEV, q=2.0, weights="samples")
    gm = quiet.aggregate_updates(ups, prev, L)
    assert quiet.last_den is None and quiet.last_sqdist is None
    keep = QFedAvgAggregator(device=DEV, q=2.0, weights="samples", keep_stats=True)
    gm2 = keep.aggregate_updates(ups, prev, L)
    assert qr.same_bits(_flat(gm.model_weights), _flat(gm2.model_weights))
    assert qr.same_bits(_flat(gm2.model_weights), want(by_samples, train_loss, 2.0, keep.last_den))
    # q = 0 with the sample weights is FedAvg in delta form: a = w, b = 0, den = sum of the fp32
    # weights.  Against FedAvgAggregator within the roundings of both forms: C + 4 on the delta
    # side (see the fp64 test), C + 1 on FedAvg's, on terms of size w_k * (|x| + |g|) and |g|;
    # the fp32 weights sum to 1 + e, |e| <= C * 2^-25, and the delta form divides by that sum
    # where FedAvg does not: C / 2 more units of 2^-24, rounded up to C
    q0 = QFedAvgAggregator(device=DEV, q=0, weights="samples", keep_stats=True)
    got = _flat(q0.aggregate_updates(ups, prev, L).model_weights)
    assert qr.same_bits(got, want(by_samples, train_loss, 0, q0.last_den))
    plain = _flat(FedAvgAggregator(device=DEV).aggregate_updates(ups).model_weights)
    w64 = np.asarray(by_samples)
    mag = np.abs(g0.astype(D)) + (
        w64[:, None] * (np.abs(rows.astype(D)) + np.abs(g0.astype(D)))).sum(0)
    assert (np.abs(got.astype(D) - plain.astype(D)) <= 1.01 * (3 * C + 5) * 2.0 ** -24 * mag).all()
    # aggregate_packed: rows already on the device, a permuted subset, out = global in place
    packed = _place(np.concatenate([rows, rows[::-1]]), 48, 0)
    gd = torch.from_numpy(g0).to(DEV)
    got = agg.aggregate_packed(packed, samples, exact_loss, gd, L, row_index=[5, 4, 3])
    assert qr.same_bits(_np(got), want(uniform, exact_loss, 1.0, agg.last_den))
    assert qr.same_bits(_np(gd), g0)
    assert agg.aggregate_packed(packed[:3], samples, exact_loss, gd, L, out=gd) is gd
    assert qr.same_bits(_np(gd), _np(got))
    bad_prev = GlobalModel(5, {"fc.bias": prev_w["fc.bias"]}, {}, [], 0.0)
    for bad in (lambda: agg.aggregate_updates([], prev, L),
                lambda: agg.aggregate_updates(ups, prev, L, losses={"c0": 2.0, "c1": 4.0}),
                lambda: agg.aggregate_updates(ups, prev, L, losses=[2.0, 4.0]),
                lambda: agg.aggregate_updates(ups, prev, L, losses=[float("nan")] * 3),
                lambda: agg.aggregate_updates(ups, prev, 0.0),
                lambda: agg.aggregate_updates(ups, bad_prev, L),
                lambda: agg.aggregate_packed(packed, samples, exact_loss, gd, L),
                lambda: agg.aggregate_packed(packed[:3], samples, exact_loss[:2], gd, L),
                lambda: QFedAvgAggregator(device=DEV, q=-1.0),
                lambda: QFedAvgAggregator(device=DEV, weights="loss")):
        with pytest.raises(FedAvgError):
            bad()


# ------------------------------------------------------------------ RankRound
SIZES, BATCH, LR = [8, 40, 100, 24], 8, 0.01      # unequal tiny shards


def _rounds(mine, nrounds=1, losses=None, **kw):
    """`nrounds` rounds over SIZES' clients `mine` on one RankRound.  Returns the RankRound, the
    global vector before round one, and per round (the trained rows by client, copied by the
    on_trained hook; the global vector; global_bufs; the metrics' losses by client; den)."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn", dropout_rate=0.0).to(DEV)
    r = RankRound(model, SIZES, mine, epochs=1, batch=BATCH, device=DEV, lanes=1, dp_seed=11,
                  shuffle_seed=77, **kw)
    xs, ys = [], []
    for k in r.slots:
        gen = torch.Generator().manual_seed(200 + k)
        xs.append(torch.randn(SIZES[k], 1, 28, 28, generator=gen))
        ys.append(torch.randint(0, 10, (SIZES[k],), generator=gen))
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    start = _np(r.global_flat).copy()
    out = []
    for i in range(nrounds):
        extra = {} if losses is None else {"client_losses": losses[i]}
        m = r.run(data, labels, offs, "sgd", LR, seed=3 + i, **extra)
        torch.cuda.synchronize()
        den = None if getattr(r, "_qfa_state", None) is None else float(_np(r._qfa_state)[0])
        out.append((dict(seen), _np(r.global_flat).copy(), _np(r.global_bufs).copy(),
                    {k: m[r.slot_of[k]].loss for k in r.clients}, den))
    return r, start, out


def _want_round(r, cfg, rows, losses, g, den, clients=None):
    clients = r.clients if clients is None else clients
    m = len(SIZES)
    pi = [1.0 / m if cfg.weights == "uniform" else r.weights[k] for k in clients]
    L = cfg.lipschitz if cfg.lipschitz is not None else 1.0 / LR
    a, b = qr.coefficients(pi, [losses[k] for k in clients], cfg.q, L)
    stack = np.stack([rows[k] for k in clients])
    acc, _, ref_den = qr.qfedavg_rows(qr.PARTIAL, stack, a, b, g)
    assert abs(den - ref_den) <= _den_tol(len(clients), stack.shape[1], ref_den)
    return qr.finish(acc, g, den)


def test_rankround_one_rank_two_rounds():
    all4 = list(range(4))
    cfg = QFedAvgConfig(q=1)
    r, g, rounds = _rounds(all4, 2, qfedavg=cfg)
    rp, gp, plain = _rounds(all4, 1, qfedavg=None)
    assert qr.same_bits(g, gp)
    # the default: the round's own last-epoch training losses stand in for F_k
    for i, (rows, glob, _, losses, den) in enumerate(rounds):
        assert all(np.isfinite(v) and v > 0 for v in losses.values())
        g = _want_round(r, cfg, rows, losses, g, den)
        assert qr.same_bits(glob, g), f"round {i + 1}"
    assert r.last_qfedavg["lipschitz"] == 1.0 / LR
    # round one trains from the same start on the same batches: the same rows go in, another
    # global comes out, and the BN running statistics do not see the rule
    for k in all4:
        assert qr.same_bits(rounds[0][0][k], plain[0][0][k])
    stack = np.stack([plain[0][0][k] for k in rp.clients])
    assert qr.same_bits(plain[0][1], nr.weighted_sum(stack, _np(rp.w32)))
    assert not qr.same_bits(rounds[0][1], plain[0][1])
    assert qr.same_bits(rounds[0][2], plain[0][2])
    # qfedavg=None is the path without the argument: the same bits
    _, _, omitted = _rounds(all4, 1)
    assert qr.same_bits(omitted[0][1], plain[0][1]) and qr.same_bits(omitted[0][2], plain[0][2])
    # exact losses from the caller, as a sequence and as a mapping; one client not live (NaN)
    given = [[0.9, 2.5, float("nan"), 0.3], {0: 1.5, 1: 0.2, 2: 3.0, 3: 0.8}]
    cfg2 = QFedAvgConfig(q=2, lipschitz=50.0, weights="samples")
    r2, g2, rounds2 = _rounds(all4, 2, losses=given, qfedavg=cfg2)
    for i, (rows, glob, _, _, den) in enumerate(rounds2):
        g2 = _want_round(r2, cfg2, rows, dict(enumerate(given[i])) if i == 0 else given[i], g2,
                         den)
        assert qr.same_bits(glob, g2), f"given losses, round {i + 1}"
    assert _np(r2._qfa_state)[1] == 4.0 and r2.last_qfedavg["lipschitz"] == 50.0


def test_rankround_fedadam_steps_toward_the_qfedavg_aggregate_and_sparse_rebuilds():
    so = fedopt.FedAdam(0.01, device=DEV)
    cfg = QFedAvgConfig(q=1)
    r, g, rounds = _rounds([0, 1, 2, 3], 2, qfedavg=cfg, server_opt=so)
    tau32 = F(so.tau)
    m, v = np.zeros(r.P, dtype=F), np.full(r.P, tau32 * tau32, dtype=F)
    for i, (rows, glob, _, losses, den) in enumerate(rounds):
        agg = _want_round(r, cfg, rows, losses, g, den)
        g, m, v = fr.server_opt_step(fr.ADAM, agg[None], None, g, m, v, server_lr=so.server_lr,
                                     beta1=so.beta1, beta2=so.beta2, tau=so.tau)
        assert qr.same_bits(glob, g), f"round {i + 1}"
    assert qr.same_bits(_np(r.partial), agg)
    # under q-FedAvg the sums from the payloads are off: the dense rows are rebuilt
    from fedhip.compress import CompressionConfig
    runs = []
    for sparse in (False, True):
        ccfg = CompressionConfig("topk", sparsity_ratio=0.9, sparse=sparse)
        r, _, rounds = _rounds([0, 1, 2, 3], 1, qfedavg=True, compression=ccfg)
        assert not r._sparse_sum() and not r._quant_sum()
        runs.append(rounds)
    assert qr.same_bits(runs[0][0][1], runs[1][0][1])


def test_rankround_refusals():
    from fedhip.round import RankRound
    from src.aggregation import dpfedavg
    from src.shared import models_pytorch as hm
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    for kw, msg in (({"aggregator": robust.MedianAggregator()}, "robust"),
                    ({"server_opt": fedopt.FedYogi(0.01, base=robust.MedianAggregator(),
                                                   device=DEV)}, "robust"),
                    ({"central_dp": dpfedavg.CentralDPConfig(1.1, 0.05)}, "central_dp"),
                    ({"fednova": True}, "fednova")):
        with pytest.raises(FedHipError, match=msg):
            RankRound(model, SIZES, [0, 1, 2, 3], epochs=1, batch=BATCH, device=DEV, lanes=1,
                      qfedavg=True, **kw)
    with pytest.raises(ValueError):
        QFedAvgConfig(q=-1)
    with pytest.raises(ValueError):
        QFedAvgConfig(lipschitz=0.0)
    with pytest.raises(ValueError):
        QFedAvgConfig(weights="loss")
    plain = RankRound(model, SIZES, [0, 1, 2, 3], epochs=1, batch=BATCH, device=DEV, lanes=1)
    with pytest.raises(FedHipError, match="client_losses"):
        plain.run(None, None, [], client_losses=[1.0] * 4)
    with pytest.raises(FedHipError, match="no live"):
        _rounds([0, 1, 2, 3], 1, losses=[[float("nan")] * 4], qfedavg=True)
    with pytest.raises(FedHipError, match="client_losses"):
        _rounds([0, 1, 2, 3], 1, losses=[[1.0] * 3], qfedavg=True)


def _rank_main(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        res = {}
        for name, exact in (("all_reduce", False), ("exact", True)):
            r, start, rounds = _rounds(mine, 1, qfedavg=QFedAvgConfig(q=1), exact=exact)
            res[name] = (start, rounds[0][0], rounds[0][1], list(r.clients), rounds[0][3],
                         rounds[0][4])
        q.put((rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def test_rankround_two_ranks_all_reduce_and_exact():
    """Two gloo ranks on cuda:0.  All-reduce mode: both ranks end with the same global vector and
    the same den, the reference's PARTIAL per rank (client-list order), the two added, FINISH
    with the all-reduced den.  exact=True: the STEP reference over all clients in global client
    order, every rank holding every client's loss."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29760 + os.getpid() % 200
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        deadline = time.monotonic() + 240
        while len(res) < world and time.monotonic() < deadline:
            try:
                rank, val = q.get(timeout=1)
                res[rank] = val
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):
                    break       # a rank died without reporting: fail now, no retry
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert r in res, f"rank {r} reported nothing (exit codes {[p.exitcode for p in procs]})"
        assert not isinstance(res[r], str), f"rank {r} failed: {res[r]}"
    assert all(p.exitcode == 0 for p in procs)
    cfg, m, L = QFedAvgConfig(q=1), len(SIZES), 1.0 / LR
    for name in ("all_reduce", "exact"):
        (s0, rows0, g0, c0, l0, d0), (s1, rows1, g1, c1, l1, d1) = res[0][name], res[1][name]
        assert sorted(c0 + c1) == list(range(m))
        assert qr.same_bits(s0, s1)
        assert qr.same_bits(g0, g1), f"{name}: ranks disagree on the global model"
        assert d0 == d1, f"{name}: ranks disagree on den"
        rows, losses = {**rows0, **rows1}, {**l0, **l1}
        P = s0.shape[0]
        if name == "all_reduce":
            parts, den = [], D(0.0)
            for c in (c0, c1):
                a, b = qr.coefficients([1.0 / m] * len(c), [losses[k] for k in c], cfg.q, L)
                acc, _, dk = qr.qfedavg_rows(qr.PARTIAL, np.stack([rows[k] for k in c]), a, b, s0)
                parts.append(acc)
                den = den + dk
            total = parts[0] + parts[1]
            assert total.dtype == F and abs(d0 - den) <= _den_tol(m, P, den)
            want = qr.qfedavg_rows(qr.FINISH, total, None, None, s0, den=d0)[0]
        else:
            a, b = qr.coefficients([1.0 / m] * m, [losses[k] for k in range(m)], cfg.q, L)
            acc, _, den = qr.qfedavg_rows(qr.PARTIAL, np.stack([rows[k] for k in range(m)]), a,
                                          b, s0)
            assert abs(d0 - den) <= _den_tol(m, P, den)
            want = qr.finish(acc, s0, d0)
        assert qr.same_bits(g0, want), name
        assert not qr.same_bits(g0, s0)
