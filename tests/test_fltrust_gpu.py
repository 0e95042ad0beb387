"""fh_fltrust_rows (csrc/fltrust.hip), FLTrustAggregator and RankRound(trust_root=) on the GPU,
against the numpy reference of tests/fltrust_ref.py (pinned by test_fltrust_ref_cpu.py).

The fp64 sums (squared norms, dot products) differ from numpy's only by the order of the
additions and are held to derived bounds, not tuned on the GPU: every product is exact in fp64
and a sum of n fp64 terms in any order is within (n - 1) * 2^-53 * sum |terms| of the exact sum,
so two orders differ by at most 2 * P * 2^-53 * sum |terms| (the terms of a squared norm are
non-negative: the sum itself).  What follows the sums is compared with the reference's fp64 lines
evaluated on the kernel's OWN sums.  The chain is six fp64 operations and a device sqrt or
division need not round as numpy's do, which would allow a few fp64 ulps on the scores and one
fp32 ulp on the coefficients; measured on an MI355X over all the shapes below and both layouts
(240 calls) the scores, S, n0 and the coefficients agreed with the reference bit for bit, so the
check is equality.  What is fp32 is held bit for bit (uint32 views) too: STEP's out is the
reference DELTA step applied with the kernel's own coefficients.

Shapes: client counts on both sides of every register-slot count, vector width (16 bytes up to
8 clients, 8 bytes up to 16, scalar above) and the two-launch split at 32; sizes below, at and
above the vector width, the 256-thread tile and a workgroup's columns per tile (256 * 4, 256 * 2,
256), one size of several workgroups with a tail, and one at which a workgroup walks two tiles.
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
import fltrust_ref as tr
from fedhip import ops
from fedhip._lib import FedHipError, call, ptr, stream_handle
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgError
from src.shared.models import GlobalModel, ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
F, D = np.float32, np.float64

CS = [1, 2, 3, 16, 17, 32, 33, 64]
PS = [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3 * 1024 + 7]
MIN_COS = 0.05


def _np(t):
    return t.detach().cpu().numpy()


def _data(C, P, seed, spread=(-1.5, 1.0)):
    """(rows, root, g): the root's delta d0 at mixed magnitudes per coordinate; client k's delta
    is mag_k * (sign_k * a_k * d0 + b_k * n_k) with n_k orthogonal to d0 and of its norm, so
    |cos| = a / sqrt(a^2 + b^2) >= 0.28 before rounding (every fourth client points away from
    the root when C >= 4), at magnitudes 10^spread per client; denormals in g, in a row and in
    the root.  The cosines of the rounded data are checked below, on the CPU."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 1, P)).astype(F)
    den_bits = rng.integers(1, 1 << 22, size=(3, P)).astype(np.uint32).view(F)
    g[::11] = den_bits[0, ::11]                          # denormal globals ...
    # deltas a few decades below the coordinate's own size: the rounding of g + delta, 2^-24 of
    # it, stays small against the delta and does not turn the directions
    scale = np.maximum(np.abs(g), 1e-3) * 10.0 ** rng.uniform(-2, 0, P)
    d0 = rng.standard_normal(P) * scale
    d0[11::22] = 0.0                                     # where the root turns denormal below
    noise = rng.standard_normal((C, P)) * scale
    noise -= (noise @ d0)[:, None] / (d0 @ d0) * d0[None, :]
    norm = np.sqrt((noise * noise).sum(1, keepdims=True))
    noise *= np.sqrt(d0 @ d0) / np.where(norm > 0, norm, 1.0)
    mag = 10.0 ** rng.uniform(spread[0], spread[1], (C, 1))
    sign = np.where((np.arange(C) % 4 == 3) & (C >= 4), -1.0, 1.0)[:, None]
    a, b = rng.uniform(0.3, 1.5, (C, 1)), rng.uniform(0.2, 1.0, (C, 1))
    rows = (g + mag * (sign * a * d0 + b * noise)).astype(F)
    root = (g + d0).astype(F)
    rows[rng.integers(C), ::11] = -den_bits[1, ::11]     # ... under a row's denormals
    root[11::22] = den_bits[2, 11::22]                   # ... and the root's
    d, d064 = rows.astype(D) - g.astype(D), root.astype(D) - g.astype(D)
    with np.errstate(all="ignore"):
        cos = (d * d064).sum(1) / np.sqrt((d * d).sum(1) * (d064 * d064).sum())
    assert (np.abs(cos) >= MIN_COS).all(), (C, P, cos)   # the clip's kink is far from every client
    return rows, root, g


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


def _run(mode, view, root, g, goff=0, ooff=4, roff=0, row_index=None, alias=False,
         root_view=None):
    """One fh_fltrust_rows into sentinel windows -> dict of numpy results."""
    P = view.shape[1]
    C = view.shape[0] if row_index is None else row_index.numel()
    gbuf, gd = _window(P, goff, fill=g)
    rbuf, rd = (None, root_view) if root_view is not None else _window(P, roff, fill=root)
    buf, out = (gbuf, gd) if alias else _window(P, ooff)
    need = ops.fltrust_workspace(C, P)
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    got, coef, trust, stats, state = ops.fltrust_rows(view, rd, gd, out, mode,
                                                      row_index=row_index, workspace=ws[:need])
    torch.cuda.synchronize()
    assert got is out and _intact(buf, goff if alias else ooff, P)
    assert (_np(ws[need:]) == 0xA5).all()
    if rbuf is not None:
        assert tr.same_bits(_np(rd), root) and _intact(rbuf, roff, P)
    if not alias:
        assert tr.same_bits(_np(gd), g) and _intact(gbuf, goff, P)
        if mode == ops.FLT_SCORE:
            assert (_np(out) == SENTINEL).all()
    return {"out": _np(out).copy(), "coef": _np(coef), "trust": _np(trust), "stats": _np(stats),
            "state": _np(state), "after": _np(ws[:8 * C].view(torch.float64)).copy()}


def _same_fp64(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))
               for k in ("trust", "stats", "state")) and tr.same_bits(a["coef"], b["coef"])


def _check(rows, root, g, view, tag, **kw):
    """SCORE and STEP on one layout against the reference; returns STEP's results."""
    C, P = rows.shape
    sq, dot, sq0 = tr.stats(rows, root, g)
    with np.errstate(all="ignore"):
        absdot = np.abs((rows - g[None, :]).astype(D) * (root - g).astype(D)[None, :]).sum(1)
    eps = 2 * P * 2.0 ** -53
    sc = _run(ops.FLT_SCORE, view, root, g, **kw)
    st = _run(ops.FLT_STEP, view, root, g, **kw)
    assert _same_fp64(sc, st), tag                       # the same launches, the same bits
    ksq, kdot, ksq0 = st["stats"][:C], st["stats"][C:2 * C], st["stats"][2 * C]
    assert (np.abs(ksq - sq) <= eps * sq).all(), (tag, ksq, sq)
    assert (np.abs(kdot - dot) <= eps * absdot).all(), (tag, kdot, dot)
    assert abs(ksq0 - sq0) <= eps * sq0, (tag, ksq0, sq0)
    coef, trust, state = tr.coefficients(ksq, kdot, ksq0)
    assert np.array_equal(st["trust"].view(np.uint64), trust.view(np.uint64)), (tag, trust)
    assert np.array_equal(st["state"].view(np.uint64), state.view(np.uint64)), (tag, state)
    assert tr.same_bits(st["coef"], coef) and not np.signbit(st["coef"]).any(), (tag, coef)
    want, after = tr.step(rows, st["coef"], g)
    assert tr.same_bits(st["out"], want), tag
    assert (np.abs(st["after"] - after) <= eps * after).all(), (tag, st["after"], after)
    return st


@pytest.mark.parametrize("C", CS)
def test_fltrust_bits(C):
    for P in PS:
        rows, root, g = _data(C, P, 1000 * C + P)
        vec = _place(rows, (P + 3) // 4 * 4 + 4, 0)    # stride % 4 == 0, > P: vector + tail
        sca = _place(rows, (P + 2) | 1, 0)             # odd stride > P: scalar path
        got = [_check(rows, root, g, v, (C, P, v.stride(0))) for v in (vec, sca)]
        # the vector and the scalar path sum in different orders: the fp64 sums may differ in
        # the last bits, the coefficients then by an fp32 ulp; with the same coefficients the
        # two paths give the same bits of out
        if tr.same_bits(got[0]["coef"], got[1]["coef"]):
            assert tr.same_bits(got[0]["out"], got[1]["out"]), (C, P)


def test_a_workgroup_walks_two_tiles_and_two_launches():
    """33 clients (two 32-slot launches) over more columns than 512 workgroups hold in one
    tile of 256: the grid-stride loop and the last, partial tile.  512 * 256 + 257 columns on
    an odd stride is the smallest such shape: 514 tiles on 257 workgroups."""
    C, P = 33, 512 * 256 + 300
    rows, root, g = _data(C, P, 7)
    _check(rows, root, g, _place(rows, P + 4, 0), (C, P))
    P = 512 * 256 + 257
    rows, root, g = _data(C, P, 8)
    _check(rows, root, g, _place(rows, (P + 2) | 1, 0), (C, P))


@pytest.mark.parametrize("C", [1, 2, 5, 33])
def test_fltrust_step_within_fp32_tolerance_of_fp64(C):
    """STEP against the rule evaluated in fp64 from the same fp32 inputs (rule_fp64: exact
    differences, exact sums).  With u = 2^-24:
      * the kernel's deltas are rounded differences, each off by at most u relative (and exact
        in the denormal range), so a norm is off by u relative and a dot product by 2u relative
        to sum |d d0| <= n_k n0: the cosine by at most 2u(1 + |cos|) <= 4u absolute, a score
        ts_k >= MIN_COS by 4u / ts_k relative, S by 4u * T / S relative (T trusted clients);
        summation order and the fp64 chain add 2^-40 at most;
      * c_k = fl32(ts_k * (n0 / n_k) / S) is therefore off by u * (4/ts_k + 2 + 4T/S + 1)
        relative; its term c_k * d_kj adds the subtract's and the multiply's rounding: + 2;
      * the C - 1 adds of acc and the final add round once each on at most
        sum_k |c_k d_kj| (+ |g_j| for the last): C * sum + |g_j|;
      * a product or a coefficient in the fp32 denormal range is rounded to a multiple of 2^-149:
        2^-150 per product and 2^-150 * |d_kj| per coefficient (sums in that range are exact).
    1.01 covers the second-order terms."""
    P = 4001
    rows, root, g = _data(C, P, 40 + C, spread=(-1.0, 1.0))
    st = _run(ops.FLT_STEP, _place(rows, 4004, 0), root, g)
    want, ts, c = tr.rule_fp64(rows, root, g)
    T, S = np.count_nonzero(ts), ts.sum()
    assert T >= 1 and np.array_equal(st["trust"] > 0, ts > 0)
    assert (np.abs(st["trust"] - ts) <= 1.01 * 4 * 2.0 ** -24).all()
    absd = np.abs(rows.astype(D) - g.astype(D))
    with np.errstate(all="ignore"):
        per = np.where(ts > 0, 4.0 / ts + 4.0 * T / S + 5.0, 0.0)
    terms = np.abs(c)[:, None] * absd
    bound = 1.01 * 2.0 ** -24 * ((per[:, None] * terms).sum(0) + C * terms.sum(0)
                                 + np.abs(g.astype(D))) + 2.0 ** -150 * (absd.sum(0) + C)
    err = np.abs(st["out"].astype(D) - want)
    print(f"C={C}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("C", [3, 17, 33])
def test_row_index_root_row_misalignment_aliasing_and_replay(C):
    P, tall = 1001, C + 6
    rng = np.random.default_rng(C)
    rows, root, g = _data(tall, P, 77 + C)
    perm = rng.permutation(tall)
    pick, rpos = perm[:C], int(perm[C])            # a permuted subset; the root is another row
    rows[rpos] = root
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    aligned = _place(rows, 1008, 0)
    want = _check(rows[pick], root, g, aligned, ("aligned", C), row_index=idx)
    # the root as a row of the same matrix
    as_row = _run(ops.FLT_STEP, aligned, root, g, row_index=idx, root_view=aligned[rpos])
    assert _same_fp64(as_row, want) and tr.same_bits(as_row["out"], want["out"])
    # the same call again: the same bits, fp64 included
    again = _run(ops.FLT_STEP, aligned, root, g, row_index=idx)
    assert _same_fp64(again, want) and tr.same_bits(again["out"], want["out"])
    assert np.array_equal(again["after"].view(np.uint64), want["after"].view(np.uint64))
    for view, kw in ((_place(rows, 1008, 1), {}),             # rows + 4 B: scalar path
                     (aligned, {"roff": 1}),                   # root + 4 B: scalar path
                     (aligned, {"goff": 3}),                   # global + 12 B: scalar path
                     (aligned, {"ooff": 1}),                   # out + 4 B: the stats pass is vector
                     (_place(rows, 1003, 0), {})):             # odd stride
        got = _check(rows[pick], root, g, view, (C, kw), row_index=idx, **kw)
        if kw == {"ooff": 1}:   # the same stats launches: the same coefficients, the same out
            assert _same_fp64(got, want)
        if tr.same_bits(got["coef"], want["coef"]):
            assert tr.same_bits(got["out"], want["out"]), (C, kw)
    # STEP with out aliased to global, aligned and not
    for off in (0, 1):
        got = _run(ops.FLT_STEP, aligned, root, g, row_index=idx, alias=True, goff=off)
        assert tr.same_bits(got["out"], tr.step(rows[pick], got["coef"], g)[0]), off
        if off == 0:
            assert tr.same_bits(got["out"], want["out"]) and _same_fp64(got, want)
    # the identity index against no index
    ident = torch.arange(tall, dtype=torch.int32, device=DEV)
    w0 = _run(ops.FLT_STEP, aligned, root, g)
    w1 = _run(ops.FLT_STEP, aligned, root, g, row_index=ident)
    assert _same_fp64(w0, w1) and tr.same_bits(w0["out"], w1["out"])
    assert tr.same_bits(w0["out"], tr.step(rows, w0["coef"], g)[0])


@pytest.mark.parametrize("C", [4, 17, 64])
def test_distrusted_and_broken_rows_and_nobody_trusted(C):
    P = 1030
    rows, root, g = _data(C, P, 5 + C)
    away = [k for k in range(C) if k % 4 == 3]
    bad = rows.copy()
    bad[away[0], 7] = np.nan
    if len(away) > 1:
        bad[away[1], :] = np.inf
        bad[away[1], ::2] = -np.inf
    for stride in (1032, 1031):    # the vector and the scalar path, each against itself
        clean = _run(ops.FLT_STEP, _place(rows, stride, 0), root, g)
        assert not clean["coef"][away].any() and not clean["trust"][away].any()
        assert (np.delete(clean["coef"], away) > 0).all()
        got = _run(ops.FLT_STEP, _place(bad, stride, 0), root, g)
        assert tr.same_bits(got["out"], clean["out"]) and tr.same_bits(got["coef"], clean["coef"])
        assert np.array_equal(got["trust"].view(np.uint64), clean["trust"].view(np.uint64))
        assert got["state"][0] == clean["state"][0] and got["state"][2] == clean["state"][2]
        assert got["state"][1] == clean["state"][1] - min(len(away), 2)
        assert np.isnan(got["stats"][away[0]])
        # without the distrusted rows: the same rule (fewer register slots may change the order
        # of the sums: the coefficients to an fp32 ulp, out from the call's own coefficients)
        keep = [k for k in range(C) if k not in away]
        idx = torch.tensor(keep, dtype=torch.int32, device=DEV)
        sub = _run(ops.FLT_STEP, _place(bad, stride, 0), root, g, row_index=idx)
        assert (np.abs(sub["coef"] - clean["coef"][keep]) <= np.spacing(clean["coef"][keep])).all()
        assert tr.same_bits(sub["out"], tr.step(bad[keep], sub["coef"], g)[0])
    # nobody trusted although the root moved and every client is live: out == g bitwise (-0 and
    # denormals in g included; the DELTA step alone would store g + 0), S = 0
    g2 = g.copy()
    g2[:4] = np.array([0x80000000, 0x00000001, 0x80000000, 0x80000001], dtype=np.uint32).view(F)
    g2[4:8] = 0.0
    d0 = root.astype(D) - g.astype(D)
    d0[:8] = 0.0
    root2 = g2.copy()
    root2[8:] = (g2[8:] + d0[8:]).astype(F)
    against = (g2.astype(D) - np.abs(rows.astype(D) - g.astype(D)) * np.sign(d0)).astype(F)
    against[:, :4] = 1.0
    for alias in (False, True):
        for stride in (1032, 1031):
            got = _run(ops.FLT_STEP, _place(against, stride, 0), root2, g2, alias=alias)
            assert tr.same_bits(got["out"], g2), (alias, stride)
            assert not got["coef"].any() and not got["trust"].any()
            assert got["state"][:3].tolist() == [0.0, C, 0.0] and got["state"][3] > 0
    # NaN payloads in g (every delta is NaN there: nobody is live): g bit for bit
    g3 = g2.copy()
    g3[:2] = np.array([0xFFA5A5A5, 0x7F800001], dtype=np.uint32).view(F)
    for alias in (False, True):
        got = _run(ops.FLT_STEP, _place(against, 1032, 0), root2, g3, alias=alias)
        assert tr.same_bits(got["out"], g3) and got["state"][:3].tolist() == [0.0, 0.0, 0.0]
    # a zero root delta: the same, whatever the clients did
    for alias in (False, True):
        got = _run(ops.FLT_STEP, _place(rows, 1032, 0), g, g, alias=alias)
        assert tr.same_bits(got["out"], g) and not got["coef"].any()
        assert got["state"][0] == 0.0 and got["state"][3] == 0.0 and got["stats"][2 * C] == 0.0
    agg = robust.FLTrustAggregator(device=DEV)
    gd = torch.from_numpy(g2).to(DEV)
    with pytest.raises(FedAvgError, match="no client is trusted"):
        agg.aggregate_packed(_place(against, 1032, 0), [1] * C, center=gd, out=gd,
                             root_row=torch.from_numpy(root2).to(DEV))
    assert tr.same_bits(_np(gd), g2) and agg.last_rejected == list(range(C))
    with pytest.raises(FedAvgError, match="root update is zero"):
        agg.aggregate_packed(_place(rows, 1032, 0), [1] * C, center=gd, root_row=gd.clone())


def test_fltrust_argument_errors_write_nothing():
    rows = torch.zeros(65, 8, device=DEV)
    g = torch.zeros(8, device=DEV)
    root = torch.ones(8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    coef = torch.full((65,), SENTINEL, device=DEV)
    trust = torch.full((65,), SENTINEL, dtype=torch.float64, device=DEV)
    stats = torch.full((131,), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.full((4,), SENTINEL, dtype=torch.float64, device=DEV)
    ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)

    def raw(C=3, P=8, mode=1, stride=8, rows_p=ptr(rows), root_p=ptr(root), g_p=ptr(g),
            out_p=ptr(out), ws_p=ptr(ws), ws_n=1 << 16, coef_p=ptr(coef), trust_p=ptr(trust),
            stats_p=ptr(stats), st_p=ptr(st)):
        call("fh_fltrust_rows", rows_p, stride, None, C, P, root_p, g_p, mode, out_p, ws_p, ws_n,
             coef_p, trust_p, stats_p, st_p, stream_handle())

    for kw, msg in ((dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"),
                    (dict(C=0), "num_clients=0"), (dict(C=65), "num_clients=65"),
                    (dict(P=-1), "P=-1"), (dict(stride=-8), "row_stride=-8"),
                    (dict(coef_p=None), "null"), (dict(trust_p=None), "null"),
                    (dict(stats_p=None), "null"), (dict(st_p=None), "null"),
                    (dict(st_p=None, P=0), "null"), (dict(rows_p=None), "null"),
                    (dict(root_p=None), "null"), (dict(g_p=None), "null"),
                    (dict(out_p=None), "null"), (dict(ws_n=8), "workspace"),
                    (dict(ws_p=None), "workspace"), (dict(ws_p=ptr(ws) + 4), "workspace"),
                    (dict(mode=0, ws_n=8), "workspace")):
        with pytest.raises(FedHipError, match=msg):
            raw(**kw)
    with pytest.raises(FedHipError, match="outside"):
        ops.fltrust_rows(rows, root, g, out, ops.FLT_STEP)
    with pytest.raises(FedHipError, match="HIP device"):
        ops.fltrust_rows(torch.zeros(3, 8), root, g, out, ops.FLT_STEP)
    with pytest.raises(FedHipError, match="mode"):
        ops.fltrust_rows(rows[:3], root, g, out, 2)
    with pytest.raises(FedHipError, match="required"):
        ops.fltrust_rows(rows[:3], root, g, None, ops.FLT_STEP)
    with pytest.raises(FedHipError, match="root"):
        ops.fltrust_rows(rows[:3], root.double(), g, out, ops.FLT_STEP)
    with pytest.raises(FedHipError, match="trust"):
        ops.fltrust_rows(rows[:3], root, g, out, ops.FLT_STEP, trust=coef)
    assert ops.fltrust_workspace(0, 8) == 0 and ops.fltrust_workspace(65, 8) == 0
    assert ops.fltrust_workspace(3, 0) == 0
    assert ops.fltrust_workspace(3, 8) >= 64 * 8 + 8 * 4 + 7 * 8
    torch.cuda.synchronize()
    for t in (out, coef, trust, stats, st):
        assert (_np(t) == SENTINEL).all()
    assert (_np(ws) == 0x5A).all()
    raw(mode=0, out_p=None)            # SCORE takes no out
    # P == 0: the state from nothing, no out, no workspace
    raw(P=0, ws_p=None, ws_n=0, rows_p=None, root_p=None, g_p=None, out_p=None)
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all()
    assert _np(coef)[:3].tolist() == [0.0] * 3 and not np.signbit(_np(coef)[:3]).any()
    assert _np(trust)[:3].tolist() == [0.0] * 3 and _np(stats)[:7].tolist() == [0.0] * 7
    assert _np(st).tolist() == [0.0, 0.0, 0.0, 0.0]
    assert (_np(coef)[3:] == SENTINEL).all() and (_np(stats)[7:] == SENTINEL).all()
    got = ops.fltrust_rows(rows[:2], root, g, out, ops.FLT_STEP, P=0)
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all() and _np(got[4]).tolist() == [0.0] * 4


# ------------------------------------------------------------------ the aggregator
SHAPES = {"conv.weight": (4, 1, 3, 3), "fc.bias": (5,)}


def _flat(weights):
    return np.concatenate([_np(weights[n]).reshape(-1) for n in SHAPES])


def _want_from(agg, rows, root, g):
    """The reference step with the aggregator's own coefficients, which are first checked
    against the reference's (numpy's sums differ from the device's in the last bits: 2 ulps)."""
    coef = np.asarray(agg.last_coef, dtype=F)
    ref = tr.fltrust_rows(tr.SCORE, rows, root, g)
    assert (np.abs(coef.astype(D) - ref[1].astype(D)) <= 2 * np.spacing(ref[1]).astype(D)).all()
    assert np.allclose(agg.last_trust, ref[2], rtol=1e-12, atol=0)
    assert agg.last_rejected == [k for k, c in enumerate(coef) if c == 0]
    assert abs(agg.last_root_norm - ref[4][3]) <= 1e-12 * ref[4][3]
    out, after = tr.step(rows, coef, g)
    assert np.allclose(_np(agg.last_sqdist), after, rtol=1e-12, atol=0)
    return out


def test_aggregate_updates_and_packed_against_the_reference():
    gen = torch.Generator().manual_seed(4)
    prev_w = {name: 0.3 * torch.randn(*shape, generator=gen) for name, shape in SHAPES.items()}
    prev = GlobalModel(round_number=3, model_weights=prev_w, accuracy_metrics={},
                       participating_clients=[], convergence_score=0.0)
    step = {name: 0.05 * torch.randn(*t.shape, generator=gen) for name, t in prev_w.items()}

    def update(cid, scale, noise, n):
        wts = {name: t + scale * step[name] + noise * torch.randn(*t.shape, generator=gen)
               for name, t in prev_w.items()}
        return ModelUpdate(client_id=cid, round_number=4, model_weights=wts, num_samples=n,
                           training_loss=0.5, privacy_budget_used=0.5, compression_ratio=0.8,
                           timestamp=datetime.now())

    server = update("server", 1.0, 0.0, 5)
    ups = [update("c0", 0.8, 0.01, 10), update("c1", -1.0, 0.01, 11),    # c1 points away
           update("c2", 50.0, 0.2, 12)]                                   # c2 is scaled up
    rows = np.stack([_flat(u.model_weights) for u in ups])
    g0, root = _flat(prev_w), _flat(server.model_weights)
    agg = robust.FLTrustAggregator(device=DEV)
    for su in (server, server.model_weights):
        gm = agg.aggregate_updates(ups, prev, su)
        assert gm.round_number == 4 and gm.participating_clients == ["c0", "c1", "c2"]
        assert [gm.model_weights[n].shape for n in SHAPES] == \
            [torch.Size(s) for s in SHAPES.values()]
        assert tr.same_bits(_flat(gm.model_weights), _want_from(agg, rows, root, g0))
        assert tr.same_bits(_flat(prev_w), g0)   # the global model is not stepped in place
        assert agg.last_rejected == [1] and agg.last_trust[1] == 0.0
    assert agg.aggregation_history[-1]["client_samples"]["c2"] == 12
    # the scaled-up client moves the model no further than the root's norm allows
    moved = np.linalg.norm(_flat(gm.model_weights).astype(D) - g0)
    assert moved <= 1.001 * agg.last_root_norm
    # aggregate_packed: rows on the device, a permuted subset, the root a row or a tensor
    packed = _place(np.concatenate([rows, root[None], rows[::-1]]), 48, 0)
    gd = torch.from_numpy(g0).to(DEV)
    got = agg.aggregate_packed(packed, [1, 1, 1], row_index=[6, 5, 4], center=gd, root_row=3)
    assert tr.same_bits(_np(got), _want_from(agg, rows, root, g0)) and tr.same_bits(_np(gd), g0)
    got2 = agg.aggregate_packed(packed[:4], [7, 8, 9], center=gd, root_row=3)    # rows 0..2
    assert tr.same_bits(_np(got2), _np(got))
    rd = torch.from_numpy(root).to(DEV)
    assert agg.aggregate_packed(packed[:3], [1] * 3, center=gd, root_row=rd, out=gd) is gd
    assert tr.same_bits(_np(gd), _np(got))
    gd = torch.from_numpy(g0).to(DEV)
    bad_prev = GlobalModel(5, {"fc.bias": prev_w["fc.bias"]}, {}, [], 0.0)
    for bad in (lambda: agg.aggregate_updates([], prev, server),
                lambda: agg.aggregate_updates(ups),
                lambda: agg.aggregate_updates(ups, prev),
                lambda: agg.aggregate_updates(ups, prev, server, weights=[1.0] * 3),
                lambda: agg.aggregate_updates(ups, bad_prev, server),
                lambda: agg.aggregate_updates(ups, prev, {"fc.bias": prev_w["fc.bias"]}),
                lambda: agg.aggregate_updates(ups, prev, prev_w),          # a root that stood still
                lambda: agg.aggregate_packed(packed, [1] * 3, center=gd, root_row=2),
                lambda: agg.aggregate_packed(packed[:3], [1] * 3, center=gd),
                lambda: agg.aggregate_packed(packed[:3], [1] * 3, center=gd.double(), root_row=rd),
                lambda: agg.aggregate_packed(packed, [1] * 65, row_index=[0] * 65, center=gd,
                                             root_row=rd)):
        with pytest.raises(FedAvgError):
            bad()


# ------------------------------------------------------------------ RankRound
SIZES, BATCH, LR = [8, 40, 100, 24], 8, 0.01      # unequal tiny shards
ROOT = 1                                          # the server's root shard


def _rounds(mine, nrounds=1, **kw):
    """`nrounds` rounds over SIZES' clients `mine` on one RankRound.  Returns the RankRound, the
    global vector before round one, and per round (the trained rows by client, copied by the
    on_trained hook; the global vector; global_bufs; the rule's last coefficients)."""
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
        r.run(data, labels, offs, "sgd", LR, seed=3 + i)
        torch.cuda.synchronize()
        coef = None if r.aggregator is None else list(r.aggregator.last_coef)
        out.append((dict(seen), _np(r.global_flat).copy(), _np(r.global_bufs).copy(), coef))
    # the hook refers back to r: without this the round would be a dead reference cycle that
    # still owns captured step graphs, freed whenever the collector next runs
    r.on_trained = None
    for lane in r.trainer.lanes:
        lane.release_graphs()
    return r, start, out


def _want_round(rows, coef, g, others):
    """The reference step over the other clients' hooked rows with the round's own coefficients,
    which are first held against the reference's (2 fp32 ulps: the sums' order)."""
    stack = np.stack([rows[k] for k in others])
    coef = np.asarray(coef, dtype=F)
    ref = tr.fltrust_rows(tr.SCORE, stack, rows[ROOT], g)[1]
    assert (np.abs(coef.astype(D) - ref.astype(D)) <= 2 * np.spacing(ref).astype(D)).all()
    return tr.step(stack, coef, g)[0]


def test_rankround_one_rank_two_rounds():
    all4, others = list(range(4)), [0, 2, 3]
    r, g, rounds = _rounds(all4, 2, aggregator=robust.FLTrustAggregator(device=DEV),
                           trust_root=ROOT)
    rp, gp, plain = _rounds(all4, 1)
    assert tr.same_bits(g, gp)
    for i, (rows, glob, _, coef) in enumerate(rounds):
        assert len(coef) == 3
        g = _want_round(rows, coef, g, others)
        assert tr.same_bits(glob, g), f"round {i + 1}"
    # round one trains from the same start on the same batches: the same rows go in (the root's
    # among them), another global comes out, and the BN running statistics do not see the rule
    for k in all4:
        assert tr.same_bits(rounds[0][0][k], plain[0][0][k])
    stack = np.stack([plain[0][0][k] for k in rp.clients])
    assert tr.same_bits(plain[0][1], nr.weighted_sum(stack, _np(rp.w32)))
    assert not tr.same_bits(rounds[0][1], plain[0][1])
    assert tr.same_bits(rounds[0][2], plain[0][2])
    # aggregator=None, trust_root=None is the path without the arguments: the same bits
    _, _, named = _rounds(all4, 1, aggregator=None, trust_root=None)
    assert tr.same_bits(named[0][1], plain[0][1]) and tr.same_bits(named[0][2], plain[0][2])


def test_rankround_fedadam_steps_toward_the_fltrust_aggregate():
    others = [0, 2, 3]
    for kw in ({"aggregator": robust.FLTrustAggregator(device=DEV)}, {}):
        base = {} if kw else {"base": robust.FLTrustAggregator(device=DEV)}
        so = fedopt.FedAdam(0.01, device=DEV, **base)
        r, g, rounds = _rounds(list(range(4)), 2, server_opt=so, trust_root=ROOT, **kw)
        tau32 = F(so.tau)
        m, v = np.zeros(r.P, dtype=F), np.full(r.P, tau32 * tau32, dtype=F)
        for i, (rows, glob, _, coef) in enumerate(rounds):
            agg = _want_round(rows, coef, g, others)
            g, m, v = fr.server_opt_step(fr.ADAM, agg[None], None, g, m, v,
                                         server_lr=so.server_lr, beta1=so.beta1, beta2=so.beta2,
                                         tau=so.tau)
            assert tr.same_bits(glob, g), f"round {i + 1}"
        assert tr.same_bits(_np(r.partial), agg)


def test_rankround_refusals_on_the_device():
    from fedhip.round import RankRound
    from src.aggregation import dpfedavg
    from src.shared import models_pytorch as hm
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    flt = robust.FLTrustAggregator
    for kw, msg in (({"aggregator": flt(device=DEV)}, "trust_root"),
                    ({"trust_root": 0}, "FLTrustAggregator"),
                    ({"aggregator": flt(device=DEV), "trust_root": 4}, "not a client"),
                    ({"aggregator": flt(device=DEV), "trust_root": 0,
                      "central_dp": dpfedavg.CentralDPConfig(1.1, 0.05)}, "central_dp"),
                    ({"aggregator": flt(device=DEV), "trust_root": 0, "fednova": True}, "fednova"),
                    ({"aggregator": flt(device=DEV), "trust_root": 0, "qfedavg": True},
                     "qfedavg")):
        with pytest.raises(FedHipError, match=msg):
            RankRound(model, SIZES, [0, 1, 2, 3], epochs=1, batch=BATCH, device=DEV, lanes=1,
                      **kw)


def _rank_main(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        r, start, rounds = _rounds(mine, 1, aggregator=robust.FLTrustAggregator(device=DEV),
                                   trust_root=ROOT, exact=True)
        q.put((rank, (start, rounds[0][0], rounds[0][1], list(r.clients), rounds[0][3])))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def test_rankround_two_ranks_exact():
    """Two gloo ranks on cuda:0 with exact=True: both ranks end with the same global vector, the
    reference over all clients but the root in global client order; the root trains on rank 1
    and its row is taken from the gather."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30260 + os.getpid() % 200
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
    (s0, rows0, g0, c0, k0), (s1, rows1, g1, c1, k1) = res[0], res[1]
    assert sorted(c0 + c1) == list(range(len(SIZES))) and ROOT in c1
    assert tr.same_bits(s0, s1)
    assert tr.same_bits(g0, g1), "ranks disagree on the global model"
    assert k0 == k1 and len(k0) == len(SIZES) - 1
    want = _want_round({**rows0, **rows1}, k0, s0, [0, 2, 3])
    assert tr.same_bits(g0, want)
    assert not tr.same_bits(g0, s0)
