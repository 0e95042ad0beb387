"""The FedNova kernel (csrc/fednova.hip) and what is built on it, on the GPU, against the numpy
reference of tests/fednova_ref.py (pinned by test_fednova_ref_cpu.py).

fh_fednova_rows is held to the reference bit for bit (uint32 views) in its three modes, for
client counts around the 4-rows-in-flight unroll, sizes below / across the 4-column vector
width and the 256-thread block, with and without a row index, through the vector path and every
way onto the scalar path (odd stride, each of rows / global / out + 4 B).  global and out live
inside sentinel-filled buffers, the gaps between rows hold NaN, and nothing but out[0:P] may
change.
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
from fedhip import _lib, ops
from fedhip._lib import FedHipError
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgError
from src.aggregation.fednova import FedNovaAggregator, FedNovaConfig
from src.shared.models import GlobalModel, ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
UNWRITTEN = -777.25
F = np.float32

CS = [1, 2, 3, 4, 5, 9, 33]
PS = [1, 3, 4, 5, 255, 1027]
MODES = [nr.STEP, nr.PARTIAL, nr.FINISH]
GRID_PASS = 8192 * 256 * 4  # coordinates one pass of the vector kernel's capped grid covers
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000,
                     0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA5A5A5, 0x7FFFFFFF,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F000000, 0xFF000000],
                    dtype=np.uint32).view(np.float32)


def _coef(C, seed=0):
    """(coef fp32 [C], tau_eff fp32): sample-count weights over uneven step counts."""
    rng = np.random.default_rng(500 + C + seed)
    n = [10 + 7 * k for k in range(C)]
    a = rng.integers(1, 140, C).tolist()
    coef, tau = nr.coefficients([x / sum(n) for x in n], a)
    return np.asarray(coef, dtype=F), F(tau)


def _data(C, P, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P).astype(F)
    rows = (g + 0.1 * rng.standard_normal((C, P))).astype(F)
    return rows, g


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show).  Returns the view
    and the whole buffer."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view, flat


def _window(x, offset):
    """x [P] inside a sentinel-filled buffer, `offset` floats from its 16-B aligned base."""
    P = x.shape[0]
    buf = torch.full((P + 16,), SENTINEL, device=DEV)
    buf[offset:offset + P].copy_(torch.from_numpy(x))
    return buf, buf[offset:offset + P], offset


def _sentinels_intact(win, P):
    buf, _, offset = win
    b = buf.cpu().numpy()
    return (b[:offset] == SENTINEL).all() and (b[offset + P:] == SENTINEL).all()


def _bits(t):
    return t.view(torch.int32).clone()


def _run(mode, placed, coef, g, tau, goff=4, ooff=4, row_index=None):
    """One launch with copies of g and a fresh out placed `goff` / `ooff` floats from aligned
    bases; returns out as numpy.  Nothing but out[0:P] may have changed."""
    view, flat = placed
    P = g.shape[0]
    wg, wo = _window(g, goff), _window(np.full(P, UNWRITTEN, dtype=F), ooff)
    c32 = None if coef is None else torch.from_numpy(np.asarray(coef, dtype=F)).to(DEV)
    before = _bits(flat)
    out = ops.fednova_rows(view, c32, wg[1], wo[1], float(tau), mode, row_index=row_index, P=P)
    torch.cuda.synchronize()
    assert out is wo[1]
    assert _sentinels_intact(wg, P) and _sentinels_intact(wo, P)
    assert nr.same_bits(wg[1].cpu().numpy(), g)          # global is only read
    assert torch.equal(_bits(flat), before)               # rows and the gaps after them too
    return wo[1].cpu().numpy()


def _layouts(P):
    """(name, row stride, rows offset, global offset, out offset), offsets in floats."""
    vec, odd = (P + 3) // 4 * 4 + 4, (P | 1) + 2 * (P % 4 == 3)
    assert vec % 4 == 0 and odd % 4 != 0 and odd >= P
    return [("vector", vec, 0, 4, 4), ("stride % 4 != 0", odd, 0, 4, 4),
            ("rows + 4 B", vec, 1, 4, 4), ("global + 4 B", vec, 0, 1, 4),
            ("out + 4 B", vec, 0, 4, 1)]


def _index_cases(C, rng):
    """(name, number of rows in the matrix, picked rows or None)."""
    tall = C + 3
    return [("no index", C, None), ("permutation", C, rng.permutation(C)),
            ("descending subset", tall, np.sort(rng.permutation(tall)[:C])[::-1].copy())]


@pytest.mark.parametrize("mode", [nr.STEP, nr.PARTIAL])
def test_fednova_bits(mode):
    for C in CS:
        coef, tau = _coef(C)
        rng = np.random.default_rng(C)
        for P in PS:
            for iname, nrows, pick in _index_cases(C, rng):
                rows, g = _data(nrows, P, 1000 * C + P)
                want = nr.fednova_rows(mode, rows if pick is None else rows[pick], coef, g, tau)
                idx = None if pick is None else torch.tensor(pick, dtype=torch.int32, device=DEV)
                placed = {}
                for name, stride, roff, goff, ooff in _layouts(P):
                    if (stride, roff) not in placed:
                        placed[stride, roff] = _place(rows, stride, roff)
                    got = _run(mode, placed[stride, roff], coef, g, tau, goff, ooff, idx)
                    assert nr.same_bits(got, want), (C, P, iname, name)


def test_fednova_finish_bits():
    """FINISH: the one row is the sum (here a PARTIAL result), alone, or picked out of a taller
    matrix by a one-element index."""
    for C in CS:
        coef, tau = _coef(C)
        for P in PS:
            rows, g = _data(C, P, 77 * C + P)
            acc = nr.fednova_rows(nr.PARTIAL, rows, coef, g)
            want = nr.fednova_rows(nr.FINISH, acc, None, g, tau)
            assert nr.same_bits(want, nr.fednova_rows(nr.STEP, rows, coef, g, tau))
            tall = np.stack([rows[0], acc, g])
            one = torch.tensor([1], dtype=torch.int32, device=DEV)
            for name, stride, roff, goff, ooff in _layouts(P):
                got = _run(nr.FINISH, _place(acc[None], stride, roff), None, g, tau, goff, ooff)
                assert nr.same_bits(got, want), (C, P, name)
                got = _run(nr.FINISH, _place(tall, stride, roff), None, g, tau, goff, ooff, one)
                assert nr.same_bits(got, want), (C, P, name, "index")


def _special_data(C, P, seed):
    """±0, denormals, ±Inf, NaNs of both signs and payloads, rows equal to the global (d = 0),
    zero coefficients and magnitudes near FLT_MAX whose difference overflows."""
    rng = np.random.default_rng(seed)
    rows, g = _data(C, P, seed)
    coef, tau = _coef(C, seed)
    coef[rng.integers(C)] = 0.0
    if C > 2:
        coef[rng.integers(C)] = -0.0
    for j in range(P):
        s = SPECIALS[(j // 8) % len(SPECIALS)]
        k = j % 8
        if k == 0:
            rows[rng.integers(C), j] = s
        elif k == 1:
            g[j] = s
        elif k == 2:    # d = 0 for every client, either sign of zero in g
            g[j] = F(0.0) if j % 16 < 8 else s
            rows[:, j] = g[j]
        elif k == 3:    # FLT_MAX against -FLT_MAX: the difference overflows
            g[j] = F(3.4028235e38) if j % 16 < 8 else F(-3.0e38)
            rows[:, j] = -g[j]
        elif k == 4:    # denormal differences and sums, global zero: out stays denormal
            g[j] = F(0.0) if j % 16 < 8 else F(-0.0)
            rows[:, j] = F(1e-40) * F(1 + j % 5)
        elif k == 5:    # products that underflow into the denormals
            g[j] = F(1e-30)
            rows[:, j] = F(1e-30) + F(1e-36) * rng.standard_normal(C).astype(F)
        elif k == 6:    # signed zeros everywhere
            rows[:, j] = F(-0.0)
            g[j] = F(-0.0) if j % 16 < 8 else F(0.0)
        else:           # every row special
            rows[:, j] = SPECIALS[(j + np.arange(C)) % len(SPECIALS)]
    return rows, g, coef, tau


def _denormal(x):
    b = np.ascontiguousarray(x, dtype=F).view(np.uint32) & 0x7FFFFFFF
    return (b > 0) & (b < 0x00800000)


@pytest.mark.parametrize("mode", MODES)
def test_fednova_special_values(mode):
    seen_nan = seen_den = 0
    for C in (1, 3, 5):
        for P in (255, 1027):
            rows, g, coef, tau = _special_data(C, P, 31 * C + P)
            if mode == nr.FINISH:   # the sum itself carries the specials
                coef, rows = None, rows[:1]
            else:
                # unit coefficients beside the zeros: the denormal columns stay denormal
                coef = np.where(coef == 0, coef, F(1.0)).astype(F)
                tau = F(1.0)
            want = nr.fednova_rows(mode, rows, coef, g, tau)
            for name, stride, roff, goff, ooff in _layouts(P)[:3]:
                got = _run(mode, _place(rows, stride, roff), coef, g, tau, goff, ooff)
                assert nr.same_bits(got, want), (C, P, name)
                nan = np.isnan(got)
                assert (got.view(np.uint32)[nan] == nr.QNAN_BITS).all()   # one NaN pattern
                seen_nan += int(nan.sum())
                seen_den += int(_denormal(got).sum())
    assert seen_nan > 0 and seen_den > 0    # NaNs were made, denormals were not flushed


def test_grid_stride_past_one_pass():
    """P = one pass of the capped vector grid + 5: the last float4 is a second trip of the
    grid-stride loop, the last coordinate the scalar tail."""
    C, P = 2, GRID_PASS + 5
    rng = np.random.default_rng(11)
    g = rng.standard_normal(P, dtype=F)
    rows = np.stack([g + F(0.1) * rng.standard_normal(P, dtype=F) for _ in range(C)])
    coef, tau = _coef(C)
    want = nr.fednova_rows(nr.STEP, rows, coef, g, tau)
    got = _run(nr.STEP, _place(rows, P + 3, 0), coef, g, tau)
    assert nr.same_bits(got, want)


def test_aliasing_out_is_global_or_rows():
    C = 5
    coef, tau = _coef(C)
    c32 = torch.from_numpy(coef).to(DEV)
    for P in (5, 1027):
        rows, g = _data(C, P, 9 + P)
        acc = nr.fednova_rows(nr.PARTIAL, rows, coef, g)
        want = nr.fednova_rows(nr.STEP, rows, coef, g, tau)
        for name, stride, roff, goff, _ in _layouts(P)[:4]:
            placed = _place(rows, stride, roff)
            assert nr.same_bits(_run(nr.STEP, placed, coef, g, tau, goff), want)
            # STEP, out is global
            wg = _window(g, goff)
            assert ops.fednova_rows(placed[0], c32, wg[1], wg[1], float(tau), nr.STEP,
                                    P=P) is wg[1]
            assert nr.same_bits(wg[1].cpu().numpy(), want) and _sentinels_intact(wg, P), name
            # FINISH, out is global
            wg = _window(g, goff)
            ops.fednova_rows(_place(acc[None], stride, roff)[0], None, wg[1], wg[1], float(tau),
                             nr.FINISH, P=P)
            assert nr.same_bits(wg[1].cpu().numpy(), want) and _sentinels_intact(wg, P), name
            # FINISH, out is rows: the sum is replaced by the new global in place
            wg, wa = _window(g, goff), _window(acc, 4 + roff)
            ops.fednova_rows(wa[1].view(1, -1), None, wg[1], wa[1], float(tau), nr.FINISH, P=P)
            assert nr.same_bits(wa[1].cpu().numpy(), want) and _sentinels_intact(wa, P), name
            assert nr.same_bits(wg[1].cpu().numpy(), g) and _sentinels_intact(wg, P)


def test_partial_partial_add_finish_composition():
    """Two ranks' worth: PARTIAL over two disjoint client subsets, the two sums added in fp32,
    FINISH.  Held to the reference of the SAME composition (STEP sums in another order)."""
    C, P = 9, 1027
    rows, g = _data(C, P, 4)
    coef, tau = _coef(C)
    a, b = [0, 3, 4, 8, 6], [7, 1, 2, 5]
    placed = _place(rows, 1028, 0)
    parts = []
    for pick in (a, b):
        idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
        got = _run(nr.PARTIAL, placed, coef[pick], g, 0.0, row_index=idx)
        assert nr.same_bits(got, nr.fednova_rows(nr.PARTIAL, rows[pick], coef[pick], g))
        parts.append(torch.from_numpy(got).to(DEV))
    total = parts[0] + parts[1]
    want_sum = nr.fednova_rows(nr.PARTIAL, rows[a], coef[a], g) \
        + nr.fednova_rows(nr.PARTIAL, rows[b], coef[b], g)
    assert want_sum.dtype == F and nr.same_bits(total.cpu().numpy(), want_sum)
    got = _run(nr.FINISH, (total.view(1, -1), total), None, g, tau)
    assert nr.same_bits(got, nr.fednova_rows(nr.FINISH, want_sum, None, g, tau))


def test_exact_identity_with_the_fedavg_kernel():
    """Small-integer rows and global, power-of-two weights, equal power-of-two step counts:
    every operation is exact and FedNova gives fh_fedavg_weighted_sum's bits."""
    rng = np.random.default_rng(3)
    for w, a in (([0.25] * 4, 4), ([0.5, 0.25, 0.125, 0.125], 8), ([1.0], 2), ([0.5, 0.5], 1)):
        C, P = len(w), 1027
        rows = rng.integers(-64, 65, (C, P)).astype(F)
        g = rng.integers(-64, 65, P).astype(F)
        coef, tau = ops.fednova_coefficients(w, [a] * C)
        view, _ = _place(rows, 1028, 0)
        fedavg = torch.full((P,), UNWRITTEN, device=DEV)
        ops.fedavg_weighted_sum(view, torch.tensor(w, dtype=torch.float32, device=DEV), fedavg,
                                P=P)
        want = fedavg.cpu().numpy()
        assert nr.same_bits(want, nr.weighted_sum(rows, w))
        assert nr.same_bits(_run(nr.STEP, (view, view), coef, g, tau), want)
        part = _run(nr.PARTIAL, (view, view), coef, g, 0.0)
        assert nr.same_bits(_run(nr.FINISH, _place(part[None], 1028, 0), None, g, tau), want)


def test_fednova_argument_errors():
    rows = torch.zeros(3, 8, device=DEV)
    c3 = torch.full((3,), 1 / 3, device=DEV)
    g = torch.zeros(8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)

    # the C ABI, called directly: every FH_E_INVALID case of include/fedhip.h
    def raw(rows=rows, coef=c3, C=3, P=8, g=g, tau=1.0, mode=nr.STEP, out=out):
        _lib.call("fh_fednova_rows", _lib.ptr(rows), 8, None, _lib.ptr(coef), C, P, _lib.ptr(g),
                  tau, mode, _lib.ptr(out), _lib.stream_handle())
    for kw, msg in (({"mode": 3}, "outside"), ({"mode": -1}, "outside"),
                    ({"C": 0}, "num_clients"), ({"C": -2}, "num_clients"),
                    ({"mode": nr.FINISH, "C": 2}, "FINISH"), ({"P": -1}, "bad sizes"),
                    ({"rows": None}, "null pointer"), ({"g": None}, "null pointer"),
                    ({"out": None}, "null pointer"), ({"coef": None}, "null pointer"),
                    ({"coef": None, "mode": nr.PARTIAL}, "null pointer"),
                    ({"tau": float("inf")}, "non-finite"), ({"tau": float("nan")}, "non-finite"),
                    ({"tau": 1e39}, "non-finite"),
                    ({"tau": float("-inf"), "mode": nr.FINISH, "C": 1}, "non-finite")):
        with pytest.raises(FedHipError, match=msg):
            raw(**kw)
    raw(P=0)                                        # a no-op, whatever the pointers
    raw(P=0, rows=None, g=None, out=None, coef=None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()    # nothing was launched
    scratch = torch.empty(8, device=DEV)
    raw(mode=nr.PARTIAL, tau=float("nan"), out=scratch)   # PARTIAL ignores tau_eff
    raw(mode=nr.FINISH, C=1, coef=None, out=scratch)      # FINISH needs no coefficients
    torch.cuda.synchronize()
    assert not scratch.isnan().any()

    # the binding: refused in Python, before any launch
    def call(rows=rows, coef=c3, g=g, out=out, tau=1.0, mode=nr.STEP, **kw):
        ops.fednova_rows(rows, coef, g, out, tau, mode, **kw)
    i3 = torch.arange(3, dtype=torch.int32, device=DEV)
    for kw, msg in (({"mode": 3}, "outside"), ({"mode": -1}, "outside"),
                    ({"coef": None}, "required"), ({"coef": c3[:0]}, "no client"),
                    ({"mode": nr.FINISH}, "not coefficients"),
                    ({"mode": nr.FINISH, "coef": None}, "ONE row"),
                    ({"tau": float("inf")}, "not finite"), ({"tau": float("nan")}, "not finite"),
                    ({"tau": 1e39, "mode": nr.FINISH, "coef": None, "rows": rows[:1]},
                     "not finite"),
                    ({"rows": torch.zeros(3, 8)}, "HIP device"),
                    ({"g": torch.zeros(8)}, "HIP device"), ({"out": torch.zeros(8)}, "HIP device"),
                    ({"g": None}, "required"), ({"out": None}, "required"),
                    ({"rows": rows[0]}, "matrix"), ({"rows": rows[:2]}, "2 rows for 3"),
                    ({"row_index": i3[:2]}, "2 row indices for 3"),
                    ({"row_index": i3.long()}, "int32"),
                    ({"g": g[:7]}, "at least P=8"), ({"out": out[:7]}, "at least P=8"),
                    ({"P": 9}, "at least P=9"), ({"P": -1}, "at least P=-1"),
                    ({"rows": rows.double()}, "float32"), ({"g": g.double()}, "float32"),
                    ({"coef": c3.double()}, "float32"),
                    ({"rows": torch.zeros(8, 3, device=DEV).t()}, "unit column stride"),
                    ({"out": torch.zeros(8, 2, device=DEV)[:, 0]}, "contiguous")):
        with pytest.raises(FedHipError, match=msg):
            call(**kw)
    call(P=0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------ FedNovaAggregator
SHAPES = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}


def _np(t):
    return t.detach().cpu().numpy()


def _want_step(rows, samples, steps, g, tau_eff="weighted"):
    coef, tau = nr.coefficients([n / sum(samples) for n in samples], steps, tau_eff)
    return nr.fednova_rows(nr.STEP, rows, np.asarray(coef, dtype=F), g, F(tau))


def test_aggregate_packed_against_the_reference():
    tall, P, stride = 7, 1001, 1008
    pick, n, steps = [5, 0, 3, 6], [30, 10, 25, 40], [4, 1, 131, 5]
    rng = np.random.default_rng(21)
    g = rng.standard_normal(P).astype(F)
    rows = (g + 0.05 * rng.standard_normal((tall, P))).astype(F)
    packed, _ = _place(rows, stride, 0)
    gd = torch.from_numpy(g).to(DEV)
    agg = FedNovaAggregator(device=DEV)
    got = agg.aggregate_packed(packed, n, steps, gd, row_index=pick)
    assert nr.same_bits(_np(got), _want_step(rows[pick], n, steps, g))
    assert nr.same_bits(_np(gd), g)
    # no index: every row, in order; out may be the global itself; an explicit tau_eff
    agg3 = FedNovaAggregator(device=DEV, tau_eff=3)
    four, _ = _place(rows[:4], stride, 0)
    assert agg3.aggregate_packed(four, n, steps, gd, out=gd) is gd
    assert nr.same_bits(_np(gd), _want_step(rows[:4], n, steps, g, 3))
    # an empty shard: no step, no samples, coefficient 0
    gd = torch.from_numpy(g).to(DEV)
    got = agg.aggregate_packed(four, [30, 0, 25, 40], [4, 0, 131, 5], gd)
    assert nr.same_bits(_np(got), _want_step(rows[:4], [30, 0, 25, 40], [4, 0, 131, 5], g))
    for bad in (lambda: agg.aggregate_packed(four, n, steps[:3], gd),
                lambda: agg.aggregate_packed(four, n, [4, 0, 131, 5], gd),
                lambda: agg.aggregate_packed(four, n, [4, -1, 131, 5], gd),
                lambda: agg.aggregate_packed(packed, n, steps, gd),
                lambda: agg.aggregate_packed(four, [], [], gd)):
        with pytest.raises(FedAvgError):
            bad()
    with pytest.raises(ValueError):
        FedNovaAggregator(device=DEV, tau_eff="mean")


def _flat(weights):
    return np.concatenate([_np(weights[n]).reshape(-1) for n in SHAPES])


def test_aggregate_updates_with_steps_as_mapping_and_sequence():
    gen = torch.Generator().manual_seed(4)
    prev_w = {name: 0.3 * torch.randn(*shape, generator=gen) for name, shape in SHAPES.items()}
    prev = GlobalModel(round_number=3, model_weights=prev_w, accuracy_metrics={},
                       participating_clients=[], convergence_score=0.0)
    ups, samples, steps = [], [10, 11, 12], [2, 40, 7]
    for k in range(3):
        wts = {name: t + 0.05 * torch.randn(*t.shape, generator=gen)
               for name, t in prev_w.items()}
        ups.append(ModelUpdate(client_id=f"c{k}", round_number=4, model_weights=wts,
                               num_samples=samples[k], training_loss=0.5,
                               privacy_budget_used=0.5, compression_ratio=0.8,
                               timestamp=datetime.now()))
    rows = np.stack([_flat(u.model_weights) for u in ups])
    g0 = _flat(prev_w)
    want = _want_step(rows, samples, steps, g0)
    assert not nr.same_bits(want, nr.weighted_sum(rows, [n / 33 for n in samples]))
    agg = FedNovaAggregator(device=DEV)
    for local_steps in ({"c2": 7, "c0": 2, "c1": 40, "other": 9}, steps, tuple(steps)):
        gm = agg.aggregate_updates(ups, prev, local_steps)
        assert gm.round_number == 4 and gm.participating_clients == ["c0", "c1", "c2"]
        assert [gm.model_weights[n].shape for n in SHAPES] == \
            [torch.Size(s) for s in SHAPES.values()]
        assert nr.same_bits(_flat(gm.model_weights), want)
        assert nr.same_bits(_flat(prev_w), g0)   # the global model is not stepped in place
    assert agg.aggregation_history[-1]["client_samples"]["c2"] == 12
    assert not hasattr(ups[0], "local_steps")
    bad_prev = GlobalModel(5, {"fc.bias": prev_w["fc.bias"]}, {}, [], 0.0)
    for bad in (lambda: agg.aggregate_updates([], prev, []),
                lambda: agg.aggregate_updates(ups, prev, {"c0": 2, "c1": 40}),
                lambda: agg.aggregate_updates(ups, prev, [2, 40]),
                lambda: agg.aggregate_updates(ups, prev, [2, 0, 7]),
                lambda: agg.aggregate_updates(ups, bad_prev, steps)):
        with pytest.raises(FedAvgError):
            bad()


# ------------------------------------------------------------------ RankRound
SIZES, BATCH = [8, 40, 100], 8      # 1, 5 and 13 local steps
STEPS = nr.local_steps(SIZES, BATCH)


def _rounds(mine, nrounds=1, model_name="simple_cnn", **kw):
    """`nrounds` rounds over SIZES' clients `mine` on one RankRound.  Returns the RankRound, the
    global vector before round one, and per round (the trained rows by client, copied by the
    on_trained hook; the global vector; global_bufs)."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    shape = (1, 28, 28) if model_name == "simple_cnn" else (3, 32, 32)
    model = hm.ModelFactory.create_model(model_name, dropout_rate=0.0).to(DEV)
    r = RankRound(model, SIZES, mine, epochs=1, batch=BATCH, device=DEV, lanes=1, dp_seed=11,
                  shuffle_seed=77, **kw)
    xs, ys = [], []
    for k in r.slots:
        gen = torch.Generator().manual_seed(200 + k)
        xs.append(torch.randn(SIZES[k], *shape, generator=gen))
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
        r.run(data, labels, offs, "sgd", 0.01, seed=3 + i)
        torch.cuda.synchronize()
        out.append((dict(seen), _np(r.global_flat).copy(), _np(r.global_bufs).copy()))
    return r, start, out


def _round_coef(weights):
    coef, tau = nr.coefficients(weights, STEPS)
    return np.asarray(coef, dtype=F), F(tau)


def test_rankround_one_rank_two_rounds():
    all3 = list(range(3))
    (r, g, rounds), (rp, gp, plain) = _rounds(all3, 2, fednova=True), \
        _rounds(all3, 1, fednova=None)
    assert r.clients == [0, 1, 2] and [r.epochs * -(-n // r.B) for n in SIZES] == [1, 5, 13]
    coef, tau = _round_coef(r.weights)
    assert nr.same_bits(_np(r._nova_c32), coef) and F(r._nova_tau) == tau
    assert nr.same_bits(g, gp)
    for i, (rows, glob, _) in enumerate(rounds):
        stack = np.stack([rows[k] for k in r.clients])
        g = nr.fednova_rows(nr.STEP, stack, coef, g, tau)
        assert nr.same_bits(glob, g), f"round {i + 1}"
    # round one trains from the same start on the same batches: the same rows go in, another
    # global comes out, and the BN running statistics do not see FedNova
    for k in r.clients:
        assert nr.same_bits(rounds[0][0][k], plain[0][0][k])
    stack = np.stack([plain[0][0][k] for k in rp.clients])
    assert nr.same_bits(plain[0][1], nr.weighted_sum(stack, _np(rp.w32)))
    assert not nr.same_bits(rounds[0][1], plain[0][1])
    assert nr.same_bits(rounds[0][2], plain[0][2])
    # fednova=None is today's path: the same bits as without the argument
    _, _, omitted = _rounds([0, 1, 2], 1)
    assert nr.same_bits(omitted[0][1], plain[0][1]) and nr.same_bits(omitted[0][2], plain[0][2])


def test_rankround_bn_statistics_keep_the_plain_fedavg():
    """A model with BatchNorm: global_bufs after round one is the plain run's, bit for bit, and
    the parameters are FedNova's."""
    all3 = list(range(3))
    r, g, rounds = _rounds(all3, 1, "cifar10_cnn", fednova=FedNovaConfig())
    rp, _, plain = _rounds(all3, 1, "cifar10_cnn")
    assert r.Q > 0 and rounds[0][2].any()
    assert nr.same_bits(rounds[0][2], plain[0][2])
    coef, tau = _round_coef(r.weights)
    stack = np.stack([rounds[0][0][k] for k in all3])
    assert nr.same_bits(rounds[0][1], nr.fednova_rows(nr.STEP, stack, coef, g, tau))
    assert not nr.same_bits(rounds[0][1], plain[0][1])


def _init_state(so, P):
    tau32 = F(so.tau)
    return np.zeros(P, dtype=F), np.full(P, tau32 * tau32, dtype=F)


def _scalars(so):
    return dict(server_lr=so.server_lr, beta1=so.beta1, beta2=so.beta2, tau=so.tau)


def test_rankround_one_rank_fedadam_steps_toward_the_fednova_aggregate():
    so = fedopt.FedAdam(0.01, device=DEV)
    r, g, rounds = _rounds([0, 1, 2], 2, fednova=True, server_opt=so)
    coef, tau = _round_coef(r.weights)
    m, v = _init_state(so, r.P)
    for i, (rows, glob, _) in enumerate(rounds):
        stack = np.stack([rows[k] for k in r.clients])
        agg = nr.fednova_rows(nr.STEP, stack, coef, g, tau)
        g, m, v = fr.server_opt_step(fr.ADAM, agg[None], None, g, m, v, **_scalars(so))
        assert nr.same_bits(glob, g), f"round {i + 1}"
    assert nr.same_bits(_np(r.partial), agg)
    assert nr.same_bits(_np(so.m), m) and nr.same_bits(_np(so.v), v)


def test_rankround_sparse_payload_run_equals_the_dense_run():
    """Under FedNova the sums from the payload are off: the dense rows are rebuilt, and the
    sparse=True run is the sparse=False run bit for bit."""
    from fedhip.compress import CompressionConfig
    runs = []
    for sparse in (False, True):
        cfg = CompressionConfig("topk", sparsity_ratio=0.9, sparse=sparse)
        r, _, rounds = _rounds([0, 1, 2], 2, fednova=True, compression=cfg)
        assert not r._sparse_sum() and not r._quant_sum()
        runs.append(rounds)
    assert r.last_sparse is not None
    for a, b in zip(*runs):
        assert nr.same_bits(a[1], b[1]) and nr.same_bits(a[2], b[2])
    assert not nr.same_bits(runs[0][0][1], runs[0][1][1])


def test_rankround_refusals():
    from fedhip.round import RankRound
    from src.aggregation import dpfedavg
    from src.shared import models_pytorch as hm
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    for kw, msg in (({"aggregator": robust.MedianAggregator()}, "robust"),
                    ({"server_opt": fedopt.FedYogi(0.01, base=robust.MedianAggregator(),
                                                   device=DEV)}, "robust"),
                    ({"central_dp": dpfedavg.CentralDPConfig(1.1, 0.05)}, "uniform weights"),
                    ({"fednova": FedNovaConfig(tau_eff=-1.0)}, "tau_eff"),
                    ({"fednova": FedNovaConfig(tau_eff="mean")}, "tau_eff")):
        kw.setdefault("fednova", True)
        with pytest.raises(FedHipError, match=msg):
            RankRound(model, SIZES, [0, 1, 2], epochs=1, batch=BATCH, device=DEV, lanes=1, **kw)


def _rank_main(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        res = {}
        for name, exact in (("all_reduce", False), ("exact", True)):
            r, start, rounds = _rounds(mine, 1, fednova=True, exact=exact)
            res[name] = (start, rounds[0][0], rounds[0][1], list(r.clients), list(r.weights))
        q.put((rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def test_rankround_two_ranks_all_reduce_and_exact():
    """Two gloo ranks on cuda:0.  All-reduce mode: both ranks end with the same global vector,
    the reference's PARTIAL per rank (client-list order), the two added, FINISH.  exact=True:
    the one-launch STEP reference over all clients in global client order."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29960 + os.getpid() % 200
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
    for name in ("all_reduce", "exact"):
        (s0, rows0, g0, c0, w0), (s1, rows1, g1, c1, w1) = res[0][name], res[1][name]
        assert sorted(c0 + c1) == [0, 1, 2] and w0 == w1
        assert nr.same_bits(s0, s1)
        assert nr.same_bits(g0, g1), f"{name}: ranks disagree on the global model"
        coef, tau = _round_coef(w0)
        rows = {**rows0, **rows1}
        if name == "all_reduce":
            parts = [nr.fednova_rows(nr.PARTIAL, np.stack([rows[k] for k in c]), coef[c], s0)
                     for c in (c0, c1)]
            total = parts[0] + parts[1]
            assert total.dtype == F
            want = nr.fednova_rows(nr.FINISH, total, None, s0, tau)
        else:
            want = nr.fednova_rows(nr.STEP, np.stack([rows[k] for k in range(3)]), coef, s0, tau)
        assert nr.same_bits(g0, want), name
        assert not nr.same_bits(g0, s0)
