"""Central DP-FedAvg (csrc/dpfedavg.hip) and what is built on it, on the GPU, against the numpy
reference of tests/dpfedavg_ref.py (pinned by test_dpfedavg_ref_cpu.py) and the Philox
reference of tests/philox_ref.py.

fh_dpfa_clip_sum is held to the reference bit for bit (uint32 views) with the reference's own
scales and injected noise: client counts around the rows-in-flight unroll, sizes below / across
the 4-column vector width, the 256-thread block and one pass of the capped grid, through the
vector path and every way onto the scalar path.  The norms are held to the exact sum within
the worst case of any-order fp64 summation, the coefficients and sigma to one fp32 ulp, the
Philox noise to philox_ref.GAUSS_TOL, the clip update to that tolerance carried through the
exponent.  No expected value comes from the code under test.

Measured on the MI355X (each test prints its figures before it asserts), as a share of the bound:
  norms      |n2 - fsum| / (P 2^-53 n2)              0.0016 worst (0 at P = 8,388,613)
  scale      0 ulp on every row, sigma 0 ulp         (bound: 1 ulp)
  noise      |nu - sigma G| / (sigma (GAUSS_TOL + 2^-24 |G|))   0.10 worst
  clip norm  |ln C_gpu - ln C_ref| <= 1.1e-8         (bound per round: 1.6e-7 .. 7.9e-7)
"""
import math
import os
from datetime import datetime

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dpfedavg_ref as dr
import fedopt_ref as fr
import philox_ref as pr
from fedhip import ops
from fedhip._lib import FedHipError
from src.aggregation import dpfedavg, fedopt, robust
from src.aggregation.fedavg import FedAvgError
from src.shared.models import GlobalModel, ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
F = np.float32

CS = [1, 2, 3, 4, 5, 9, 33]
PS = [1, 3, 13, 1001, 4099]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000,
                     0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA5A5A5, 0x7FFFFFFF],
                    dtype=np.uint32).view(np.float32)
GRID_PASS = 8192 * 256 * 4  # coordinates one pass of the vector kernel's capped grid covers
Z = 1.1


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _data(C, P, seed):
    """(rows [C, P], g): deltas of norms spread over a decade and a half around 0.1 sqrt(P)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P).astype(F)
    mag = 10.0 ** rng.uniform(-1.5, 0.0, (C, 1))
    rows = (g + mag * 0.1 * rng.standard_normal((C, P))).astype(F)
    return rows, g


def _clip_between(norms):
    """A clip norm no norm is near: the geometric mean of the two middle norms (one norm:
    twice it), so some rows are clipped and some are not."""
    n = np.sort(np.asarray(norms, dtype=np.float64))
    if len(n) == 1:
        return 2.0 * float(n[0])
    return float(math.sqrt(n[len(n) // 2 - 1] * n[len(n) // 2]))


def _not_near(norms, clip):
    """The condition on the inputs under which b_k must equal the reference."""
    return bool((np.abs(np.asarray(norms) - clip) > 1e-9 * clip).all())


def _specials_into(rows, g, seed):
    rng = np.random.default_rng(seed)
    C, P = rows.shape
    for j in range(P):
        s = SPECIALS[(j // 4) % len(SPECIALS)]
        k = j % 4
        if k == 0:
            rows[rng.integers(C), j] = s
        elif k == 1:
            g[j] = s
        elif k == 2:   # signed zeros: a zero delta, a zero g
            rows[:, j] = F(-0.0)
            g[j] = F(-0.0) if j % 8 < 4 else F(0.0)
        else:          # products that underflow to a denormal or to zero
            g[j] = F(0.0)
            rows[:, j] = F(1e-38) if j % 8 < 4 else F(-3e-44)


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show)."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


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


def _sum(view, scale, g, noise=None, offs=(4, 4, 4), alias=False, **kw):
    """One fh_dpfa_clip_sum launch; g / out / noise placed `offs` floats into their windows.
    alias: out IS the global window.  Returns out as numpy."""
    P = view.shape[1]
    wg = None if g is None else _window(g, offs[0])
    wo = wg if alias else _window(np.full(P, 7.0, dtype=F), offs[1])
    wn = None if noise is None else _window(noise, offs[2])
    out = ops.dpfa_clip_sum(view, _dev(np.asarray(scale, dtype=F)), wo[1],
                            global_=None if wg is None else wg[1],
                            noise=None if wn is None else wn[1], P=P, **kw)
    torch.cuda.synchronize()
    assert out is wo[1]
    assert all(_sentinels_intact(w, P) for w in (wg, wo, wn) if w is not None)
    if wg is not None and not alias:
        assert dr.same_bits(_np(wg[1]), g)  # g is read only
    return _np(wo[1])


def _layouts(P):
    vec, odd = (P + 3) // 4 * 4 + 4, P | 1
    return [("vector", vec, 0, (4, 4, 4)), ("odd stride", odd, 0, (4, 4, 4)),
            ("rows + 4 B", vec, 1, (4, 4, 4)), ("global + 4 B", vec, 0, (1, 4, 4)),
            ("out + 4 B", vec, 0, (4, 1, 4)), ("noise + 4 B", vec, 0, (4, 4, 1))]


def _case(C, P, seed, special=False):
    """(rows, g, scale, noise): scales and noise from the reference."""
    rows, g = _data(C, P, seed)
    sq = dr.sqnorms(rows, g)
    clip = _clip_between(np.sqrt(sq))
    _, scale = dr.clip_coef(sq, clip, C)
    noise = (dr.sigma_avg(Z, clip, C) * dr.gauss(seed, P)).astype(F)
    if special:
        _specials_into(rows, g, seed)
        noise[3::7] = SPECIALS[np.arange(len(noise[3::7])) % len(SPECIALS)]
    return rows, g, scale, noise


# ------------------------------------------------------------------ the sum kernel
@pytest.mark.parametrize("special", [False, True])
def test_clip_sum_bits(special):
    for C in CS:
        for P in PS:
            rows, g, scale, noise = _case(C, P, 1000 * C + P, special)
            want = dr.clipped_sum(rows, scale, g, noise=noise)
            want0 = dr.clipped_sum(rows, scale, g)  # no noise: no add
            views = {}
            for name, stride, roff, offs in _layouts(P):
                if (stride, roff) not in views:
                    views[stride, roff] = _place(rows, stride, roff)
                got = _sum(views[stride, roff], scale, g, noise, offs)
                assert dr.same_bits(got, want), (C, P, name)
                got = _sum(views[stride, roff], scale, g, None, offs, alias=name != "out + 4 B")
                assert dr.same_bits(got, want0), (C, P, name, "no noise")
    assert not dr.same_bits(want, want0)


def test_row_index_picks_rows_in_its_order_and_out_may_be_global():
    C, tall, P = 5, 11, 1001
    rng = np.random.default_rng(3)
    rows, g = _data(tall, P, 300)
    _specials_into(rows, g, 301)
    pick = rng.permutation(tall)[:C]
    noise = (0.01 * rng.standard_normal(P)).astype(F)
    scale = (rng.random(C) / C).astype(F)
    want = dr.clipped_sum(rows[pick], scale, g, noise=noise)
    assert not dr.same_bits(want, dr.clipped_sum(rows[np.sort(pick)], scale, g, noise=noise))
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    for stride, roff in ((1008, 0), (1003, 0), (1008, 1)):
        for alias in (False, True):
            got = _sum(_place(rows, stride, roff), scale, g, noise, row_index=idx, alias=alias)
            assert dr.same_bits(got, want), (stride, roff, alias)


def test_delta_mode_partial_and_single_row_finish():
    """global None: the rows are deltas, out = the clipped sum (+ noise).  add_global=False:
    a rank's partial.  rows_are_deltas with one row and scale 1: only the noise and g are
    added (the finish of several ranks)."""
    one = np.ones(1, dtype=F)
    for C, P in ((3, 13), (4, 1001), (9, 4099)):
        rows, g, scale, noise = _case(C, P, 40 + P, special=True)
        d = dr.deltas(rows, g)
        for name, stride, roff, offs in _layouts(P)[:3]:
            view = _place(rows, stride, roff)
            dview = _place(d, stride, roff)
            part = dr.clipped_sum(rows, scale, g, add_global=False)
            assert dr.same_bits(_sum(view, scale, g, None, offs, add_global=False), part)
            assert dr.same_bits(_sum(dview, scale, None, None, offs),
                                dr.clipped_sum(d, scale)), (C, P, name)
            assert dr.same_bits(_sum(dview, scale, None, noise, offs),
                                dr.clipped_sum(d, scale, noise=noise)), (C, P, name)
            assert dr.same_bits(_sum(dview, scale, g, noise, offs, rows_are_deltas=True),
                                dr.clipped_sum(d, scale, g, noise=noise, rows_are_deltas=True))
            want = dr.clipped_sum(part[None], one, g, noise=noise, rows_are_deltas=True)
            pview = _place(part[None], stride, roff)
            assert dr.same_bits(_sum(pview, one, g, noise, offs, rows_are_deltas=True), want)
    # in place on the partial itself: out is the one row
    P = 1001
    rows, g, scale, noise = _case(4, P, 77)
    part = dr.clipped_sum(rows, scale, g, add_global=False)
    pd, gd = _dev(part), _dev(g)
    ops.dpfa_clip_sum(pd.view(1, -1), _dev(one), pd, global_=gd, noise=_dev(noise),
                      rows_are_deltas=True)
    assert dr.same_bits(_np(pd), dr.clipped_sum(part[None], one, g, noise=noise,
                                                rows_are_deltas=True))


def test_grid_stride_past_one_pass():
    """P = one pass of the capped vector grid + 5: the last full float4 is a second trip of
    the grid-stride loop, the last coordinate the partial vector; the norm pass runs 1025
    chunks per row."""
    C, P = 2, GRID_PASS + 5
    rng = np.random.default_rng(11)
    g = rng.standard_normal(P, dtype=F)
    rows = np.stack([g + F(0.1) * rng.standard_normal(P, dtype=F) for _ in range(C)])
    noise = F(0.01) * rng.standard_normal(P, dtype=F)
    scale = np.array([0.4, 0.3], dtype=F)
    view = _place(rows, P + 3, 0)
    want = dr.clipped_sum(rows, scale, g, noise=noise)
    assert dr.same_bits(_sum(view, scale, g, noise), want)
    gd = _dev(g)
    sq = _np(ops.dpfa_row_sqnorm(view, gd, P=P))
    ref = dr.sqnorms(rows, g)
    err = np.abs(sq - ref) / (P * 2.0 ** -53 * ref)
    print("norm err / bound at P = %d: %s" % (P, err))
    assert (err <= 1.0).all()


# ------------------------------------------------------------------ norms
def test_row_sqnorm_against_the_exact_sum_and_repeatable():
    """|n2 - fsum| <= P 2^-53 n2: the worst case of any-order fp64 summation of P non-negative
    terms (each square of an fp32 value is exact in fp64).  P = 20011 spans three chunks."""
    worst = 0.0
    for C in (1, 3, 5):
        for P in PS + [20011]:
            rows, g = _data(C, P, 7 * C + P)
            ref = dr.sqnorms(rows, g)
            ref0 = dr.sqnorms(rows)
            vec, odd = (P + 3) // 4 * 4 + 4, P | 1
            for name, stride, roff, goff in (("vector", vec, 0, 4), ("odd stride", odd, 0, 4),
                                             ("rows + 4 B", vec, 1, 4), ("global + 4 B", vec, 0, 1),
                                             ("both + 4 B", vec, 1, 1), ("both + 12 B", vec, 3, 3)):
                view = _place(rows, stride, roff)
                wg = _window(g, goff)
                a = _np(ops.dpfa_row_sqnorm(view, wg[1], P=P))
                b = _np(ops.dpfa_row_sqnorm(view, wg[1], P=P))
                assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
                err = (np.abs(a - ref) / (P * 2.0 ** -53 * ref)).max()
                worst = max(worst, err)
                assert err <= 1.0, (C, P, name, err)
                a0 = _np(ops.dpfa_row_sqnorm(view, None, P=P))  # the rows as deltas
                assert (np.abs(a0 - ref0) <= P * 2.0 ** -53 * ref0).all(), (C, P, name)
                assert _sentinels_intact(wg, P)
    print("norm err / bound, worst: %.3g" % worst)
    # a permuted subset of a taller matrix, written into the caller's buffer
    rows, g = _data(11, 1001, 5)
    pick = np.random.default_rng(5).permutation(11)[:5]
    out = torch.full((7,), -1.0, dtype=torch.float64, device=DEV)
    ops.dpfa_row_sqnorm(_place(rows, 1003, 0), _dev(g), P=1001, out=out,
                        row_index=torch.tensor(pick, dtype=torch.int32, device=DEV))
    ref = dr.sqnorms(rows[pick], g)
    assert (np.abs(_np(out)[:5] - ref) <= 1001 * 2.0 ** -53 * ref).all()
    assert (_np(out)[5:] == -1.0).all()


# ------------------------------------------------------------------ coefficients
def _ulps(a, b):
    """Distance in fp32 ulps between positive finite fp32 values."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _state(clip):
    st = torch.zeros(ops.DPFA_STATE_DOUBLES, dtype=torch.float64, device=DEV)
    st[ops.DPFA_CLIP] = clip
    return st


def test_clip_coef_bits_scale_and_sigma():
    """b_k equals the reference (no norm is within 1e-9 relative of C_t: checked); the norm's
    error (<= 4099 * 2^-53 relative) is far below half an fp32 ulp (2^-25), so c_k, and with it
    s_k = fl32(c_k * w), can differ from the reference by the flip of one rounding: 1 ulp.
    sigma_avg has no norm in it: 1 ulp covers the device's fp64 multiply / divide order."""
    C, P, m = 6, 4099, 10
    rows, g = _data(C, P, 21)
    rows[C - 1] = g  # a zero delta row: n = 0 gives c = 1, b = 1
    ref_sq = dr.sqnorms(rows, g)
    norms = np.sqrt(ref_sq)
    view, gd = _place(rows, 4104, 0), _dev(g)
    sq = ops.dpfa_row_sqnorm(view, gd, P=P)
    assert _np(sq)[C - 1] == 0.0
    pos = np.sort(norms[norms > 0])
    for what, clip in (("all clipped", 0.5 * pos[0]), ("none clipped", 2.0 * pos[-1]),
                       ("mixed", _clip_between(pos))):
        assert _not_near(norms, clip)
        bits_ref, s_ref = dr.clip_coef(ref_sq, clip, m)
        st = _state(clip)
        scale, bits, sigma = ops.dpfa_clip_coef(sq, st, m, Z)
        torch.cuda.synchronize()
        assert _np(bits).tolist() == bits_ref.tolist(), what
        du = _ulps(_np(scale), s_ref)
        su = _ulps(_np(sigma), np.array([dr.sigma_avg(Z, clip, m)]))
        print("%s: scale ulps %s, sigma ulps %s" % (what, du.tolist(), su.tolist()))
        assert (du <= 1).all() and (su <= 1).all(), what
        stn = _np(st)
        assert stn[ops.DPFA_CLIP] == clip and stn[ops.DPFA_BITSUM] == bits_ref.sum()
        assert stn[ops.DPFA_SIGMA] == float(_np(sigma)[0])
        assert bits_ref[C - 1] == 1 and s_ref[C - 1] == F(1) / F(m)
        if what == "all clipped":
            assert bits_ref.sum() == 1  # only the zero row
        if what == "none clipped":
            assert bits_ref.all() and dr.same_bits(_np(scale), s_ref)
        if what == "mixed":
            assert 1 < bits_ref.sum() < C


# ------------------------------------------------------------------ the Philox noise
@pytest.mark.parametrize("seed", [0x1234, 0xFEDCBA9876543210])
def test_philox_noise_stream(seed):
    """Zero rows in delta mode: out_j = nu_j = fl32(sigma * G_j) exactly.  |nu_j - sigma G_j^ref|
    <= sigma * (GAUSS_TOL + 2^-24 |G_j^ref|): the fp32 Box-Muller's tolerance (philox_ref) and
    the rounding of the product."""
    P, sigma = 4099, F(0.37)
    zeros = torch.zeros(1, P + 1, device=DEV)[:, :P]
    out = torch.empty(P, device=DEV)
    sg = _dev(np.array([sigma], dtype=F))
    ops.dpfa_clip_sum(zeros, _dev(np.ones(1, dtype=F)), out, sigma=sg, seed=seed)
    nu = _np(out).astype(np.float64)
    G = dr.gauss(seed, P)
    err = np.abs(nu - float(sigma) * G) / (float(sigma) * (pr.GAUSS_TOL + 2.0 ** -24 * np.abs(G)))
    print("noise err / bound, worst: %.3g" % err.max())
    assert (err <= 1.0).all()
    assert 0.9 < nu.std() / float(sigma) < 1.1
    # the scalar path draws the same stream: bit for bit the vector path's
    out2 = torch.empty(P + 1, device=DEV)[1:]
    ops.dpfa_clip_sum(zeros, _dev(np.ones(1, dtype=F)), out2, sigma=sg, seed=seed)
    assert dr.same_bits(_np(out2), _np(out))
    # the server's stream is no client's: rows keyed 0..3 of the same seed differ from it
    for key in range(4):
        other = float(sigma) * pr.gauss_row(seed, key, P)
        assert (np.abs(nu - other) > float(sigma) * 1e-3).mean() > 0.99, key
    # on real rows: out = g + (acc + nu) with the device's own nu, bit for bit
    rows, g, scale, _ = _case(5, P, 31)
    view, gd = _place(rows, 4100, 0), _dev(g)
    ops.dpfa_clip_sum(view, _dev(scale), out, global_=gd, sigma=sg, seed=seed)
    assert dr.same_bits(_np(out), dr.clipped_sum(rows, scale, g, noise=nu.astype(F)))
    # no sigma and no injected noise (z = 0): out = g + acc, the noise add is skipped
    ops.dpfa_clip_sum(view, _dev(scale), out, global_=gd, seed=seed)
    assert dr.same_bits(_np(out), dr.clipped_sum(rows, scale, g))


# ------------------------------------------------------------------ the clip update
def test_clip_update_three_rounds_on_the_device():
    """|ln C_gpu - ln C_ref| <= eta * sigma_b * GAUSS_TOL / m + 1e-12 in every round (xi's fp32
    tolerance through the exponent; fp64 exp / log): the state is carried on the device, and
    each round's reference starts from the clip norm the device held before it."""
    m, gamma, eta, sb = 10, 0.4, 0.2, 0.75
    st = _state(1.75)
    clip = 1.75
    tol = eta * sb * pr.GAUSS_TOL / m + 1e-12
    for rnd, nbits in enumerate((0, 10, 4)):
        key = dr.round_key(9, 3, rnd)
        st[ops.DPFA_BITSUM] = float(nbits)
        ops.dpfa_clip_update(st, m, gamma, eta, sb, seed=key)
        bbar, nxt = dr.clip_update(clip, nbits, m, gamma, eta, sb, key)
        stn = _np(st)
        print("round %d: ln C_gpu - ln C_ref = %.3g (tol %.3g)"
              % (rnd, math.log(stn[ops.DPFA_CLIP]) - math.log(nxt), tol))
        assert abs(math.log(stn[ops.DPFA_CLIP]) - math.log(nxt)) <= tol
        assert stn[ops.DPFA_NEXT] == stn[ops.DPFA_CLIP] and stn[ops.DPFA_PREV] == clip
        assert abs(stn[ops.DPFA_BBAR] - bbar) <= sb * pr.GAUSS_TOL / m + 1e-15
        clip = float(stn[ops.DPFA_CLIP])  # carried by the device
    assert clip != 1.75
    # the all-reduced count from a tensor of its own
    st2 = _state(1.75)
    ops.dpfa_clip_update(st2, m, gamma, eta, sb, seed=dr.round_key(9, 3, 0),
                         bit_sum=torch.zeros(1, dtype=torch.float64, device=DEV))
    want = dr.clip_update(1.75, 0, m, gamma, eta, sb, dr.round_key(9, 3, 0))[1]
    assert abs(math.log(_np(st2)[ops.DPFA_CLIP]) - math.log(want)) <= eta * sb * pr.GAUSS_TOL / m \
        + 1e-12
    # eta = 0: the clip norm keeps its bits
    c0 = 1.0 / 3.0
    st3 = _state(c0)
    st3[ops.DPFA_BITSUM] = 3.0
    ops.dpfa_clip_update(st3, m, gamma, 0.0, 5.0, seed=1)
    assert _np(st3)[ops.DPFA_CLIP] == c0 and _np(st3)[ops.DPFA_BBAR] == 0.3


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    rows = torch.zeros(3, 8, device=DEV)
    g = torch.full((8,), SENTINEL, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    scale = torch.full((3,), 1 / 3, device=DEV)
    st = _state(1.0)
    sq = torch.ones(3, dtype=torch.float64, device=DEV)
    idx = torch.zeros(3, dtype=torch.int32, device=DEV)

    def csum(rows=rows, scale=scale, out=out, **kw):
        kw.setdefault("global_", g)
        ops.dpfa_clip_sum(rows, scale, out, **kw)
    for kw, msg in (({"rows": rows[:0], "scale": scale[:0]}, "num_clients"),
                    ({"scale": None}, "null pointer"),
                    ({"rows": torch.zeros(3, 8)}, "HIP device"),
                    ({"out": torch.zeros(8)}, "HIP device"),
                    ({"rows": rows.double()}, "float32"), ({"rows": rows.t()}, "unit column"),
                    ({"rows": rows[0]}, "matrix"),
                    ({"P": 9}, "P=9"), ({"out": out[:7]}, "at least 8"),
                    ({"global_": g[:7]}, "at least 8"), ({"scale": scale[:2]}, "at least 3"),
                    ({"noise": out[:7]}, "at least 8"), ({"sigma": out[:0]}, "at least 1"),
                    ({"out": out.double()}, "float32"),
                    ({"row_index": idx.long()}, "int32"),
                    ({"out": torch.zeros(8, 2, device=DEV)[:, 0]}, "contiguous")):
        with pytest.raises(FedHipError, match=msg):
            csum(**kw)
    # the C ABI's own checks, past the wrapper
    from fedhip._lib import call, ptr, stream_handle
    for args, msg in (((ptr(rows), 8, None, ptr(scale), 3, -1, ptr(g), ptr(out), None, None, 0, 0,
                        0), "bad sizes"),
                      ((ptr(rows), -8, None, ptr(scale), 3, 8, ptr(g), ptr(out), None, None, 0, 0,
                        0), "bad sizes"),
                      ((ptr(rows), 8, None, ptr(scale), 3, 8, ptr(g), ptr(out), None, None, 0, 0,
                        4), "unknown flags"),
                      ((ptr(rows), 8, None, ptr(scale), 3, 8, None, ptr(out), None, None, 0, 0,
                        0), "rows are deltas"),
                      ((None, 8, None, ptr(scale), 3, 8, ptr(g), ptr(out), None, None, 0, 0, 0),
                       "null pointer"),
                      ((ptr(rows), 8, None, ptr(scale), 3, 8, ptr(g), None, None, None, 0, 0, 0),
                       "null pointer")):
        with pytest.raises(FedHipError, match=msg):
            call("fh_dpfa_clip_sum", *args, stream_handle())
    csum(P=0)
    for args, msg in (((ptr(rows), 8, None, None, 0, 8, None, 0, ptr(sq)), "num_clients"),
                      ((ptr(rows), 8, None, None, 3, -1, None, 0, ptr(sq)), "bad sizes"),
                      ((ptr(rows), 8, None, None, 3, 8, None, 0, None), "null pointer"),
                      ((None, 8, None, None, 3, 8, None, 0, ptr(sq)), "null pointer"),
                      ((ptr(rows), 8, None, None, 3, 8, None, 0, ptr(sq)), "workspace"),
                      ((ptr(rows), 8, None, None, 3, 8, ptr(out), 8, ptr(sq)), "workspace")):
        with pytest.raises(FedHipError, match=msg):
            call("fh_dpfa_row_sqnorm", *args, stream_handle())
    for kw, msg in (({"rows": torch.zeros(3, 8)}, "HIP device"), ({"P": 9}, "P=9"),
                    ({"global_": g.double()}, "float32"), ({"out": sq[:2]}, "at least 3"),
                    ({"out": sq.float()}, "float64")):
        a = dict(rows=rows, global_=g)
        a.update(kw)
        with pytest.raises(FedHipError, match=msg):
            ops.dpfa_row_sqnorm(a.pop("rows"), a.pop("global_"), **a)
    for a, msg in (((sq[:0], st, 3, 1.0), "num_clients"), ((sq, st, 2, 1.0), "total_clients"),
                   ((sq, st, 3, -1.0), "noise multiplier"),
                   ((sq, st, 3, float("nan")), "noise multiplier"),
                   ((sq, st[:5], 3, 1.0), "at least 8"), ((sq.float(), st, 3, 1.0), "float64"),
                   ((sq, st.cpu(), 3, 1.0), "HIP device")):
        with pytest.raises(FedHipError, match=msg):
            ops.dpfa_clip_coef(*a)
    with pytest.raises(FedHipError, match="null pointer"):
        call("fh_dpfa_clip_coef", ptr(sq), 3, 3, 1.0, None, ptr(scale), ptr(idx), None,
             stream_handle())
    for a, msg in (((st, 0, 0.5, 0.2, 1.0), "total_clients"), ((st, 3, 1.5, 0.2, 1.0), "quantile"),
                   ((st, 3, -0.1, 0.2, 1.0), "quantile"), ((st, 3, 0.5, -0.2, 1.0), "clip_lr"),
                   ((st, 3, 0.5, float("inf"), 1.0), "clip_lr"),
                   ((st, 3, 0.5, 0.2, -1.0), "bit_noise"), ((st[:5], 3, 0.5, 0.2, 1.0), "at least 8")):
        with pytest.raises(FedHipError, match=msg):
            ops.dpfa_clip_update(*a)
    with pytest.raises(FedHipError, match="null pointer"):
        call("fh_dpfa_clip_update", None, ptr(sq), 3, 0.5, 0.2, 1.0, 0, stream_handle())
    torch.cuda.synchronize()
    assert (_np(out) == SENTINEL).all() and (_np(g) == SENTINEL).all()  # nothing was launched
    assert _np(st)[ops.DPFA_CLIP] == 1.0 and not _np(st)[1:].any()


def test_python_refusals():
    from fedhip.round import DPConfig, RankRound
    from src.shared import models_pytorch as hm
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    cfg = dpfedavg.CentralDPConfig(Z, 1.0, bit_noise=1.0)

    def make(**kw):
        return RankRound(model, SIZES, list(range(4)), epochs=1, device=DEV, lanes=1, **kw)
    with pytest.raises(FedHipError, match="joint accounting"):
        make(central_dp=cfg, dp=DPConfig(epsilon=1.0))
    with pytest.raises(FedHipError, match="robust aggregator"):
        make(central_dp=cfg, aggregator=robust.MedianAggregator())
    with pytest.raises(FedHipError, match="robust aggregator"):
        make(central_dp=cfg,
             server_opt=fedopt.FedYogi(0.05, base=robust.MedianAggregator(), device=DEV))
    with pytest.raises(ValueError, match="bit_noise"):
        dpfedavg.CentralDPConfig(Z, 1.0, bit_noise=0.5 * Z)
    # bit_noise None is m / 20: 2 * 4 / 20 <= z is only known once m is
    with pytest.raises(FedHipError, match="bit_noise"):
        make(central_dp=dpfedavg.CentralDPConfig(Z, 1.0))
    with pytest.raises(ValueError, match="CentralDPConfig"):
        dpfedavg.DPFedAvg({"noise_multiplier": 1.0}, DEV)


# ------------------------------------------------------------------ DPFedAvg
SHAPES = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}


def _flat(weights):
    return np.concatenate([_np(weights[n]).reshape(-1) for n in SHAPES])


def _check_round(agg, rows, g, clip, m, key, cfg, noise, got_out, got_clip):
    """One fused round of `agg` (a DPFedAvg after the round) against the reference at the clip
    norm `clip` the device held before the round (the configured one, or the one the previous
    round's check accepted): the scales within 1 ulp, the bits equal, the sum bit for bit from
    the GPU's own scales, the next clip norm within the derived tolerance."""
    zd, sb = cfg.resolve(m)
    ref_sq = dr.sqnorms(rows, g)
    assert _not_near(np.sqrt(ref_sq), clip)
    bits_ref, s_ref = dr.clip_coef(ref_sq, clip, m)
    scale = _np(agg.last["scale"])
    assert _np(agg.last["bits"]).tolist() == bits_ref.tolist()
    assert (_ulps(scale, s_ref) <= 1).all()
    assert np.allclose(_np(agg.last["norms"]), np.sqrt(ref_sq), rtol=1e-12, atol=0)
    assert dr.same_bits(got_out, dr.clipped_sum(rows, scale, g, noise=noise))
    _, nxt = dr.clip_update(clip, int(bits_ref.sum()), m, cfg.target_quantile, cfg.clip_lr, sb,
                            key)
    tol = cfg.clip_lr * sb * pr.GAUSS_TOL / m + 1e-12
    print("ln C_gpu - ln C_ref = %.3g (tol %.3g)" % (math.log(got_clip) - math.log(nxt), tol))
    assert abs(math.log(got_clip) - math.log(nxt)) <= tol
    assert agg.last["bits"].numel() == len(rows)


def test_step_rows_three_rounds_and_state_round_trip():
    tall, P, stride, m = 7, 1001, 1008, 4
    pick = [5, 0, 3, 6]
    rng = np.random.default_rng(21)
    g = rng.standard_normal(P).astype(F)
    cfg = dpfedavg.CentralDPConfig(Z, 1.0, target_quantile=0.5, clip_lr=0.3, bit_noise=1.0)
    agg = dpfedavg.DPFedAvg(cfg, DEV, dp_seed=5)
    gd = _dev(g)
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    clip, clone = None, None
    for rnd in range(3):
        rows = (g + 10.0 ** rng.uniform(-1.5, 0, (tall, 1)) * 0.1
                * rng.standard_normal((tall, P))).astype(F)
        if rnd == 0:  # the initial clip norm: between the picked rows' norms
            clip = _clip_between(np.sqrt(dr.sqnorms(rows[pick], g)))
            agg.state[ops.DPFA_CLIP] = clip
            assert agg.clip_norm == clip
        noise = (0.01 * rng.standard_normal(P)).astype(F)
        key = dr.round_key(5, 0, rnd)
        opt = agg if rnd < 2 else clone  # the third round runs on the restored copy
        assert opt.step_rows(_place(rows, stride, 0), gd, idx, m, key, noise=_dev(noise)) is gd
        _check_round(opt, rows[pick], g, clip, m, key, cfg, noise, _np(gd), opt.clip_norm)
        assert opt.clip_norm != clip
        g, clip = _np(gd).copy(), opt.clip_norm  # the device carries its own clip norm on
        if rnd == 1:
            clone = dpfedavg.DPFedAvg(dpfedavg.CentralDPConfig(0.0, 9.0, clip_lr=0.0), DEV)
            clone.load_state_dict(agg.state_dict())
            assert clone.config == agg.config and clone.state is not agg.state
            assert clone.clip_norm == agg.clip_norm and clone.rounds == 2
    for bad in ({}, dict(agg.state_dict(), state=agg.state[:5]),
                dict(agg.state_dict(), clip_norm=-1.0),
                dict(agg.state_dict(), state=torch.zeros_like(agg.state))):
        with pytest.raises(FedAvgError):
            clone.load_state_dict(bad)
    with pytest.raises(FedAvgError, match="client rows"):
        agg.step_rows(_place(rows, stride, 0), gd, idx, 3, 0)
    # a fixed clip norm (clip_lr = 0) with the device's own noise: the clip norm keeps its
    # bits, sigma is fl32(z * C / m), and out - (g + acc) is the Philox stream within tolerance
    fixed = dpfedavg.DPFedAvg(dpfedavg.CentralDPConfig(Z, clip, clip_lr=0.0), DEV, dp_seed=5)
    out = torch.empty(P, device=DEV)
    fixed.step_rows(_place(rows, stride, 0), gd, idx, m, 99, out=out)
    assert fixed.clip_norm == clip and dr.same_bits(_np(gd), g)
    sg = _np(fixed.sigma)[0]
    assert _ulps([sg], [dr.sigma_avg(Z, clip, m)])[0] <= 1
    acc = dr.clipped_sum(rows[pick], _np(fixed.last["scale"]), g, add_global=False)
    G = dr.gauss(99, P)
    lo = dr.clipped_sum(acc[None], np.ones(1, dtype=F), g, rows_are_deltas=True,
                        noise=(float(sg) * G).astype(F))
    # three roundings away from the real sum g + acc + sigma G: the product, two adds
    bound = float(sg) * (pr.GAUSS_TOL + 2.0 ** -24 * np.abs(G)) \
        + 2.0 ** -23 * (np.abs(acc) + np.abs(lo) + float(sg) * np.abs(G))
    assert (np.abs(_np(out).astype(np.float64) - lo.astype(np.float64)) <= bound).all()


def test_aggregate_updates_round_trip():
    gen = torch.Generator().manual_seed(4)
    prev_w = {name: 0.3 * torch.randn(*shape, generator=gen) for name, shape in SHAPES.items()}
    prev = GlobalModel(round_number=3, model_weights=prev_w, accuracy_metrics={},
                       participating_clients=[], convergence_score=0.0)
    ups = []
    for k in range(3):
        wts = {name: t + 0.05 * (k + 1) * torch.randn(*t.shape, generator=gen)
               for name, t in prev_w.items()}
        ups.append(ModelUpdate(client_id=f"c{k}", round_number=4, model_weights=wts,
                               num_samples=10 + k, training_loss=0.5, privacy_budget_used=0.5,
                               compression_ratio=0.8, timestamp=datetime.now()))
    rows = np.stack([_flat(u.model_weights) for u in ups])
    g0 = _flat(prev_w)
    clip = _clip_between(np.sqrt(dr.sqnorms(rows, g0)))
    cfg = dpfedavg.CentralDPConfig(0.0, clip, clip_lr=0.2, bit_noise=0.0)  # z = 0: no noise
    agg = dpfedavg.DPFedAvg(cfg, DEV, dp_seed=8)
    gm = agg.aggregate_updates(ups, 4, prev)
    assert gm.round_number == 4 and gm.participating_clients == ["c0", "c1", "c2"]
    assert [gm.model_weights[n].shape for n in SHAPES] == [torch.Size(s) for s in SHAPES.values()]
    _check_round(agg, rows, g0, clip, 3, dr.round_key(8, 0, 4), cfg, None,
                 _flat(gm.model_weights), agg.clip_norm)
    assert dr.same_bits(_flat(prev_w), g0)  # the previous model is not stepped in place
    with pytest.raises(FedAvgError):
        agg.aggregate_updates([], 5, prev)
    bad_prev = GlobalModel(5, {"fc.bias": prev_w["fc.bias"]}, {}, [], 0.0)
    with pytest.raises(FedAvgError, match="previous model"):
        agg.aggregate_updates(ups, 5, bad_prev)


# ------------------------------------------------------------------ RankRound
SIZES = [70, 55, 48, 40]
DP_SEED = 5
_CACHE = {}


def _client_data(k, n, shape=(1, 28, 28)):
    g = torch.Generator().manual_seed(200 + k)
    return torch.randn(n, *shape, generator=g), torch.randint(0, 10, (n,), generator=g)


def _central_noise(P, rnd):
    return (0.002 * np.random.default_rng(900 + rnd).standard_normal(P)).astype(F)


def _rounds(mine, nrounds=1, model="simple_cnn", sizes=SIZES, dp_seed=DP_SEED, inject=True,
            **kw):
    """`nrounds` rounds of SimpleCNN over SIZES' clients `mine` on one RankRound.  Returns the
    RankRound, the global vector before round one, and per round (the trained rows by client,
    copied by the on_trained hook; the global vector; global_bufs; partial; the clip norm
    after the round; the last scales and bits)."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    shape = (1, 28, 28) if model == "simple_cnn" else (3, 32, 32)
    model = hm.ModelFactory.create_model(model).to(DEV)
    r = RankRound(model, sizes, mine, epochs=1, device=DEV, lanes=1, shuffle_seed=77,
                  dp_seed=dp_seed, **kw)
    xs, ys = zip(*[_client_data(k, sizes[k], shape) for k in r.slots])
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [sizes[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    start = _np(r.global_flat).copy()
    out = []
    for i in range(nrounds):
        if r.central is not None and inject:
            r.central_noise = _dev(_central_noise(r.P, i))
        r.run(data, labels, offs, "sgd", 0.01, seed=3 + i)
        torch.cuda.synchronize()
        c = r.central
        out.append((dict(seen), _np(r.global_flat).copy(), _np(r.global_bufs).copy(),
                    _np(r.partial).copy(), None if c is None else c.clip_norm,
                    None if c is None else _np(c.last["scale"]).copy(),
                    None if c is None else _np(c.last["bits"]).copy()))
    return r, start, out


def _plain():
    """The plain one-rank round (no central DP), once: its rows say which clip norm splits
    the clients."""
    if "plain" not in _CACHE:
        r, start, rounds = _rounds(list(range(4)))
        stack = np.stack([rounds[0][0][k] for k in range(4)])
        clip = _clip_between(np.sqrt(dr.sqnorms(stack, start)))
        _CACHE["plain"] = (start, rounds, clip, _np(r.w32).copy())
    return _CACHE["plain"]


def _config(clip, **kw):
    return dpfedavg.CentralDPConfig(Z, clip, target_quantile=0.5, clip_lr=0.3, bit_noise=1.0, **kw)


def test_rankround_one_rank_two_rounds():
    all4 = list(range(4))
    start, plain, clip, w = _plain()
    cfg = _config(clip)
    r, g, rounds = _rounds(all4, 2, central_dp=cfg)
    assert dr.same_bits(g, start) and r.clients == all4
    m = len(SIZES)
    for i, (rows, glob, bufs, _, clip_after, scale, bits) in enumerate(rounds):
        # round 2 runs at the clip norm round 1 left on the device (checked below)
        clip = cfg.clip_norm if i == 0 else rounds[i - 1][4]
        stack = np.stack([rows[k] for k in all4])
        if i == 0:  # same seeds: the rows the plain round trained
            assert all(dr.same_bits(rows[k], plain[0][0][k]) for k in all4)
        ref_sq = dr.sqnorms(stack, g)
        assert _not_near(np.sqrt(ref_sq), clip)
        bits_ref, s_ref = dr.clip_coef(ref_sq, clip, m)
        assert bits.tolist() == bits_ref.tolist() and (_ulps(scale, s_ref) <= 1).all()
        assert dr.same_bits(glob, dr.clipped_sum(stack, scale, g, noise=_central_noise(r.P, i))), \
            f"round {i + 1}"
        key = dr.round_key(DP_SEED, 3 + i, i)
        _, nxt = dr.clip_update(clip, int(bits_ref.sum()), m, 0.5, 0.3, 1.0, key)
        tol = 0.3 * 1.0 * pr.GAUSS_TOL / m + 1e-12
        print("round %d: ln C_gpu - ln C_ref = %.3g (tol %.3g)"
              % (i + 1, math.log(clip_after) - math.log(nxt), tol))
        assert abs(math.log(clip_after) - math.log(nxt)) <= tol
        g = glob
    assert 0 < rounds[0][6].sum() < m  # some clipped, some not: the clip norm was well chosen
    assert rounds[0][4] != cfg.clip_norm  # and round 2 ran at the updated norm
    # central_dp=None is today's path: same bits as without the argument; the BN running
    # statistics are the plain FedAvg's (release_buffers=True)
    _, _, none = _rounds(all4, central_dp=None)
    assert dr.same_bits(plain[0][1], none[0][1]) and dr.same_bits(plain[0][2], none[0][2])
    assert not dr.same_bits(plain[0][1], rounds[0][1])
    assert dr.same_bits(plain[0][2], rounds[0][2])
    stack = np.stack([plain[0][0][k] for k in all4])
    assert dr.same_bits(plain[0][1], fr.weighted_sum(stack, w))


def test_rankround_release_buffers():
    """SimpleCNN has no BatchNorm: the running statistics are CIFAR10CNN's.  release_buffers
    True: global_bufs is the plain round's FedAvg of them; False: it is left as it was."""
    sizes, both = [40, 33], [0, 1]
    kw = dict(model="cifar10_cnn", sizes=sizes)
    r0, start, plain = _rounds(both, 1, **kw)
    assert r0.Q > 0
    stack = np.stack([plain[0][0][k] for k in both])
    clip = _clip_between(np.sqrt(dr.sqnorms(stack, start)))
    cfg = dpfedavg.CentralDPConfig(Z, clip, clip_lr=0.0)
    untouched = _np(_rounds(both, 0, **kw)[0].global_bufs)
    assert not dr.same_bits(plain[0][2], untouched)
    _, _, on = _rounds(both, 1, central_dp=cfg, **kw)
    assert dr.same_bits(on[0][2], plain[0][2])
    assert dr.same_bits(on[0][1], dr.clipped_sum(stack, on[0][5], start,
                                                 noise=_central_noise(r0.P, 0)))
    cfg = dpfedavg.CentralDPConfig(Z, clip, clip_lr=0.0, release_buffers=False)
    _, _, off = _rounds(both, 1, central_dp=cfg, **kw)
    assert dr.same_bits(off[0][2], untouched)
    assert dr.same_bits(off[0][1], on[0][1])


def test_rankround_fedadam_steps_toward_the_noisy_aggregate():
    all4 = list(range(4))
    start, plain, clip, _ = _plain()
    r, g, rounds = _rounds(all4, 1, central_dp=_config(clip))
    noise = _central_noise(r.P, 0)
    stack = np.stack([rounds[0][0][k] for k in all4])
    noisy = dr.clipped_sum(stack, rounds[0][5], g, noise=noise)
    assert dr.same_bits(rounds[0][1], noisy)
    # server_opt=FedAdam steps toward the noisy aggregate, which lands in `partial`
    so = fedopt.FedAdam(0.01, device=DEV)
    r, g, rounds = _rounds(all4, 1, central_dp=_config(clip), server_opt=so)
    assert dr.same_bits(rounds[0][3], noisy)
    tau32 = F(so.tau)
    want = fr.server_opt_step(fr.ADAM, noisy[None], None, g, np.zeros(r.P, dtype=F),
                              np.full(r.P, tau32 * tau32, dtype=F), server_lr=so.server_lr,
                              beta1=so.beta1, beta2=so.beta2, tau=so.tau)
    assert dr.same_bits(rounds[0][1], want[0]) and dr.same_bits(_np(so.m), want[1])


def _rank_main(rank, world, port, clip, exact, q, own_draws=False):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        extra = dict(dp_seed=None, inject=False) if own_draws else {}
        r, start, rounds = _rounds(mine, 1, central_dp=_config(clip), exact=exact, **extra)
        res = (start, rounds[0], _np(r.central.state).copy(), list(r.clients))
        q.put((rank, res + (r.dp_seed,) if own_draws else res))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def _two_ranks(clip, exact, port, own_draws=False):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, clip, exact, q, own_draws))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert not isinstance(res[r], str), f"rank {r} failed: {res[r]}"
    assert all(p.exitcode == 0 for p in procs)
    return res[0], res[1]


def test_rankround_two_ranks_all_reduce():
    """Two gloo ranks on cuda:0: each rank's clipped partial sum and bit count are all-reduced
    and both ranks finish alike.  Both end with bit-identical global vectors and clip state,
    equal to the reference finish applied to the all-reduced partial and bit sum."""
    _, _, clip, _ = _plain()
    (s0, rd0, st0, c0), (s1, rd1, st1, c1) = _two_ranks(clip, False,
                                                        29860 + os.getpid() % 100)
    assert sorted(c0 + c1) == list(range(len(SIZES)))
    assert dr.same_bits(s0, s1)
    assert dr.same_bits(rd0[1], rd1[1]), "ranks disagree on the global model"
    assert np.array_equal(st0.view(np.uint64), st1.view(np.uint64)), "... on the clip state"
    assert dr.same_bits(rd0[3], rd1[3])
    m = len(SIZES)
    parts, nbits = [], 0
    for (rows, _, _, _, _, scale, bits), c in ((rd0, c0), (rd1, c1)):
        stack = np.stack([rows[k] for k in c])
        ref_sq = dr.sqnorms(stack, s0)
        assert _not_near(np.sqrt(ref_sq), clip)
        bits_ref, s_ref = dr.clip_coef(ref_sq, clip, m)
        assert bits.tolist() == bits_ref.tolist() and (_ulps(scale, s_ref) <= 1).all()
        parts.append(dr.clipped_sum(stack, scale, s0, add_global=False))
        nbits += int(bits_ref.sum())
    total = parts[0] + parts[1]
    assert dr.same_bits(rd0[3], total)  # `partial` holds the all-reduced sum
    P = s0.size
    want = dr.clipped_sum(total[None], np.ones(1, dtype=F), s0, noise=_central_noise(P, 0),
                          rows_are_deltas=True)
    assert dr.same_bits(rd0[1], want)
    assert st0[ops.DPFA_BITSUM] == nbits and st0[ops.DPFA_PREV] == clip
    _, nxt = dr.clip_update(clip, nbits, m, 0.5, 0.3, 1.0, dr.round_key(DP_SEED, 3, 0))
    assert abs(math.log(rd0[4]) - math.log(nxt)) <= 0.3 * 1.0 * pr.GAUSS_TOL / m + 1e-12


def test_rankround_two_ranks_exact_equals_the_one_rank_path():
    """exact=True: the fused path over the all-gathered rows in global client order.  Both
    ranks hold the same bits, and they are the bits the one-rank fused path gives on the same
    rows (run here on one device) and the reference gives from the GPU's scales."""
    _, _, clip, _ = _plain()
    (s0, rd0, st0, c0), (s1, rd1, st1, c1) = _two_ranks(clip, True, 29660 + os.getpid() % 100)
    assert dr.same_bits(rd0[1], rd1[1]) and np.array_equal(st0.view(np.uint64), st1.view(np.uint64))
    assert dr.same_bits(rd0[5], rd1[5]) and rd0[5].size == len(SIZES)
    rows = {**rd0[0], **rd1[0]}
    stack = np.stack([rows[k] for k in range(len(SIZES))])
    P, m = s0.size, len(SIZES)
    noise = _central_noise(P, 0)
    assert dr.same_bits(rd0[1], dr.clipped_sum(stack, rd0[5], s0, noise=noise))
    one = dpfedavg.DPFedAvg(_config(clip), DEV, dp_seed=DP_SEED)
    gd = _dev(s0)
    one.step_rows(_dev(stack), gd, None, m, dr.round_key(DP_SEED, 3, 0), noise=_dev(noise))
    assert dr.same_bits(rd0[1], _np(gd))
    assert np.array_equal(st0.view(np.uint64), _np(one.state).view(np.uint64))


@pytest.mark.parametrize("exact", [False, True])
def test_rankround_two_ranks_default_seed_and_own_draws_agree(exact):
    """No dp_seed given and no noise injected, z > 0: every rank draws its own secret, the ranks
    adopt rank 0's at construction, and the one Philox draw of the aggregate and xi are the
    same on both.  Bit-identical global vectors and clip state; the noise is really there."""
    _, _, clip, _ = _plain()
    (s0, rd0, st0, c0, seed0), (s1, rd1, st1, c1, seed1) = _two_ranks(
        clip, exact, 29560 + 50 * int(exact) + os.getpid() % 50, own_draws=True)
    assert seed0 == seed1 and seed0 != DP_SEED
    assert dr.same_bits(rd0[1], rd1[1]), "ranks disagree on the global model"
    assert np.array_equal(st0.view(np.uint64), st1.view(np.uint64)), "... on the clip state"
    m, P = len(SIZES), s0.size
    rows = {**rd0[0], **rd1[0]}
    if exact:
        stack = np.stack([rows[k] for k in range(m)])
        acc = dr.clipped_sum(stack, rd0[5], s0, add_global=False)
    else:
        acc = rd0[3]  # `partial`: the all-reduced clipped sum
    quiet = dr.clipped_sum(acc[None], np.ones(1, dtype=F), s0, rows_are_deltas=True)
    assert not dr.same_bits(rd0[1], quiet)
    # and it is the server stream under the agreed key, within the Box-Muller tolerance
    sg = F(st0[ops.DPFA_SIGMA])
    assert _ulps([sg], [dr.sigma_avg(dr.z_delta(Z, 0.3, 1.0), clip, m)])[0] <= 1
    G = dr.gauss(dr.round_key(seed0, 3, 0), P)
    lo = dr.clipped_sum(acc[None], np.ones(1, dtype=F), s0, rows_are_deltas=True,
                        noise=(float(sg) * G).astype(F))
    bound = float(sg) * (pr.GAUSS_TOL + 2.0 ** -24 * np.abs(G)) \
        + 2.0 ** -23 * (np.abs(acc) + np.abs(lo) + float(sg) * np.abs(G))
    assert (np.abs(rd0[1].astype(np.float64) - lo.astype(np.float64)) <= bound).all()
