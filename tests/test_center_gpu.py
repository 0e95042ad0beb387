"""The geometric-median / centered-clipping kernels (csrc/center.hip) and the two rules built on
them, on the GPU, against the numpy reference of tests/center_ref.py (pinned by
test_center_ref_cpu.py).

fh_center_iter's `out` is held to the reference bit for bit (uint32 views) over client counts on
both sides of every register-slot count, sizes below / across the vector width and the 256-thread
tile, both modes, normal, small-integer and special-value data, coefficients with exact zeros on
NaN / Inf rows, through the vector path and the scalar path (odd stride, misaligned rows,
misaligned out / centre).  Its `sqdist` must be exact where every sum is exact (small integers)
and within the fp64 summation-order bound  P * 2^-53 * sum  otherwise.  fh_center_coef is held
bit for bit, state included.  The rules are compared with the reference replaying the device's
own distances, so the fp32 side is bit for bit although fp64 sums differ in their last bit.
"""
import numpy as np
import pytest
import torch

import center_ref as cr
import fedopt_ref as fr
from fedhip import ops
from fedhip._lib import FedHipError, call, ptr, stream_handle
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
F = np.float32

CS = [1, 2, 3, 5, 16, 17, 33, 64]
PS = [1, 3, 13, 1001, 4099]
MODES = [cr.MEAN, cr.DELTA]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000,
                     0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA5A5A5, 0x7FFFFFFF],
                    dtype=np.uint32).view(np.float32)


def _case(kind, C, P, seed):
    """(rows, coef, center, poisoned rows).  Up to two rows (never all) are NaN / Inf rows with
    coefficient +0 / -0; `special` also scatters special values over the other rows."""
    rng = np.random.default_rng(seed)
    if kind == "smallint":
        rows = rng.integers(-8, 9, size=(C, P)).astype(F)
        coef = rng.integers(-2, 3, size=C).astype(F)  # integer coefficients, zeros among them
        center = rng.integers(-8, 9, size=P).astype(F)
    else:
        rows = rng.standard_normal((C, P)).astype(F)
        coef = (rng.standard_normal(C) / C).astype(F)
        center = rng.standard_normal(P).astype(F)
        if C > 3:
            coef[rng.integers(C)] = 0.0  # an ordinary row that is skipped
    poisoned = []
    if kind == "special":
        for j in range(0, P, 3):
            rows[rng.integers(C), j] = SPECIALS[(j // 3) % len(SPECIALS)]
        center[::7] = SPECIALS[np.arange(len(center[::7])) % 5]  # zeros and denormals
    if C >= 3:
        poisoned = sorted(rng.permutation(C)[:2].tolist())
        rows[poisoned[0], rng.integers(P)] = np.nan
        rows[poisoned[1], :] = np.inf if P % 2 else -np.inf
        coef[poisoned[0]], coef[poisoned[1]] = 0.0, -0.0
    return rows, coef, center, poisoned


def _window(P, offset, fill=None):
    """P floats inside a sentinel-filled buffer, `offset` floats from its 16-B base."""
    buf = torch.full((P + 16,), SENTINEL, device=DEV)
    view = buf[offset:offset + P]
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return buf, view


def _sentinels_intact(buf, offset, P):
    b = buf.cpu().numpy()
    return (b[:offset] == SENTINEL).all() and (b[offset + P:] == SENTINEL).all()


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show)."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


def _iter(view, coef, mode, center=None, out_offset=4, center_offset=0, row_index=None,
          alias=False):
    """One fh_center_iter into a sentinel window; alias: out IS the centre buffer (DELTA)."""
    P = view.shape[1]
    c32 = torch.from_numpy(np.ascontiguousarray(coef, dtype=F)).to(DEV)
    cdev = None
    if alias:
        buf, out = _window(P, out_offset, fill=center)
        cdev = out
    else:
        buf, out = _window(P, out_offset)
        if mode == cr.DELTA:
            _, cdev = _window(P, center_offset, fill=center)
    got, sq = ops.center_iter(view, c32, out, mode, center=cdev, row_index=row_index)
    torch.cuda.synchronize()
    assert got is out and _sentinels_intact(buf, out_offset, P)
    return out.cpu().numpy(), sq.cpu().numpy()


def _sq_ok(got, want, P, exact):
    """Same NaN / Inf pattern; finite entries exact, or within the summation-order bound."""
    if not (np.array_equal(np.isnan(got), np.isnan(want))
            and np.array_equal(np.isinf(got), np.isinf(want))):
        return False
    fin = np.isfinite(want)
    if exact:
        return np.array_equal(got[fin], want[fin])
    return bool(np.all(np.abs(got[fin] - want[fin]) <= P * 2.0 ** -53 * want[fin]))


# The smallest shape with two tiles per workgroup: the 64-slot scalar instance (at most 512
# workgroups, one column per thread) over 512 * 256 + 257 columns is 514 tiles on 257 workgroups,
# the last tile partial.
P_TWO_TILES = 512 * 256 + 257


@pytest.mark.parametrize("C", CS)
def test_center_iter_bits(C):
    for ki, kind in enumerate(("normal", "smallint", "special")):
        for P in PS + [P_TWO_TILES] * (C == 64 and kind == "normal"):
            rows, coef, center, poisoned = _case(kind, C, P, 1000 * C + 10 * ki + P)
            vec = _place(rows, (P + 3) // 4 * 4 + 4, 0)   # 16-B columns + scalar tail
            sca = _place(rows, P | 1, 0)                  # odd stride: scalar path
            for mode in MODES:
                want, want_sq = cr.center_iter(mode, rows, coef, center=center)
                for view in (vec, sca)[P == P_TWO_TILES:]:
                    got, sq = _iter(view, coef, mode, center=center)
                    tag = (kind, P, mode, view.stride(0))
                    assert cr.same_bits(got, want), tag
                    assert _sq_ok(sq, want_sq, P, exact=kind == "smallint"), (tag, sq, want_sq)
                    if kind == "normal":  # non-finite exactly for the non-finite rows
                        bad = np.zeros(C, dtype=bool)
                        bad[poisoned] = True
                        assert np.array_equal(~np.isfinite(sq), bad), tag


@pytest.mark.parametrize("C", [3, 17, 33, 64])
def test_center_iter_row_index_misalignment_aliasing_and_replay(C):
    P, tall = 1001, C + 5
    rng = np.random.default_rng(C)
    rows, _, center, _ = _case("special", tall, P, 77 + C)
    pick = rng.permutation(tall)[:C]           # a subset of a taller matrix, permuted
    coef = (rng.standard_normal(C) / C).astype(F)
    for k in range(C):
        if not np.isfinite(rows[pick[k]]).all() and k % 2:
            coef[k] = 0.0
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    aligned = _place(rows, 1008, 0)
    for mode in MODES:
        want, want_sq = cr.center_iter(mode, rows[pick], coef, center=center)
        a, sq = _iter(aligned, coef, mode, center=center, row_index=idx)
        assert cr.same_bits(a, want) and _sq_ok(sq, want_sq, P, exact=False)
        # the same call again: the same bits, distances included
        a2, sq2 = _iter(aligned, coef, mode, center=center, row_index=idx)
        assert cr.same_bits(a2, a) and np.array_equal(sq2.view(np.uint64), sq.view(np.uint64))
        for view, kw in ((_place(rows, 1008, 1), {}),              # rows + 4 B
                         (aligned, {"out_offset": 1}),              # out + 4 B
                         (aligned, {"center_offset": 3}),           # centre + 12 B
                         (_place(rows, 1003, 0), {})):              # odd stride
            got, sq3 = _iter(view, coef, mode, center=center, row_index=idx, **kw)
            assert cr.same_bits(got, want), (mode, kw)
            assert _sq_ok(sq3, want_sq, P, exact=False), (mode, kw)
    # out aliased to the centre in DELTA, on both paths
    for off in (0, 1):
        got, sq = _iter(aligned, coef, cr.DELTA, center=center, row_index=idx, alias=True,
                        out_offset=off)
        assert cr.same_bits(got, want) and _sq_ok(sq, want_sq, P, exact=False)
    # the identity index against no index (the first C rows of the taller matrix)
    ident = torch.arange(C, dtype=torch.int32, device=DEV)
    w0, _ = cr.center_iter(cr.MEAN, rows[:C], coef)
    assert cr.same_bits(_iter(aligned, coef, cr.MEAN)[0], w0)
    assert cr.same_bits(_iter(aligned, coef, cr.MEAN, row_index=ident)[0], w0)


def test_center_iter_many_tiles_and_exact_sums():
    """P = 700,003: several tiles per workgroup on every path, a 3-column tail; small integers
    keep every fp64 sum exact whatever the order."""
    P = 700003
    for C in (5, 33):
        rng = np.random.default_rng(C)
        rows = rng.integers(-8, 9, size=(C, P)).astype(F)
        coef = rng.integers(-2, 3, size=C).astype(F)
        center = rng.integers(-8, 9, size=P).astype(F)
        view = _place(rows, P + 1, 0)
        for mode in MODES:
            want, want_sq = cr.center_iter(mode, rows, coef, center=center)
            got, sq = _iter(view, coef, mode, center=center)
            assert cr.same_bits(got, want) and np.array_equal(sq, want_sq), (C, mode)


def test_center_iter_argument_errors():
    rows = torch.zeros(65, 8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    sq = torch.full((65,), SENTINEL, dtype=torch.float64, device=DEV)
    coef = torch.ones(65, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def raw(C=3, P=8, mode=0, rows_p=ptr(rows), coef_p=ptr(coef), center_p=None,
            out_p=ptr(out), ws_p=ptr(ws), ws_n=1 << 16, sq_p=ptr(sq)):
        call("fh_center_iter", rows_p, 8, None, coef_p, C, P, center_p, mode, out_p, ws_p, ws_n,
             sq_p, stream_handle())

    for kw, msg in ((dict(C=0), "outside"), (dict(C=65), "outside"), (dict(mode=2), "mode"),
                    (dict(mode=-1), "mode"), (dict(P=-1), "bad sizes"), (dict(ws_n=8), "workspace"),
                    (dict(ws_p=None), "workspace"), (dict(rows_p=None), "null"),
                    (dict(coef_p=None), "null"), (dict(out_p=None), "null"),
                    (dict(sq_p=None), "null"), (dict(mode=1), "null")):
        with pytest.raises(FedHipError, match=msg):
            raw(**kw)
    with pytest.raises(FedHipError, match="outside"):
        ops.center_iter(rows, coef, out, ops.CENTER_MEAN)
    with pytest.raises(FedHipError, match="center"):
        ops.center_iter(rows[:3], coef[:3], out, ops.CENTER_DELTA)
    with pytest.raises(FedHipError, match="HIP device"):
        ops.center_iter(torch.zeros(3, 8), coef[:3], out, ops.CENTER_MEAN)
    assert ops.load().fh_center_iter_workspace(0, 8) == 0
    assert ops.load().fh_center_iter_workspace(65, 8) == 0
    assert ops.load().fh_center_iter_workspace(3, 0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (sq.cpu().numpy() == SENTINEL).all()
    # P == 0: out untouched, zero distances
    _, z = ops.center_iter(rows[:3], coef[:3], out, ops.CENTER_MEAN, P=0, sqdist=sq[:3])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and z.cpu().numpy().tolist() == [0.0] * 3


# ------------------------------------------------------------------ fh_center_coef
def _coef_inputs(C, seed, param):
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(np.log(param) - 3, np.log(param) + 3, size=C))  # both sides of param
    sq = d * d
    alpha = rng.uniform(0.1, 1.0, size=C)
    alpha /= alpha.sum()
    special = [(0.0, None), (param * param, None), (np.nan, None), (np.inf, None), (None, 0.0),
               (1e-320, None), (1e300, None)]
    for i, (s, a) in enumerate(special[:C]):
        k = (i * 3) % C
        if s is not None:
            sq[k] = s
        if a is not None:
            alpha[k] = a
    return sq, alpha


@pytest.mark.parametrize("C", [1, 2, 17, 64])
def test_center_coef_bits(C):
    for rule in (cr.GEOMED, cr.CCLIP):
        for param in (1e-6, 0.75, 40.0):
            for seed in range(3):
                sq, alpha = _coef_inputs(C, 100 * C + seed, param)
                want, want_st = cr.center_coef(rule, sq, alpha, param)
                coef, st = ops.center_coef(torch.from_numpy(sq).to(DEV),
                                           torch.from_numpy(alpha).to(DEV), rule, param)
                torch.cuda.synchronize()
                tag = (rule, param, seed)
                assert cr.same_bits(coef.cpu().numpy(), want), tag
                assert np.array_equal(st.cpu().numpy().view(np.uint64),
                                      want_st.view(np.uint64)), (tag, st, want_st)
    # everything rejected: zeros and live = 0
    sq = torch.full((C,), float("nan"), dtype=torch.float64, device=DEV)
    a = torch.full((C,), 1.0 / C, dtype=torch.float64, device=DEV)
    coef, st = ops.center_coef(sq, a, cr.GEOMED, 1.0)
    assert coef.cpu().numpy().view(np.uint32).tolist() == [0] * C
    assert st.cpu().numpy()[:3].tolist() == [0.0, 0.0, 0.0]


def test_center_coef_argument_errors():
    sq = torch.ones(65, dtype=torch.float64, device=DEV)
    a = torch.ones(65, dtype=torch.float64, device=DEV)
    coef = torch.full((65,), SENTINEL, device=DEV)
    st = torch.zeros(4, dtype=torch.float64, device=DEV)

    def raw(C=3, rule=0, param=1.0, sq_p=ptr(sq), a_p=ptr(a), c_p=ptr(coef), st_p=ptr(st)):
        call("fh_center_coef", sq_p, a_p, C, rule, param, c_p, st_p, stream_handle())

    for kw, msg in ((dict(C=0), "outside"), (dict(C=65), "outside"), (dict(rule=2), "rule"),
                    (dict(rule=-1), "rule"), (dict(param=0.0), "positive"),
                    (dict(param=-1.0), "positive"), (dict(param=float("nan")), "positive"),
                    (dict(param=float("inf")), "positive"), (dict(sq_p=None), "null"),
                    (dict(a_p=None), "null"), (dict(c_p=None), "null"), (dict(st_p=None), "null")):
        with pytest.raises(FedHipError, match=msg):
            raw(**kw)
    with pytest.raises(FedHipError, match="alpha"):
        ops.center_coef(sq[:3], a[:2], 0, 1.0)
    torch.cuda.synchronize()
    assert (coef.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------ the rules end to end
def _rule_case(C, P, seed, integers=False):
    rng = np.random.default_rng(seed)
    if integers:
        center = rng.integers(-4, 5, size=P).astype(F)
        rows = (center + rng.integers(-4, 5, size=(C, P))).astype(F)
    else:
        center = rng.standard_normal(P).astype(F)
        rows = (center + 0.1 * rng.standard_normal((C, P))).astype(F)
        rows[0] += 3.0  # one client far out
    n = [10 + 7 * k for k in range(C)]
    return rows, center, n


def _check_rule(agg, ref_fn, rows, alpha, center, packed, n, row_index=None, replay=True,
                out=None):
    P = rows.shape[1]
    cdev = None if center is None else torch.from_numpy(center.copy()).to(DEV)
    got = agg.aggregate_packed(packed, n, row_index=row_index, out=out, center=cdev)
    torch.cuda.synchronize()
    assert out is None or got is out
    dev_sq = agg.last_sqdist.cpu().numpy()
    assert dev_sq.shape == (agg.iters + 1, rows.shape[0]) and dev_sq.dtype == np.float64
    want, info = ref_fn(rows, alpha, center=center, replay=list(dev_sq) if replay else None)
    assert cr.same_bits(got.cpu().numpy(), want)
    # the device's distances against the reference's own; without replay the rows and the start
    # centre are small integers, so the first pass is exact (the later centres are not integers)
    for i in range(agg.iters + 1):
        assert _sq_ok(dev_sq[i], info["sqdist"][i], P, exact=not replay and i == 0), i
    assert cr.same_bits(np.array(agg.last_coef, dtype=F), info["last_coef"])
    assert agg.last_rejected == info["rejected"]
    if replay:  # the same distances in, the same objective out
        assert agg.last_objective == info["objective"]
    else:
        assert abs(agg.last_objective - info["objective"]) <= P * 2.0 ** -53 * info["objective"]
    return got


@pytest.mark.parametrize("C", [3, 9, 33])
def test_rules_end_to_end(C):
    for P in (13, 4099):
        for iters in (1, 3):
            rows, center, n = _rule_case(C, P, 10 * C + P + iters)
            packed = _place(rows, (P + 3) // 4 * 4, 0)
            gm = robust.GeometricMedianAggregator(nu=1e-6, iters=iters)
            alpha = cr.sample_weights(n)
            ref = lambda r, a, center, replay: cr.geometric_median(  # noqa: E731
                r, a, nu=1e-6, iters=iters, center=center, replay=replay)
            _check_rule(gm, ref, rows, alpha, center, packed, n)
            _check_rule(gm, ref, rows, alpha, None, packed, n)  # from the median
            cc = robust.CenteredClipAggregator(tau=0.12 * np.sqrt(P), iters=iters)
            ref = lambda r, a, center, replay: cr.centered_clip(  # noqa: E731
                r, a, cc.tau, iters=iters, center=center, replay=replay)
            out = torch.empty(P, device=DEV)
            _check_rule(cc, ref, rows, [1.0 / C] * C, center, packed, n, out=out)
        # small integers, one iteration: every distance is exact, so no replay is needed
        rows, center, n = _rule_case(C, P, 5 * C + P, integers=True)
        packed = _place(rows, P | 1, 0)
        gm = robust.GeometricMedianAggregator(nu=0.5, iters=1, weighting="uniform")
        _check_rule(gm, lambda r, a, center, replay: cr.geometric_median(
            r, a, nu=0.5, iters=1, center=center, replay=replay), rows, [1.0 / C] * C, center,
            packed, n, replay=False)
        cc = robust.CenteredClipAggregator(tau=3.0, iters=1, weighting="samples")
        _check_rule(cc, lambda r, a, center, replay: cr.centered_clip(
            r, a, 3.0, iters=1, center=center, replay=replay), rows, cr.sample_weights(n),
            center, packed, n, replay=False)


def test_rules_row_index_in_place_and_refusals():
    C, P = 5, 1001
    rows, center, n = _rule_case(8, P, 3)
    pick = [6, 1, 7, 0, 3]
    packed = _place(rows, 1008, 0)
    n5 = n[:C]
    cc = robust.CenteredClipAggregator(tau=2.0, iters=2)
    ref = lambda r, a, center, replay: cr.centered_clip(  # noqa: E731
        r, a, 2.0, iters=2, center=center, replay=replay)
    _check_rule(cc, ref, rows[pick], [1.0 / C] * C, center, packed, n5, row_index=pick)
    # in place: out is the centre tensor itself (what RankRound passes without a server_opt)
    g = torch.from_numpy(center.copy()).to(DEV)
    assert cc.aggregate_packed(packed, n5, row_index=pick, out=g, center=g) is g
    want, _ = ref(rows[pick], [1.0 / C] * C, center, list(cc.last_sqdist.cpu().numpy()))
    assert cr.same_bits(g.cpu().numpy(), want)
    gm = robust.GeometricMedianAggregator(iters=2)
    g = torch.from_numpy(center.copy()).to(DEV)
    gm.aggregate_packed(packed, n5, row_index=pick, out=g, center=g)
    want, _ = cr.geometric_median(rows[pick], cr.sample_weights(n5), iters=2, center=center,
                                  replay=list(gm.last_sqdist.cpu().numpy()))
    assert cr.same_bits(g.cpu().numpy(), want)
    with pytest.raises(FedAvgError, match="centre"):
        cc.aggregate_packed(packed, n5, row_index=pick)
    with pytest.raises(FedAvgError, match="No updates"):
        gm.aggregate_packed(packed, [])
    with pytest.raises(FedAvgError, match="rows for"):
        gm.aggregate_packed(packed, n5)
    bad = _place(np.full((3, P), np.nan, dtype=F), 1008, 0)
    with pytest.raises(FedAvgError, match="no live client"):
        gm.aggregate_packed(bad, [1, 1, 1], center=torch.zeros(P, device=DEV))


def test_robustness_condition():
    """C = 9, P = 1001, honest rows N(0, 1), three rows at 1e4 on every coordinate (one of them
    with a NaN): both rules end inside the honest cloud, which plain FedAvg does not
    (tests/test_center_ref_cpu.py shows the same for the reference)."""
    rows = np.random.default_rng(7).standard_normal((9, 1001)).astype(F)
    bad = [1, 4, 6]
    rows[bad] = 1e4
    rows[4, 17] = np.nan
    honest = np.delete(rows, bad, axis=0).astype(np.float64)
    mean = honest.mean(axis=0)
    radius = max(np.linalg.norm(x - mean) for x in honest)
    packed = _place(rows, 1004, 0)
    gm = robust.GeometricMedianAggregator()
    out = gm.aggregate_packed(packed, [1] * 9).cpu().numpy()
    assert np.linalg.norm(out - mean) < radius and 4 in gm.last_rejected
    tau = float(np.median(np.linalg.norm(honest, axis=1)))
    cc = robust.CenteredClipAggregator(tau=tau)
    out = cc.aggregate_packed(packed, [1] * 9, center=torch.zeros(1001, device=DEV)).cpu().numpy()
    assert np.linalg.norm(out - mean) < radius and 4 in cc.last_rejected
    w = torch.full((8,), 1.0 / 8, device=DEV)
    idx = torch.tensor([k for k in range(9) if k != 4], dtype=torch.int32, device=DEV)
    fa = ops.fedavg_weighted_sum(packed, w, torch.empty(1001, device=DEV), row_index=idx)
    assert np.linalg.norm(fa.cpu().numpy() - mean) > radius


# ------------------------------------------------------------------ aggregate_updates
def test_aggregate_updates_entry_points():
    from datetime import datetime

    from src.shared.models import GlobalModel, ModelUpdate
    shapes = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}
    g = torch.Generator().manual_seed(5)
    prev = {k: 0.3 * torch.randn(*s, generator=g) for k, s in shapes.items()}
    ups = [ModelUpdate(client_id=f"c{k}", round_number=1,
                       model_weights={n: prev[n] + 0.05 * torch.randn(*s, generator=g)
                                      for n, s in shapes.items()},
                       num_samples=10 + k, training_loss=0.5, privacy_budget_used=0.5,
                       compression_ratio=0.8, timestamp=datetime.now()) for k in range(5)]

    def flat(w):
        return np.concatenate([w[n].detach().cpu().numpy().reshape(-1) for n in shapes])
    rows = np.stack([flat(u.model_weights) for u in ups])
    gm_model = GlobalModel(round_number=0, model_weights=prev, accuracy_metrics={},
                           participating_clients=[], convergence_score=0.0,
                           created_at=datetime.now())
    cc = robust.CenteredClipAggregator(tau=0.2, iters=2)
    got = cc.aggregate_updates(ups, gm_model)
    want, _ = cr.centered_clip(rows, [0.2] * 5, 0.2, iters=2, center=flat(prev),
                               replay=list(cc.last_sqdist.cpu().numpy()))
    assert cr.same_bits(flat(got.model_weights), want)
    assert [got.model_weights[n].shape for n in shapes] == [torch.Size(s)
                                                            for s in shapes.values()]
    assert cc.aggregation_history[-1]["num_clients"] == 5
    gmed = robust.GeometricMedianAggregator(iters=2)
    got = gmed.aggregate_updates(ups)  # no centre: starts from the coordinate-wise median
    want, _ = cr.geometric_median(rows, cr.sample_weights([10 + k for k in range(5)]), iters=2,
                                  replay=list(gmed.last_sqdist.cpu().numpy()))
    assert cr.same_bits(flat(got.model_weights), want)


# ------------------------------------------------------------------ RankRound
SIZES = [70, 55, 48, 40]


def _client_data(k, n):
    g = torch.Generator().manual_seed(200 + k)
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _round(**kw):
    """One round of SimpleCNN over SIZES' four clients; returns the previous global vector, the
    trained rows in client order (copied by the on_trained hook) and the new global vector."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    r = RankRound(model, SIZES, list(range(4)), epochs=1, device=DEV, lanes=1, shuffle_seed=77,
                  **kw)
    g0 = r.global_flat.cpu().numpy().copy()
    xs, ys = zip(*[_client_data(k, SIZES[k]) for k in r.slots])
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    r.run(data, labels, offs, "sgd", 0.01, seed=3)
    torch.cuda.synchronize()
    return g0, np.stack([seen[k] for k in range(4)]), r.global_flat.cpu().numpy().copy()


def test_rankround_with_the_center_rules():
    alpha = cr.sample_weights(SIZES)
    gm = robust.GeometricMedianAggregator(iters=2)
    g0, rows, glob = _round(aggregator=gm)
    want, info = cr.geometric_median(rows, alpha, iters=2, center=g0,
                                     replay=list(gm.last_sqdist.cpu().numpy()))
    assert cr.same_bits(glob, want) and not cr.same_bits(glob, g0)
    assert gm.last_rejected == [] and gm.last_objective == info["objective"]
    tau = 0.5 * float(np.sqrt(cr.sqdist(rows, g0).min()))  # every client is clipped
    cc = robust.CenteredClipAggregator(tau=tau, iters=2)
    g0, rows, glob = _round(aggregator=cc)
    want, _ = cr.centered_clip(rows, [0.25] * 4, tau, iters=2, center=g0,
                               replay=list(cc.last_sqdist.cpu().numpy()))
    assert cr.same_bits(glob, want) and not cr.same_bits(glob, g0)
    assert np.all(np.array(cc.last_coef) < 0.25)
    # a server optimizer whose base is the rule: the rule's aggregate around the previous
    # global, then one FedAdam step toward it
    gm = robust.GeometricMedianAggregator(iters=1)
    so = fedopt.FedAdam(0.05, base=gm, device=DEV)
    g0, rows, glob = _round(server_opt=so)
    agg, _ = cr.geometric_median(rows, alpha, iters=1, center=g0,
                                 replay=list(gm.last_sqdist.cpu().numpy()))
    tau32 = F(so.tau)
    m0, v0 = np.zeros(g0.size, dtype=F), np.full(g0.size, tau32 * tau32, dtype=F)
    want = fr.server_opt_step(fr.ADAM, agg[None], None, g0, m0, v0, server_lr=so.server_lr,
                              beta1=so.beta1, beta2=so.beta2, tau=so.tau)
    assert cr.same_bits(glob, want[0])
    # ... and step_packed hands the rule the global vector as its centre, too
    so2 = fedopt.FedAdam(0.05, base=robust.CenteredClipAggregator(tau=tau), device=DEV)
    gd = torch.from_numpy(g0.copy()).to(DEV)
    so2.step_packed(_place(rows, rows.shape[1] + 2, 0), SIZES, gd)
    agg, _ = cr.centered_clip(rows, [0.25] * 4, tau, iters=1, center=g0,
                              replay=list(so2.base.last_sqdist.cpu().numpy()))
    want = fr.server_opt_step(fr.ADAM, agg[None], None, g0, m0, v0, server_lr=so2.server_lr,
                              beta1=so2.beta1, beta2=so2.beta2, tau=so2.tau)
    assert cr.same_bits(gd.cpu().numpy(), want[0])
