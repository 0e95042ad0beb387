"""Pins tests/center_ref.py (the reference the GPU tests of csrc/center.hip compare against) on
hand-worked cases, and the host side of the two rules: constructor refusals and the factory
kinds.  No GPU."""
import math

import numpy as np
import pytest

import center_ref as cr
from src.aggregation import robust
from src.aggregation.fedavg import FedAvgAggregator

F = np.float32
NAN, INF = float("nan"), float("inf")


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ------------------------------------------------------------------ center_iter
def test_iter_hand_cases():
    rows = np.array([[1, 2, 3], [3, 6, -1]], dtype=F)
    out, sq = cr.center_iter(cr.MEAN, rows, [0.5, 0.25])
    assert out.tolist() == [1.25, 2.5, 1.25]
    # distances to out: row 0 (-0.25, -0.5, 1.75), row 1 (1.75, 3.5, -2.25)
    assert sq.tolist() == [0.0625 + 0.25 + 3.0625, 3.0625 + 12.25 + 5.0625]
    g = np.array([1, 1, 1], dtype=F)
    out, sq = cr.center_iter(cr.DELTA, rows, [0.5, 0.25], center=g)
    # g + (0.5 * (x0 - g) + 0.25 * (x1 - g)) = 1 + (0, .5, 1) + (.5, 1.25, -.5)
    assert out.tolist() == [1.5, 2.75, 1.5]
    assert sq.tolist() == [0.25 + 0.5625 + 2.25, 2.25 + 10.5625 + 6.25]
    assert out.dtype == F and sq.dtype == np.float64


def test_iter_one_client_and_equal_rows():
    x = np.array([[0.1, -7.0, 2.0 ** -140]], dtype=F)  # a denormal (and its half) is kept
    out, sq = cr.center_iter(cr.MEAN, x, [1.0])
    assert cr.same_bits(out, x[0]) and sq.tolist() == [0.0]
    two = np.repeat(x, 2, axis=0)
    out, sq = cr.center_iter(cr.MEAN, two, [0.5, 0.5])
    assert cr.same_bits(out, x[0]) and sq.tolist() == [0.0, 0.0]
    out, sq = cr.center_iter(cr.DELTA, two, [0.5, 0.5], center=x[0])
    assert cr.same_bits(out, x[0]) and sq.tolist() == [0.0, 0.0]


def test_iter_rounds_every_operation():
    # 0.1f * 3 rounds, then + 1e8f absorbs it; an FMA or a wider accumulator would differ
    rows = np.array([[3.0], [1e8], [-1e8]], dtype=F)
    out, _ = cr.center_iter(cr.MEAN, rows, [0.1, 1.0, 1.0])
    assert float(out[0]) == 0.0
    t = F(0.1) * F(3.0)
    assert float(t) != 0.3 and float((t + F(1e8)) - F(1e8)) == 0.0


def test_iter_zero_coefficient_skips_the_row_but_not_its_distance():
    rows = np.array([[1, 2], [NAN, 5], [INF, -INF], [3, 4]], dtype=F)
    for zero in (0.0, -0.0):
        out, sq = cr.center_iter(cr.MEAN, rows, [0.5, zero, zero, 0.5])
        assert out.tolist() == [2.0, 3.0]
        assert sq[0] == 2.0 and sq[3] == 2.0 and math.isnan(sq[1]) and sq[2] == INF
        out, sq = cr.center_iter(cr.DELTA, rows, [0.5, zero, zero, 0.5],
                                 center=np.array([1, 1], dtype=F))
        assert out.tolist() == [2.0, 3.0] and math.isnan(sq[1]) and sq[2] == INF
    # a non-zero coefficient lets it through, as the one quiet NaN
    out, _ = cr.center_iter(cr.MEAN, rows, [0.5, 1e-30, 0.0, 0.5])
    assert bits(out)[0] == 0x7FC00000 and out[1] == 3.0
    out, _ = cr.center_iter(cr.MEAN, -rows, [0.5, 1.0, 0.0, 0.5])  # -NaN in, +qNaN out
    assert bits(out)[0] == 0x7FC00000
    # all coefficients zero: +0 in MEAN, the centre in DELTA
    out, sq = cr.center_iter(cr.MEAN, rows, [0.0] * 4)
    assert bits(out).tolist() == [0, 0] and sq[0] == 5.0
    out, _ = cr.center_iter(cr.DELTA, rows, [0.0] * 4, center=np.array([7, -0.0], dtype=F))
    assert bits(out).tolist() == bits(np.array([7, 0.0], dtype=F)).tolist()


# ------------------------------------------------------------------ center_coef
def test_coef_geomed_hand_cases():
    # d = (3, 4, 0.5 < nu = 1): b = (0.5/3, 0.25/4, 0.25/1)
    coef, st = cr.center_coef(cr.GEOMED, [9.0, 16.0, 0.25], [0.5, 0.25, 0.25], 1.0)
    b = [0.5 / 3.0, 0.25 / 4.0, 0.25]
    B = (b[0] + b[1]) + b[2]
    assert coef.tolist() == [float(F(x / B)) for x in b]
    assert st.tolist() == [3.0, (0.5 * 3.0 + 0.25 * 4.0) + 0.25 * 0.5, B, 1.0]
    # C = 1: coefficient exactly 1 whatever the distance
    for s in (0.0, 1e-30, 7.0):
        coef, st = cr.center_coef(cr.GEOMED, [s], [1.0], 1e-6)
        assert coef.tolist() == [1.0] and st[0] == 1.0
    # equal distances (e.g. equal rows, d = 0 < nu): coef = fl32(alpha_k)
    alpha = [0.1, 0.2, 0.3, 0.4]
    coef, st = cr.center_coef(cr.GEOMED, [0.0] * 4, alpha, 0.5)
    B = ((0.1 / 0.5 + 0.2 / 0.5) + 0.3 / 0.5) + 0.4 / 0.5
    assert coef.tolist() == [float(F((a / 0.5) / B)) for a in alpha]
    assert np.allclose(coef, alpha, rtol=2 ** -23, atol=0)
    assert st[1] == 0.0


def test_coef_cclip_hand_cases():
    # d = (0, 2 = tau, 8 > tau): factors 1, 1, 0.25
    coef, st = cr.center_coef(cr.CCLIP, [0.0, 4.0, 64.0], [0.25, 0.25, 0.5], 2.0)
    assert coef.tolist() == [0.25, 0.25, 0.125]
    assert st.tolist() == [3.0, (0.0 + 0.5) + 4.0, 0.625, 2.0]
    coef, _ = cr.center_coef(cr.CCLIP, [9.0], [1 / 3], 1.0)
    assert coef.tolist() == [float(F((1 / 3) * (1.0 / 3.0)))]


def test_coef_rejects_nonfinite_and_weightless_clients():
    sq = [4.0, NAN, INF, 1.0, 9.0]
    alpha = [0.25, 0.25, 0.25, 0.0, 0.25]
    for rule in (cr.GEOMED, cr.CCLIP):
        coef, st = cr.center_coef(rule, sq, alpha, 1.0)
        assert coef[1] == 0 and coef[2] == 0 and coef[3] == 0 and coef[0] > 0 and coef[4] > 0
        assert st[0] == 2.0 and st[1] == 0.25 * 2.0 + 0.25 * 3.0
        # all rejected: zeros, live = 0
        coef, st = cr.center_coef(rule, [NAN, INF, 1.0], [0.5, 0.5, 0.0], 1.0)
        assert bits(coef).tolist() == [0, 0, 0] and st[:3].tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------ the two rules
def _honest(C, P, seed):
    return np.random.default_rng(seed).standard_normal((C, P)).astype(F)


def test_nonfinite_rows_are_rejected_and_stay_rejected():
    rows = _honest(6, 40, 1)
    rows[1, 3] = NAN
    rows[4, 7] = INF
    alpha = cr.sample_weights([10, 20, 30, 40, 50, 60])
    out, info = cr.geometric_median(rows, alpha, iters=3, center=np.zeros(40, dtype=F))
    for c in info["coef"]:
        assert c[1] == 0 and c[4] == 0 and np.all(c[[0, 2, 3, 5]] > 0)
    assert info["rejected"] == [1, 4] and info["live"] == 4.0
    assert np.isfinite(out).all()
    out, info = cr.centered_clip(rows, [1 / 6] * 6, 2.0, iters=2, center=np.zeros(40, dtype=F))
    assert info["rejected"] == [1, 4] and np.isfinite(out).all()
    # without a centre the median start itself may be hit: still rejected from then on
    out, info = cr.geometric_median(rows, alpha, iters=2)
    assert info["rejected"] == [1, 4] and np.isfinite(out).all()


def test_all_rejected_gives_zeros():
    rows = np.full((3, 5), NAN, dtype=F)
    out, info = cr.geometric_median(rows, [1 / 3] * 3, iters=2, center=np.zeros(5, dtype=F))
    assert info["live"] == 0.0 and bits(out).tolist() == [0] * 5
    assert bits(info["last_coef"]).tolist() == [0] * 3


def test_geomed_equal_rows_and_single_client():
    x = _honest(1, 17, 2)
    out, info = cr.geometric_median(x, [1.0], iters=3)
    assert cr.same_bits(out, x[0]) and info["last_coef"].tolist() == [1.0]
    rows = np.repeat(x, 4, axis=0)
    alpha = [0.1, 0.2, 0.3, 0.4]
    out, info = cr.geometric_median(rows, alpha, nu=1e-6, iters=2)
    # every distance is 0 < nu: b_k = alpha_k / nu, coef = fl32(alpha_k) up to the rounding of B
    assert np.allclose(info["last_coef"], alpha, rtol=2 ** -22, atol=0)
    assert np.allclose(out, x[0], rtol=1e-6, atol=0)


def test_cclip_with_a_huge_tau_is_the_fedavg_of_deltas():
    rows, g = _honest(5, 33, 3), _honest(1, 33, 4)[0]
    alpha = cr.sample_weights([3, 1, 4, 1, 5])
    out, info = cr.centered_clip(rows, alpha, 1e300, iters=1, center=g)
    assert info["last_coef"].tolist() == [float(F(a)) for a in alpha]
    acc = np.zeros(33, dtype=F)
    for x, a in zip(rows, alpha):
        acc = acc + F(a) * (x - g)
    assert cr.same_bits(out, g + acc)


def test_weiszfeld_objective_does_not_increase():
    rows = _honest(9, 200, 5)
    rows[:2] += 30.0
    alpha = [1 / 9] * 9
    out, info = cr.geometric_median(rows, alpha, nu=1e-6, iters=6)
    obj = [float(s[1]) for s in info["state"]]
    # Exact Weiszfeld steps never increase the objective.  The fp32 centre is off the exact one
    # by at most (C + 1) roundings of a sum whose terms are bounded by max ||x_k||, and the
    # objective (sum alpha = 1) is 1-Lipschitz in the centre: that is the only slack allowed.
    slack = (9 + 1) * 2.0 ** -24 * max(np.linalg.norm(x.astype(np.float64)) for x in rows)
    assert all(b <= a + slack for a, b in zip(obj, obj[1:])), obj
    assert obj[1] < obj[0] - slack and obj[2] < obj[1] - slack
    assert obj[-1] < obj[0] and info["objective"] == obj[-1]


def test_replay_uses_the_given_distances():
    rows, alpha = _honest(4, 9, 6), [0.25] * 4
    _, own = cr.geometric_median(rows, alpha, iters=2)
    out, same = cr.geometric_median(rows, alpha, iters=2, replay=own["sqdist"])
    assert cr.same_bits(out, cr.geometric_median(rows, alpha, iters=2)[0])
    fake = [np.array([1.0, 4.0, 9.0, 16.0])] * 3
    out2, info = cr.geometric_median(rows, alpha, iters=2, replay=fake)
    want, _ = cr.center_coef(cr.GEOMED, fake[0], alpha, 1e-6)
    assert cr.same_bits(info["last_coef"], want) and not cr.same_bits(out, out2)


def test_robustness_condition_holds_for_the_reference():
    """C = 9, three rows at 1e4 (one with a NaN): both rules stay within the honest cloud,
    plain FedAvg does not."""
    rows = _honest(9, 1001, 7)
    bad = [1, 4, 6]
    rows[bad] = 1e4
    rows[4, 17] = NAN
    honest = np.delete(rows, bad, axis=0)
    mean = honest.astype(np.float64).mean(axis=0)
    radius = max(np.linalg.norm(x - mean) for x in honest.astype(np.float64))
    alpha = [1 / 9] * 9
    out, info = cr.geometric_median(rows, alpha)
    assert np.linalg.norm(out - mean) < radius and 4 in info["rejected"]
    tau = float(np.median(np.linalg.norm(honest.astype(np.float64), axis=1)))
    out, info = cr.centered_clip(rows, alpha, tau, iters=1, center=np.zeros(1001, dtype=F))
    assert np.linalg.norm(out - mean) < radius and 4 in info["rejected"]
    finite = np.delete(rows, 4, axis=0)  # FedAvg of even the finite rows is far outside
    fedavg = finite.astype(np.float64).mean(axis=0)
    assert np.linalg.norm(fedavg - mean) > radius


# ------------------------------------------------------------------ host side of the rules
@pytest.mark.parametrize("kw", [dict(nu=0.0), dict(nu=-1.0), dict(nu=NAN), dict(nu=INF),
                                dict(nu="1"), dict(iters=0), dict(iters=1.5), dict(iters=True),
                                dict(weighting="median")])
def test_geometric_median_constructor_refusals(kw):
    with pytest.raises(ValueError):
        robust.GeometricMedianAggregator(**kw)


@pytest.mark.parametrize("kw", [dict(tau=0.0), dict(tau=-2.0), dict(tau=NAN), dict(tau=INF),
                                dict(tau=None), dict(tau=1.0, iters=0),
                                dict(tau=1.0, weighting="krum")])
def test_centered_clip_constructor_refusals(kw):
    with pytest.raises(ValueError):
        robust.CenteredClipAggregator(**kw)


def test_factory_kinds_and_defaults():
    gm = robust.create_robust_aggregator("geometric_median")
    assert isinstance(gm, robust.GeometricMedianAggregator) and isinstance(gm, FedAvgAggregator)
    assert (gm.nu, gm.iters, gm.weighting, gm.uses_center) == (1e-6, 3, "samples", True)
    cc = robust.create_robust_aggregator("centered_clip", tau=2.5, iters=2)
    assert isinstance(cc, robust.CenteredClipAggregator)
    assert (cc.tau, cc.iters, cc.weighting, cc.uses_center) == (2.5, 2, "uniform", True)
    assert gm._alpha([1, 3]) == [0.25, 0.75] and cc._alpha([1, 3]) == [0.5, 0.5]
    assert not getattr(robust.MedianAggregator(), "uses_center", False)
    with pytest.raises(ValueError):
        robust.create_robust_aggregator("geometric_mean")
    with pytest.raises(TypeError):
        robust.create_robust_aggregator("centered_clip")  # tau is required
