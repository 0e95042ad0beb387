"""tests/fltrust_ref.py, the numpy definition of FLTrust that the GPU tests compare against,
pinned on hand-worked cases; and the host-side refusals of FLTrustAggregator and
RankRound(trust_root=) that need no GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import fltrust_ref as tr
from fedhip import _lib
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgAggregator, FedAvgError

F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")

# d0 = (3, 4): |d0| = 5.  Deltas with cosine 1, 0, -1 and 3/5 against it.
G = np.array([1.0, -2.0], dtype=F)
D0 = np.array([3.0, 4.0], dtype=F)
DELTAS = np.array([[6.0, 8.0], [4.0, -3.0], [-3.0, -4.0], [5.0, 0.0]], dtype=F)
ROOT, ROWS = G + D0, G + DELTAS


def test_small_integer_deltas_by_hand():
    sq, dot, sq0 = tr.stats(ROWS, ROOT, G)
    assert sq.tolist() == [100.0, 25.0, 25.0, 25.0] and dot.tolist() == [50.0, 0.0, -25.0, 15.0]
    assert sq0 == 25.0
    coef, trust, state = tr.coefficients(sq, dot, sq0)
    assert trust.tolist() == [1.0, 0.0, 0.0, 15.0 / 25.0]
    S = Fraction(1) + Fraction(trust[3])             # what fp64 holds of 3/5, exactly
    assert state.tolist() == [1.0 + 0.6, 4.0, 2.0, 5.0] and Fraction(state[0]) - S <= 2 ** -52
    # c_0 = 1 * (5 / 10) / 1.6 = 5/16, c_3 = (3/5) * (5 / 5) / 1.6 = 3/8: both fp32 numbers, and
    # the fp64 chain's few-ulp error is far from moving the rounding to fp32
    assert coef.dtype == F and coef.tolist() == [0.3125, 0.0, 0.0, 0.375]
    out, coef2, trust2, st, state2 = tr.fltrust_rows(tr.STEP, ROWS, ROOT, G)
    # out = g + 5/16 * (6, 8) + 3/8 * (5, 0) = g + (3.75, 2.5), every operation exact
    assert out.dtype == F and out.tolist() == [4.75, 0.5]
    assert tr.same_bits(coef2, coef) and np.array_equal(trust2, trust)
    assert st.tolist() == [100.0, 25.0, 25.0, 25.0, 50.0, 0.0, -25.0, 15.0, 25.0]
    assert tr.fltrust_rows(tr.SCORE, ROWS, ROOT, G)[0] is None
    want, ts64, c64 = tr.rule_fp64(ROWS, ROOT, G)
    assert np.allclose(want, [4.75, 0.5], rtol=1e-15) and np.allclose(ts64, trust, rtol=1e-15)
    # sqdist_after: the clients' squared distances to the new model (3.75, 2.5) + g
    assert tr.step(ROWS, coef, G)[1].tolist() == [2.25 ** 2 + 5.5 ** 2, 0.25 ** 2 + 5.5 ** 2,
                                                  6.75 ** 2 + 6.5 ** 2, 1.25 ** 2 + 2.5 ** 2]


def test_a_client_equal_to_g_is_not_live():
    rows = np.concatenate([ROWS[:1], G[None]])
    sq, dot, sq0 = tr.stats(rows, ROOT, G)
    coef, trust, state = tr.coefficients(sq, dot, sq0)
    assert sq[1] == 0.0 and trust.tolist() == [1.0, 0.0] and coef.tolist() == [0.5, 0.0]
    assert state.tolist() == [1.0, 1.0, 1.0, 5.0]     # S, one live client, one trusted, n0
    assert tr.step(rows, coef, G)[0].tolist() == [4.0, 2.0]  # g + d0: the delta at the root's norm


def test_zero_root_delta_and_nobody_trusted_leave_g_bit_for_bit():
    g = np.array([0x80000000, 0xFFA5A5A5, 0x00000001, 0x3F800000], dtype=np.uint32).view(F)
    rows = np.array([[1, 2, 3, 4], [0, 1, 0, 1]], dtype=F)
    out, coef, trust, st, state = tr.fltrust_rows(tr.STEP, rows, g, g)   # root == g
    assert tr.same_bits(out, g) and not coef.any() and not np.signbit(coef).any()
    assert not trust.any() and state[0] == 0.0 and st[-1] != st[-1]      # NaN - NaN in g
    g2 = np.array([-0.0, 0.0, 1.0, 2.0], dtype=F)
    out, coef, trust, st, state = tr.fltrust_rows(tr.STEP, rows, g2, g2)
    assert tr.same_bits(out, g2) and st[-1] == 0.0 and state.tolist() == [0.0, 2.0, 0.0, 0.0]
    # a root that moved, and every client against it
    root = g2 + np.array([1, 1, 0, 0], dtype=F)
    away = g2 - np.array([[1, 2, 0, 0], [3, 0, 5, 0]], dtype=F)
    out, coef, trust, st, state = tr.fltrust_rows(tr.STEP, away, root, g2)
    assert tr.same_bits(out, g2) and not coef.any() and state[:3].tolist() == [0.0, 2.0, 0.0]
    # an infinite root delta: sq0 is not finite
    root[0] = INF
    out, coef, *_ = tr.fltrust_rows(tr.STEP, rows, root, g2)
    assert tr.same_bits(out, g2) and not coef.any()


def test_appending_distrusted_and_broken_rows_changes_no_bit():
    rng = np.random.default_rng(3)
    P = 37
    g = rng.standard_normal(P).astype(F)
    d0 = rng.standard_normal(P).astype(F)
    rows = (g + 0.5 * d0 + 0.3 * rng.standard_normal((3, P))).astype(F)
    base, coef, *_ = tr.fltrust_rows(tr.STEP, rows, g + d0, g)
    assert (coef > 0).all()
    nan_row, inf_row, ninf_row = rows[0].copy(), rows[1].copy(), rows[2].copy()
    nan_row[5], inf_row[:], ninf_row[::2] = NAN, INF, -INF
    extra = np.stack([(g - d0).astype(F), (g - 2 * d0).astype(F), nan_row, inf_row, ninf_row])
    out, coef2, trust2, _, state = tr.fltrust_rows(tr.STEP, np.concatenate([rows, extra]),
                                                   g + d0, g)
    assert tr.same_bits(out, base) and tr.same_bits(coef2[:3], coef)
    assert not coef2[3:].any() and not trust2[3:].any() and state[1:3].tolist() == [5.0, 3.0]
    out, *_ = tr.fltrust_rows(tr.STEP, np.concatenate([extra, rows]), g + d0, g)
    assert tr.same_bits(out, base)    # whatever their position


def test_scaling_a_delta_by_1000_keeps_its_contribution():
    """Small integers: d' = 1000 * d, its squares and dot product are exact, so the fp64 chain
    gives c' = c / 1000 up to a few fp64 ulps, then one fp32 rounding on either side: the
    contributions fl32(c' * d') and fl32(c * d) differ by at most 4 * 2^-24 relative (two
    roundings of c, two of the products); 1.01 covers the second order and the fp64 crumbs."""
    rng = np.random.default_rng(5)
    P = 64
    g = np.zeros(P, dtype=F)
    d0 = rng.integers(-9, 10, P).astype(F)
    rows = rng.integers(-9, 10, (3, P)).astype(F)
    rows[0] = d0 + rng.integers(-2, 3, P).astype(F)   # one surely trusted client
    rows[1] = 2 * d0 - rows[0]                        # and one it is compared with
    big = rows.copy()
    big[0] *= 1000
    c = tr.fltrust_rows(tr.SCORE, rows, d0, g)[1]
    cb = tr.fltrust_rows(tr.SCORE, big, d0, g)[1]
    assert c[0] > 0 and tr.same_bits(cb[1:], c[1:])   # the others do not notice
    assert abs(float(cb[0]) * 1000 - float(c[0])) <= 2.02 * 2.0 ** -24 * float(c[0])
    t, tb = c[0] * rows[0], cb[0] * big[0]
    assert t.dtype == F and (np.abs(tb.astype(D) - t.astype(D)) <=
                             4.04 * 2.0 ** -24 * np.abs(t.astype(D))).all()


@pytest.mark.parametrize("C", [1, 3, 8])
def test_all_clients_equal_to_the_root_give_the_root(C):
    """Every cosine is 1 (clipped from 1 +- 2^-52), c_k = fl32(1/C) up to an ulp.  acc sums C
    terms c_k * d0: one rounding in c_k, one in the product, C - 1 adds, and d0 = fl32(r - g)
    carries one more: (C + 2) * 2^-24 * |r - g|; the final add rounds once at |out| ~ |r|."""
    rng = np.random.default_rng(C)
    P = 101
    g = rng.standard_normal(P).astype(F)
    r = (g + rng.standard_normal(P) * 0.1).astype(F)
    out, coef, trust, _, state = tr.fltrust_rows(tr.STEP, np.tile(r, (C, 1)), r, g)
    assert (np.abs(trust - 1.0) <= 2.0 ** -51).all() and abs(state[0] - C) <= C * 2.0 ** -51
    assert (np.abs(coef.astype(D) - 1.0 / C) <= 2.0 ** -24 / C).all()
    r64, g64 = r.astype(D), g.astype(D)
    bound = 1.01 * 2.0 ** -24 * ((C + 2) * np.abs(r64 - g64) + np.abs(r64))
    assert (np.abs(out.astype(D) - r64) <= bound).all()


# ------------------------------------------------------------------ host side of the rule
def test_factory_and_attributes():
    agg = robust.create_robust_aggregator("fltrust")
    assert isinstance(agg, robust.FLTrustAggregator) and isinstance(agg, FedAvgAggregator)
    assert agg.uses_center and agg.uses_root
    assert not getattr(robust.CenteredClipAggregator(tau=1.0), "uses_root", False)


def test_aggregator_refusals_name_what_is_missing():
    agg = robust.FLTrustAggregator()
    rows = torch.zeros(3, 4)
    with pytest.raises(FedAvgError, match="No updates"):
        agg.aggregate_packed(rows, [], center=rows[0], root_row=2)
    with pytest.raises(FedAvgError, match="center .*and root_row"):
        agg.aggregate_packed(rows, [1, 1])
    with pytest.raises(FedAvgError, match="needs root_row"):
        agg.aggregate_packed(rows, [1, 1], center=torch.zeros(4))
    with pytest.raises(FedAvgError, match="needs center"):
        agg.aggregate_packed(rows, [1, 1], root_row=2)
    with pytest.raises(FedAvgError, match="one of the clients"):
        agg.aggregate_packed(rows, [1, 1], center=torch.zeros(4), root_row=1)
    with pytest.raises(FedAvgError, match="one of the clients"):
        agg.aggregate_packed(rows, [1, 1], row_index=[2, 0], center=torch.zeros(4), root_row=2)
    with pytest.raises(FedAvgError, match="not a row"):
        agg.aggregate_packed(rows, [1, 1], center=torch.zeros(4), root_row=3)
    with pytest.raises(FedAvgError, match="differ in length"):
        agg.aggregate_packed(rows, [1, 1], row_index=[0], center=torch.zeros(4), root_row=2)
    with pytest.raises(FedAvgError, match="no row_index"):
        agg.aggregate_packed(rows, [1, 1], center=torch.zeros(4), root_row=torch.zeros(4))
    # the reference-style entry: never a silent FedAvg
    with pytest.raises(FedAvgError, match="global_model .*and server_update"):
        agg.aggregate_updates([object()])
    with pytest.raises(FedAvgError, match="needs server_update"):
        from src.shared.models import GlobalModel
        agg.aggregate_updates([object()], GlobalModel(0, {}, {}, [], 0.0))
    with pytest.raises(FedAvgError, match="its own weights"):
        agg.aggregate_updates([object()], None, None, weights=[1.0])
    with pytest.raises(FedAvgError, match="center= and root_row="):
        agg._weighted_average([object()], [1.0])


def _round(**kw):
    from fedhip import round as fround
    return fround.RankRound(torch.nn.Linear(2, 2), kw.pop("sizes", [10, 10, 0]),
                            kw.pop("mine", [0, 1, 2]), **kw)


def test_rankround_trust_root_refusals(monkeypatch):
    """Checked at construction, before the trainer (and the device) is touched."""
    flt = robust.FLTrustAggregator
    for kw, msg in ((dict(aggregator=flt()), "pass trust_root"),
                    (dict(server_opt=fedopt.FedAdam(0.1, base=flt())), "pass trust_root"),
                    (dict(trust_root=0), "FLTrustAggregator"),
                    (dict(trust_root=0, aggregator=robust.MedianAggregator()), "FLTrustAggregator"),
                    (dict(trust_root=3, aggregator=flt()), "not a client of the round"),
                    (dict(trust_root=-1, aggregator=flt()), "not a client of the round"),
                    (dict(trust_root=True, aggregator=flt()), "not a client of the round"),
                    (dict(trust_root=1, aggregator=flt(), mine=[0, 2]), "this rank's clients"),
                    (dict(trust_root=2, aggregator=flt()), "empty"),
                    (dict(trust_root=0, aggregator=flt(), mine=[0]), "0 clients beside"),
                    (dict(trust_root=0, aggregator=flt(), sizes=[8] * 66, mine=list(range(66))),
                     "65 clients beside"),
                    (dict(trust_root=0, aggregator=flt(), fednova=True), "fednova"),
                    (dict(trust_root=0, aggregator=flt(), qfedavg=True), "qfedavg")):
        with pytest.raises(_lib.FedHipError, match=msg):
            _round(**kw)
    from fedhip import round as fround
    monkeypatch.setattr(fround.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(fround.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(_lib.FedHipError, match="exact=True"):
        _round(trust_root=0, aggregator=flt(), group=object())
    # gathered: the root may live on another rank, and the limit counts every client
    with pytest.raises(_lib.FedHipError, match="65 clients beside"):
        _round(trust_root=1, aggregator=flt(), group=object(), exact=True, sizes=[8] * 66,
               mine=[0])
