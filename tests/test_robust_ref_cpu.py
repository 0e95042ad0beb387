"""CPU tier for the robust aggregation rules: pins the numpy references of tests/robust_ref.py
(which the GPU tests hold the kernels to, bit for bit) against np.sort / np.median and
hand-made cases, and checks everything the product validates on the host: the argument checks
of the two entry points (no launch), the aggregator classes' ranges, Krum's n >= 2f + 3 and
RankRound's refusal of a robust rule over several ranks without exact=True."""
import math

import numpy as np
import pytest
import torch

import robust_ref as rr
from fedhip import _lib
from src.aggregation import robust
from src.aggregation.fedavg import FedAvgAggregator, FedAvgError


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("C,trim", [(1, 0), (2, 0), (5, 0), (5, 1), (5, 2), (8, 3), (9, 4),
                                    (33, 7), (64, 31)])
def test_trimmed_mean_equals_sorted_sequential_sum(C, trim):
    """Finite data without signed zeros: np.sort, then a sequential fp32 sum and division."""
    rng = np.random.default_rng(C * 100 + trim)
    rows = rng.standard_normal((C, 257)).astype(np.float32)
    s = np.sort(rows, axis=0)
    want = np.empty(257, dtype=np.float32)
    for j in range(257):
        acc = np.float32(s[trim, j])
        for k in range(trim + 1, C - trim):
            acc = np.float32(acc + s[k, j])
        want[j] = np.float32(acc / np.float32(C - 2 * trim))
    assert rr.same_bits(rr.trimmed_mean(rows, trim), want)
    assert rr.same_bits(rr.sorted_rows(rows), s)


@pytest.mark.parametrize("C", [1, 3, 7, 33])
def test_median_equals_np_median_for_odd_counts(C):
    rng = np.random.default_rng(C)
    rows = rng.standard_normal((C, 101)).astype(np.float32)
    assert rr.same_bits(rr.median(rows), np.median(rows, axis=0).astype(np.float32))


def test_median_even_count_is_the_mean_of_the_middle_pair():
    rows = np.array([[4.0], [1.0], [3.0], [10.0]], dtype=np.float32)
    assert rr.median(rows)[0] == np.float32(3.5)


def test_total_order_of_special_values():
    neg_nan, pos_nan_payload = f32(0xFFC12345), f32(0x7F800001)  # a quiet and a signalling NaN
    col = np.array([pos_nan_payload, np.inf, 1.0, 0.0, -0.0, -1e-45, -1.0, -np.inf, neg_nan,
                    1e-45], dtype=np.float32)
    k = rr.keys(col)
    order = np.argsort(k, kind="stable")
    got = _bits(col[order])
    want = _bits(np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32))
    assert np.array_equal(got[:8], want)
    assert k[0] == k[8] == rr.KEY_NAN and k[1] < rr.KEY_NAN  # one NaN key, above +Inf
    assert np.array_equal(_bits(rr.unkey(k))[[0, 8]], [rr.QNAN_BITS] * 2)
    non_nan = np.array([np.inf, 1.0, 0.0, -0.0, -1e-45, -np.inf], dtype=np.float32)
    assert rr.same_bits(rr.unkey(rr.keys(non_nan)), non_nan)  # the transform is a bijection
    rows = col.reshape(-1, 1)
    # trim 2 drops {-Inf, -1} and {NaN, NaN}: (((-1e-45 + -0) + +0) + 1e-45 + 1) + Inf = Inf
    assert rr.trimmed_mean(rows, 2)[0] == np.inf
    # trim 1 keeps one NaN: it propagates, as the one quiet NaN
    assert _bits(rr.trimmed_mean(rows, 1))[0] == rr.QNAN_BITS
    # trim 3 keeps -0, +0, 1e-45, 1: the sum is 1 in fp32
    assert rr.trimmed_mean(rows, 3)[0] == np.float32(0.25)
    # -Inf + Inf inside the window is a NaN result, written as the same quiet NaN
    assert _bits(rr.trimmed_mean(np.array([[-np.inf], [np.inf]], np.float32), 0))[0] == rr.QNAN_BITS
    # signed zeros: -0 sorts below +0, and (-0 + -0) / 2 stays -0
    assert _bits(rr.trimmed_mean(np.array([[0.0], [-0.0], [-0.0], [5.0]], np.float32), 1))[0] \
        == 0  # kept: -0, +0
    assert _bits(rr.trimmed_mean(np.array([[-0.0], [-0.0], [-3.0], [5.0]], np.float32), 1))[0] \
        == 0x80000000


def test_row_permutation_leaves_the_bits_unchanged():
    rng = np.random.default_rng(7)
    rows = rng.integers(-3, 4, size=(9, 300)).astype(np.float32)  # heavily tied
    rows[2, ::7] = np.nan
    rows[5, ::11] = -0.0
    rows[6, ::13] = np.inf
    for trim in (0, 2, 4):
        want = rr.trimmed_mean(rows, trim)
        for seed in range(3):
            perm = np.random.default_rng(seed).permutation(9)
            assert rr.same_bits(rr.trimmed_mean(rows[perm], trim), want)


def test_pairwise_reference_small_case():
    rows = np.array([[0, 0, 0], [1, 2, 2], [-1, 0, 4]], dtype=np.float32)
    d = rr.pairwise_sqdist(rows)
    assert d.dtype == np.float64 and np.array_equal(d, d.T) and not d.diagonal().any()
    assert d[0, 1] == 9 and d[0, 2] == 17 and d[1, 2] == 12


def _outlier_case():
    """9 points on a line: 7 honest ones at 0, 1, .., 6 (/ 64, so every distance is exact) and
    outliers at 50 and -80."""
    x = np.array([0, 1, 3200, 2, 3, 4, -5120, 5, 6]) / 64.0
    rows = np.stack([x, 2 * x], axis=1).astype(np.float32)
    return rows, [2, 6]


def test_krum_selection_matches_brute_force_and_drops_the_outliers():
    rows, outliers = _outlier_case()
    dist = rr.pairwise_sqdist(rows)
    for f, m in ((2, 1), (2, 7), (2, 3), (3, 6), (0, 9)):
        want, scores = rr.krum_select(dist, f, m)
        assert robust.krum_select(dist, f, m) == want
        assert robust.krum_scores(dist, f) == scores
        if f >= 2:
            assert not set(want) & set(outliers)
    # Krum proper, n - f - 2 = 5 neighbours: the points 2/64, 3/64 and 4/64 (indices 3, 4, 5)
    # tie exactly (1 + 1 + 4 + 4 + 9, times 5 / 4096); the lowest index wins
    sc = robust.krum_scores(dist, 2)
    assert sc[3] == sc[4] == sc[5] == 19 * 5 / 4096 and min(sc) == sc[3]
    assert robust.krum_select(dist, 2, 1) == [3]
    # ties go to the lowest index: duplicate rows have equal scores
    dup = np.zeros((7, 7))
    assert robust.krum_select(dup, 1, 3) == [0, 1, 2]
    # a row of NaN distances ranks last, whatever its index
    bad = rr.pairwise_sqdist(rows)
    bad[0, :] = bad[:, 0] = np.nan
    bad[0, 0] = 0.0
    assert 0 not in robust.krum_select(bad, 2, 6)


def test_uniform_mean_is_the_fedavg_arithmetic():
    from oracle import fedavg_ref
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((3, 50)).astype(np.float32)
    assert rr.same_bits(rr.uniform_mean(rows, 3), fedavg_ref.weighted_average(rows, [1 / 3] * 3))


# ------------------------------------------------------------------ host-side validation
def test_entry_points_validate_on_the_host():
    """Bad arguments fail with a message before any launch (no device here)."""
    def tm(C, trim, P=8, stride=8):
        _lib.call("fh_trimmed_mean_rows", None, stride, None, C, trim, P, None, None)
    for C, trim in ((0, 0), (65, 0), (-1, 0)):
        with pytest.raises(_lib.FedHipError, match=r"outside \[1, 64\]"):
            tm(C, trim)
    for C, trim in ((4, 2), (5, 3), (1, 1), (8, -1), (64, 32)):
        with pytest.raises(_lib.FedHipError, match="trim"):
            tm(C, trim)
    with pytest.raises(_lib.FedHipError, match="bad sizes"):
        tm(4, 1, P=-1)
    with pytest.raises(_lib.FedHipError, match="null pointer"):
        tm(4, 1)
    assert _lib.call("fh_trimmed_mean_rows", None, 8, None, 4, 1, 0, None, None) == 0  # P == 0

    def pw(C, P=8):
        _lib.call("fh_pairwise_sqdist", None, 8, None, C, P, None, 0, None, None)
    for C in (0, 1, 65):
        with pytest.raises(_lib.FedHipError, match=r"outside \[2, 64\]"):
            pw(C)
    with pytest.raises(_lib.FedHipError, match="bad sizes"):
        pw(4, P=-1)
    with pytest.raises(_lib.FedHipError, match="null pointer"):
        pw(4)
    lib = _lib.load()
    # one double per pair and chunk of coordinates; chunks of >= 64 columns, about 1024 of them
    assert lib.fh_pairwise_sqdist_workspace(3, 1) == 3 * 8
    assert lib.fh_pairwise_sqdist_workspace(3, 65) == 2 * 3 * 8
    assert lib.fh_pairwise_sqdist_workspace(32, 1470890) == math.ceil(1470890 / 1472) * 496 * 8
    assert lib.fh_pairwise_sqdist_workspace(1, 100) == 0 == lib.fh_pairwise_sqdist_workspace(65, 100)


def test_aggregator_argument_ranges():
    for bad in (-0.1, 0.5, 0.7):
        with pytest.raises(ValueError, match="trim_ratio"):
            robust.TrimmedMeanAggregator(trim_ratio=bad)
    assert robust.TrimmedMeanAggregator(trim_ratio=0.3)._trim(7) == 2
    assert robust.TrimmedMeanAggregator()._trim(9) == 0 and robust.trim_count(0.1, 32) == 3
    assert [robust.MedianAggregator()._trim(c) for c in (1, 2, 3, 4, 7, 64)] == [0, 0, 1, 1, 3, 31]
    with pytest.raises(ValueError):
        robust.KrumAggregator(num_byzantine=-1)
    with pytest.raises(ValueError):
        robust.KrumAggregator(num_byzantine=1, num_selected=0)
    kinds = {"trimmed_mean": robust.TrimmedMeanAggregator, "median": robust.MedianAggregator,
             "krum": robust.KrumAggregator, "multi_krum": robust.KrumAggregator}
    for kind, cls in kinds.items():
        kw = {"num_byzantine": 2} if "krum" in kind else {}
        agg = robust.create_robust_aggregator(kind, **kw)
        assert type(agg) is cls and isinstance(agg, FedAvgAggregator)
    assert robust.create_robust_aggregator("krum", num_byzantine=2).num_selected == 1
    assert robust.create_robust_aggregator("multi_krum", num_byzantine=2).num_selected is None
    with pytest.raises(ValueError, match="unknown"):
        robust.create_robust_aggregator("mean")


def test_krum_needs_2f_plus_3_clients():
    with pytest.raises(FedAvgError, match="2f"):
        robust.krum_scores(np.zeros((6, 6)), 2)
    robust.krum_scores(np.zeros((7, 7)), 2)
    # the aggregator refuses before anything reaches the device
    agg = robust.KrumAggregator(num_byzantine=1)
    with pytest.raises(FedAvgError, match="2f"):
        agg.aggregate_packed(torch.zeros(4, 8), [10] * 4)
    with pytest.raises(FedAvgError, match="No updates"):
        agg.aggregate_packed(torch.zeros(0, 8), [])
    with pytest.raises(FedAvgError, match="row_index"):
        agg.aggregate_packed(torch.zeros(6, 8), [10] * 5, row_index=[0, 1])


def test_rankround_refuses_a_robust_rule_over_ranks_without_exact(monkeypatch):
    """Checked at construction, before the trainer (and the device) is touched."""
    from fedhip import round as fround
    monkeypatch.setattr(fround.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(fround.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(_lib.FedHipError, match="exact=True"):
        fround.RankRound(torch.nn.Linear(2, 2), [10, 10], [0], group=object(),
                         aggregator=robust.MedianAggregator())
