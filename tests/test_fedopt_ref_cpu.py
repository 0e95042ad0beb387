"""CPU tier for the adaptive server optimizers: pins the numpy reference of tests/fedopt_ref.py
(which the GPU tests hold fh_server_opt_step to, bit for bit) against hand-worked cases, and
checks everything the product validates on the host: the entry point's argument checks (no
launch), the ServerOptimizer constructor and load_state_dict, and RankRound's refusal of a
robust rule given twice."""
import ctypes

import numpy as np
import pytest
import torch

import fedopt_ref as fr
from fedhip import _lib, ops
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import AdaptiveFedAvg, FedAvgAggregator, FedAvgError

F = np.float32
# exactly representable scalars: every intermediate below is exact, so the expected values are
# plain decimal literals
LR, B1, B2, TAU = 2.0, 0.5, 0.75, 1.0


def _step(rule, a, g, m, v, **kw):
    sc = dict(server_lr=LR, beta1=B1, beta2=B2, tau=TAU)
    sc.update(kw)
    return fr.server_opt_step(rule, np.array([a], dtype=F), None, np.array(g, dtype=F),
                              np.array(m, dtype=F), None if v is None else np.array(v, dtype=F),
                              **sc)


def test_rule_ids_match_the_header():
    assert (fr.MOMENTUM, fr.ADAGRAD, fr.ADAM, fr.YOGI) == (0, 1, 2, 3)
    assert (ops.SOPT_MOMENTUM, ops.SOPT_ADAGRAD, ops.SOPT_ADAM, ops.SOPT_YOGI) == (0, 1, 2, 3)
    assert fedopt.RULES == {"fedavgm": 0, "fedadagrad": 1, "fedadam": 2, "fedyogi": 3}


def test_known_answers_momentum():
    # d = a - g = [2, -2, 0];  m' = 0.5*m + d;  g' = g + 2*m'
    g, m, v = _step(fr.MOMENTUM, [3, -1, 1], [1, 1, 1], [4, -4, 6], None)
    assert v is None
    assert np.array_equal(m, F([4, -4, 3])) and np.array_equal(g, F([9, -7, 7]))


def test_known_answers_adagrad():
    # d = [2, -2];  m' = 0.5*m + 0.5*d = [3, -3];  v' = v + 4 = [9, 4]
    # g' = g + 2 * m' / (sqrt(v') + 1) = 1 + 2*[3/4, -3/3]
    g, m, v = _step(fr.ADAGRAD, [3, -1], [1, 1], [4, -4], [5, 0])
    assert np.array_equal(m, F([3, -3])) and np.array_equal(v, F([9, 4]))
    assert np.array_equal(g, F([2.5, -1]))


def test_known_answers_adam():
    # d = [2, -2];  m' = [3, -3];  v' = 0.75*v + 0.25*4 = [4, 16]
    # g' = 1 + 2 * [3/3, -3/5]:  -0.6 is not exact, the one rounded division is
    g, m, v = _step(fr.ADAM, [3, -1], [1, 1], [4, -4], [4, 20])
    assert np.array_equal(m, F([3, -3])) and np.array_equal(v, F([4, 16]))
    assert g[0] == F(3) and g[1] == F(1) + F(2) * (F(-3) / F(5))


def test_known_answers_yogi_all_three_signs():
    # d = 2, d^2 = 4, (1-b2)*d^2 = 1:  v = 10 > d^2 -> 9;  v = 3 < d^2 -> 4;  v = 4 == d^2 -> 4
    g, m, v = _step(fr.YOGI, [3, 3, 3], [1, 1, 1], [4, 4, 4], [10, 3, 4])
    assert np.array_equal(v, F([9, 4, 4])) and np.array_equal(m, F([3, 3, 3]))
    assert np.array_equal(g, F([2.5, 3, 3]))
    # a NaN in v - d^2 takes s = 0: v' = v - (o2 * 0) is then NaN through v itself
    g, m, v = _step(fr.YOGI, [3], [1], [4], [np.nan])
    assert v.view(np.uint32)[0] == 0x7FC00000 and g.view(np.uint32)[0] == 0x7FC00000
    assert m[0] == F(3)
    # d^2 = Inf with v = Inf: t = NaN, s = 0, o2 * 0 = NaN
    g, m, v = _step(fr.YOGI, [3e38], [-3e38], [0], [np.inf])
    assert v.view(np.uint32)[0] == 0x7FC00000


def test_every_nan_is_the_one_quiet_nan():
    neg_nan = np.array([0xFFC12345], dtype=np.uint32).view(F)[0]
    for rule in range(4):
        g, m, v = _step(rule, [neg_nan, 1.0], [1.0, 1.0], [0.0, neg_nan],
                        None if rule == fr.MOMENTUM else [1.0, 1.0])
        assert np.array_equal(g.view(np.uint32), [0x7FC00000] * 2)
        assert np.array_equal(m.view(np.uint32), [0x7FC00000] * 2)
        if v is not None:
            assert v.view(np.uint32)[0] == 0x7FC00000 and v[1] == v[1]


def test_adam_without_memory_is_a_sign_step():
    """beta1 = beta2 = 0, tau = 0: m' = d, v' = d^2, sqrt(fl(d^2)) = |d| in binary fp when d^2
    neither underflows nor overflows, so the step is exactly g +- lr."""
    rng = np.random.default_rng(0)
    eta = F(0.125)
    g0 = rng.standard_normal(1000).astype(F)
    a = (g0 + rng.standard_normal(1000).astype(F)).astype(F)
    d = a - g0
    keep = d != 0
    g, m, v = fr.server_opt_step(fr.ADAM, a[None], None, g0, np.zeros_like(g0),
                                 np.ones_like(g0), eta, 0.0, 0.0, 0.0)
    assert fr.same_bits(m, d) and fr.same_bits(v, d * d)
    assert fr.same_bits(g[keep], (g0 + eta * np.sign(d).astype(F))[keep])
    # d == 0: 0 / 0 is NaN, stored as the one quiet NaN
    g, _, _ = fr.server_opt_step(fr.ADAM, F([[1.0]]), None, F([1.0]), F([0.0]), F([1.0]),
                                 eta, 0.0, 0.0, 0.0)
    assert g.view(np.uint32)[0] == 0x7FC00000


def test_rows_mode_aggregate_is_the_fedavg_arithmetic():
    from oracle import fedavg_ref
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((5, 77)).astype(F)
    w = fedavg_ref.calculate_sample_weights([10, 11, 12, 13, 14])
    agg = fedavg_ref.weighted_average(rows, w)
    assert fr.same_bits(fr.weighted_sum(rows, w), agg)
    g0, m0 = rng.standard_normal(77).astype(F), rng.standard_normal(77).astype(F)
    v0 = rng.random(77).astype(F)
    before = [x.copy() for x in (rows, g0, m0, v0)]
    for rule in range(4):
        by_rows = fr.server_opt_step(rule, rows, w, g0, m0, v0, 0.1, 0.9, 0.99, 1e-3)
        single = fr.server_opt_step(rule, agg[None], None, g0, m0, v0, 0.1, 0.9, 0.99, 1e-3)
        for x, y in zip(by_rows, single):
            assert (x is None and y is None) or fr.same_bits(x, y)
    # the reference leaves its inputs alone
    assert all(fr.same_bits(x, y) for x, y in zip((rows, g0, m0, v0), before))


# ------------------------------------------------------------------ host-side validation
def test_entry_point_validates_on_the_host():
    """Bad arguments fail with a message before any launch (no device here).  The non-null
    pointers are host addresses: nothing dereferences them before the checks fail."""
    dummy = ctypes.addressof(ctypes.create_string_buffer(64))

    def step(rows=dummy, weights=dummy, C=2, P=8, g=dummy, m=dummy, v=dummy, rule=2, lr=0.1,
             b1=0.9, b2=0.99, tau=1e-3, stride=8):
        return _lib.call("fh_server_opt_step", rows, stride, None, weights, C, P, g, m, v, rule,
                         lr, b1, b2, tau, None)
    for rule in (-1, 4, 100):
        with pytest.raises(_lib.FedHipError, match=r"rule=.* outside \[0, 3\]"):
            step(rule=rule)
    for C in (0, -1):
        with pytest.raises(_lib.FedHipError, match="num_clients"):
            step(C=C)
    for C in (2, 33):
        with pytest.raises(_lib.FedHipError, match="no weights"):
            step(weights=None, C=C)
    with pytest.raises(_lib.FedHipError, match="bad sizes"):
        step(P=-1)
    for kw in ({"lr": float("inf")}, {"lr": float("nan")}, {"b1": float("nan")},
               {"b2": float("-inf")}, {"tau": float("inf")}, {"lr": 1e39}):
        with pytest.raises(_lib.FedHipError, match="non-finite"):
            step(**kw)
    with pytest.raises(_lib.FedHipError, match="negative"):
        step(tau=-1e-3)
    for kw in ({"rows": None}, {"g": None}, {"m": None}, {"v": None}, {"v": None, "rule": 1},
               {"v": None, "rule": 3}):
        with pytest.raises(_lib.FedHipError, match="null pointer"):
            step(**kw)
    # P == 0 is a no-op, whatever the pointers; FedAvgM needs no v
    assert step(P=0, rows=None, g=None, m=None, v=None) == 0
    assert step(P=0, rule=0, v=None, weights=None, C=1) == 0


def test_ops_binding_checks_the_vectors_before_the_call():
    """ops.server_opt_step refuses host tensors, and state vectors shorter than P."""
    rows, vec = torch.zeros(2, 8), torch.zeros(8)
    with pytest.raises(_lib.FedHipError, match="HIP device"):
        ops.server_opt_step(rows, vec, vec.clone(), vec.clone(), 2, 0.1, 0.9, 0.99, 1e-3)


def test_server_optimizer_constructor():
    with pytest.raises(ValueError, match="unknown"):
        fedopt.create_server_optimizer("fedsgd", server_lr=0.1)
    for bad in (4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="rule"):
            fedopt.ServerOptimizer(bad, 0.1)
    for kw in ({"server_lr": float("nan")}, {"server_lr": 1e39}, {"beta1": float("inf")},
               {"beta2": float("nan")}, {"tau": float("inf")}):
        with pytest.raises(ValueError, match="finite"):
            fedopt.ServerOptimizer(2, **{"server_lr": 0.1, **kw})
    with pytest.raises(ValueError, match="tau"):
        fedopt.FedAdam(0.1, tau=-1.0)
    with pytest.raises(ValueError, match="base"):
        fedopt.FedAdam(0.1, base=object())
    kinds = {"fedavgm": fedopt.FedAvgM, "fedadagrad": fedopt.FedAdagrad,
             "fedadam": fedopt.FedAdam, "fedyogi": fedopt.FedYogi}
    for rule, (kind, factory) in enumerate(kinds.items()):
        a = fedopt.create_server_optimizer(kind, server_lr=0.1, device="cpu")
        b = factory(0.1, device="cpu")
        assert a.rule == b.rule == rule and isinstance(a, fedopt.ServerOptimizer)
        assert (a.beta1, a.beta2, a.tau) == (float(F(0.9)), float(F(0.99)), float(F(1e-3)))
        assert type(a.base) is FedAvgAggregator and a.plain_base and a.m is None and a.v is None
    # scalars are rounded to fp32 once
    so = fedopt.ServerOptimizer("fedyogi", 0.1, beta1=0.7, beta2=0.3, tau=0.01, device="cpu")
    assert so.rule == 3 and so.server_lr == float(F(0.1)) != 0.1 and so.tau == float(F(0.01))
    assert fedopt.FedAdam(0.1, base=AdaptiveFedAvg(device="cpu")).plain_base
    for base in (robust.MedianAggregator(), robust.KrumAggregator(num_byzantine=1)):
        assert not fedopt.FedAdam(0.1, base=base).plain_base


def test_state_is_lazy_sized_once_and_round_trips():
    so = fedopt.FedAdam(0.1, tau=0.5, device="cpu")
    m, v = so._state(5, "cpu")
    assert m.tolist() == [0.0] * 5 and v.tolist() == [0.25] * 5
    with pytest.raises(FedAvgError, match="5 parameters"):
        so._state(6, "cpu")
    with pytest.raises(FedAvgError, match="aggregate"):
        so.step_vector(torch.zeros(3), torch.zeros(5))
    so.m.copy_(torch.arange(5.0))
    sd = so.state_dict()
    assert set(sd) == {"rule", "server_lr", "beta1", "beta2", "tau", "m", "v"}
    so.m.zero_()
    assert sd["m"].tolist() == [0, 1, 2, 3, 4]  # a copy
    other = fedopt.FedAvgM(1.0, device="cpu")
    other.load_state_dict(sd)
    assert other.rule == 2 and other.server_lr == so.server_lr and other.tau == 0.5
    assert other.m.tolist() == [0, 1, 2, 3, 4] and other.v.tolist() == [0.25] * 5
    other.reset()
    assert other.m is None and other.v is None
    assert other._state(7, "cpu")[1].tolist() == [0.25] * 7
    # FedAvgM keeps no second moment
    mo = fedopt.FedAvgM(1.0, device="cpu")
    assert mo._state(3, "cpu")[1] is None and mo.state_dict()["v"] is None
    fresh = fedopt.FedYogi(0.1, device="cpu")
    fresh.load_state_dict(fedopt.FedYogi(0.2, device="cpu").state_dict())  # no state yet
    assert fresh.m is None and fresh.server_lr == float(F(0.2))


def test_load_state_dict_errors():
    so = fedopt.FedAdam(0.1, device="cpu")
    so._state(4, "cpu")
    good = so.state_dict()
    for drop in good:
        with pytest.raises(FedAvgError, match="lacks"):
            so.load_state_dict({k: x for k, x in good.items() if k != drop})
    for key, bad, msg in (("rule", 7, "rule"), ("rule", "adam", "unknown"),
                          ("tau", -1.0, "tau"), ("beta1", float("nan"), "finite"),
                          ("v", None, "no v"), ("v", torch.zeros(5), "m's length"),
                          ("m", torch.zeros(4, dtype=torch.float64), "float32"),
                          ("m", torch.zeros(2, 2), "float32"), ("m", [0.0] * 4, "float32"),
                          ("m", None, "no m")):
        with pytest.raises(FedAvgError, match=msg):
            so.load_state_dict({**good, key: bad})
    # a failed load leaves the object as it was
    assert so.rule == 2 and so.m.numel() == 4 and so.tau == float(F(1e-3))


def test_step_packed_argument_errors_before_the_device():
    so = fedopt.FedAdam(0.1, device="cpu")
    g = torch.zeros(8)
    with pytest.raises(FedAvgError, match="No updates"):
        so.step_packed(torch.zeros(0, 8), [], g)
    with pytest.raises(FedAvgError, match="row_index"):
        so.step_packed(torch.zeros(6, 8), [10] * 5, g, row_index=[0, 1])
    with pytest.raises(FedAvgError, match="rows for"):
        so.step_packed(torch.zeros(6, 8), [10] * 5, g)


def test_rankround_refuses_a_robust_rule_given_twice():
    """Checked at construction, before the trainer (and the device) is touched."""
    from fedhip import round as fround
    so = fedopt.FedAdam(0.1, base=robust.MedianAggregator())
    with pytest.raises(_lib.FedHipError, match="ambiguous"):
        fround.RankRound(torch.nn.Linear(2, 2), [10, 10], [0],
                         aggregator=robust.MedianAggregator(), server_opt=so)


def test_rankround_refuses_a_robust_base_over_ranks_without_exact(monkeypatch):
    from fedhip import round as fround
    monkeypatch.setattr(fround.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(fround.dist, "get_world_size", lambda group=None: 2)
    so = fedopt.FedYogi(0.1, base=robust.MedianAggregator())
    with pytest.raises(_lib.FedHipError, match="exact=True"):
        fround.RankRound(torch.nn.Linear(2, 2), [10, 10], [0], group=object(), server_opt=so)
