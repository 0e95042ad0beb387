"""Pins tests/dpfedavg_ref.py, the numpy reference the GPU tests of central DP-FedAvg compare
against: a hand-computed case, an independent fp64 formulation, the clip update, the z_delta
identity, the accountant, and deliberately wrong variants that the comparison must notice.
CPU tier: no GPU, no kernel."""
import math
import os
import re

import numpy as np
import pytest

import dpfedavg_ref as dr
import philox_ref as pr
from src.aggregation import dpfedavg

F = np.float32


def fx(h):
    return F(float.fromhex(h))


# ---------------------------------------------------------------- the hand-computed case
# g = (1, -2, 1/2, 4); the deltas are exact in fp32, so are x = g + d and fl32(x - g) = d:
#   d_0 = (3, 4, 0, 0)      n_0 = 5      > C = 5/2:  b = 0, c = 1/2
#   d_1 = (0, 0, 3/2, 2)    n_1 = 5/2   <= C      :  b = 1, c = 1
#   d_2 = (1, 2, 2, 4)      n_2 = 5      > C      :  b = 0, c = 1/2
# m = 3:  W = fl32(1/3) = 11184811 * 2^-25 = 0x1.555556p-2;  s = (W/2, W, W/2), exact halvings.
# Products and sums below, each rounded to 24 bits, nearest even; 3W = 2^25+1 units of 2^-25:
#   j=0: p = W/2*3 = (2^25+1)*2^-26 -> 1/2 (the 1 is below half an ulp); + 0; + W/2*1:
#        1/2 + W/2 = 44739243*2^-26 -> 11184811*2^-24 = 2W                       acc = 0x1.555556p-1
#   j=1: p = W/2*4 = 2W; + 0; + W/2*2 = W:  2W + W = 3W = (2^25+1)*2^-25 -> 1    acc = 1
#   j=2: 0; + W*3/2 = (2^25+1)*2^-26 -> 1/2; + W/2*2 = W:
#        1/2 + W = 27962027*2^-25 -> 13981014*2^-24 (tie .5 -> even)              acc = 0x1.aaaaacp-1
#   j=3: 0; + W*2 = 2W; + W/2*4 = 2W:  4W exact                                   acc = 0x1.555556p+0
# noise nu = (1/4, -1/2, 0, 1):  t = fl32(acc + nu), out = fl32(g + t):
#   j=0: t = 2W + 1/4 = 0x1.d55556p-1 (exact);  1 + t = 0x1.eaaaabp+0 -> tie -> 0x1.eaaaacp+0
#   j=1: t = 1 - 1/2 = 1/2;                    -2 + 1/2 = -3/2
#   j=2: t = acc;                              1/2 + 0x1.aaaaacp-1 = 0x1.555556p+0 (exact)
#   j=3: t = 4W + 1 = 0x1.2aaaabp+1 -> tie -> 0x1.2aaaacp+1;  4 + t = 0x1.955556p+2 (exact)
G = np.array([1, -2, 0.5, 4], dtype=F)
D = np.array([[3, 4, 0, 0], [0, 0, 1.5, 2], [1, 2, 2, 4]], dtype=F)
NU = np.array([0.25, -0.5, 0, 1], dtype=F)
W = fx("0x1.555556p-2")
HAND_S = np.array([fx("0x1.555556p-3"), W, fx("0x1.555556p-3")], dtype=F)
HAND_ACC = np.array([fx("0x1.555556p-1"), F(1), fx("0x1.aaaaacp-1"), fx("0x1.555556p+0")], dtype=F)
HAND_OUT = np.array([fx("0x1.eaaaacp+0"), F(-1.5), fx("0x1.555556p+0"), fx("0x1.955556p+2")],
                    dtype=F)


def test_hand_computed_three_clients_four_coordinates():
    X = G + D
    assert dr.same_bits(X - G, D)
    assert W == F(1) / F(3) and int(W.view(np.uint32)) == 0x3EAAAAAB
    sq = dr.sqnorms(X, G)
    assert sq.tolist() == [25.0, 6.25, 25.0]
    bits, s = dr.clip_coef(sq, 2.5, 3)
    assert bits.tolist() == [0, 1, 0]
    assert dr.same_bits(s, HAND_S)
    assert dr.same_bits(dr.clipped_sum(X, s, G, add_global=False), HAND_ACC)
    assert dr.same_bits(dr.clipped_sum(D, s), HAND_ACC)          # delta mode, no g
    assert dr.same_bits(dr.clipped_sum(X, s, G, noise=NU), HAND_OUT)
    # the single-row finish on the partial: 0 + 1*acc = acc, then the same noise and g
    one = np.ones(1, dtype=F)
    assert dr.same_bits(dr.clipped_sum(HAND_ACC[None], one, G, noise=NU, rows_are_deltas=True),
                        HAND_OUT)
    # sigma_avg = fl32(z * C / m) = fl32(1.2 * 2.5 / 3) = fl32(1.0000000000000002) = 1
    assert dr.sigma_avg(1.2, 2.5, 3) == F(1.0)
    # the fused step: one of three clients is under the clip norm, no bit noise:
    # C' = 2.5 * exp(-0.2 * (1/3 - 0.5))
    st = dr.step(X, G, 2.5, 3, z=0.0, gamma=0.5, eta=0.2, sigma_b=0.0, seed=1, noise=NU)
    assert dr.same_bits(st["out"], HAND_OUT) and st["bbar"] == 1 / 3
    assert st["clip_next"] == 2.5 * math.exp(-0.2 * (1 / 3 - 0.5))
    # a zero delta row: n = 0 gives c = 1, b = 1; a NaN row: b = 0, c = 1 (and a NaN sum)
    bits0, s0 = dr.clip_coef(np.array([0.0, np.nan]), 2.5, 3)
    assert bits0.tolist() == [1, 0] and dr.same_bits(s0, np.array([W, W]))


def _seeded(C, P, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P).astype(F)
    mag = 10.0 ** rng.uniform(-1.5 * spread, 0.0, (C, 1))
    rows = (g + mag * 0.1 * rng.standard_normal((C, P))).astype(F)
    return rows, g


def test_independent_fp64_formulation_agrees_within_the_rounding_bound():
    """fp64 throughout (coefficient, weight, products, sum) from the same fp32 deltas: the fp32
    reference rounds c, 1/m, their product and each term once (4 roundings per term) and the
    running sum m - 1 times (0 + p is exact): (m + 3) * 2^-24 * sum_k |s_k d_kj| to first
    order."""
    for C, P, seed in ((3, 257, 1), (8, 1001, 2), (33, 513, 3)):
        rows, g = _seeded(C, P, seed)
        d = (rows - g).astype(np.float64)
        n = np.sqrt((d * d).sum(axis=1))
        clip = float(np.median(n))
        s64 = np.minimum(1.0, clip / n) / C
        want = (s64[:, None] * d).sum(axis=0)
        bound = (C + 3) * 2.0 ** -24 * (np.abs(s64[:, None] * d)).sum(axis=0)
        _, s = dr.clip_coef(dr.sqnorms(rows, g), clip, C)
        got = dr.clipped_sum(rows, s, g, add_global=False).astype(np.float64)
        assert 0 < (n <= clip).sum() < C
        assert (np.abs(got - want) <= bound).all(), (C, P)
        # and the exact norm against the plain fp64 one
        assert np.allclose(dr.sqnorms(rows, g), n * n, rtol=P * 2.0 ** -53, atol=0)


def test_clip_update_on_both_sides_of_the_quantile():
    C0, gamma, eta, m = 1.75, 0.3, 0.2, 10
    # all clipped: sum b = 0, bbar = 0: the norm rises by exactly exp(eta * gamma)
    bbar, up = dr.clip_update(C0, 0, m, gamma, eta, 0.0, seed=5)
    assert bbar == 0.0 and up == C0 * math.exp(eta * gamma) and up > C0
    # none clipped: bbar = 1: it falls by exp(-eta * (1 - gamma))
    bbar, down = dr.clip_update(C0, m, m, gamma, eta, 0.0, seed=5)
    assert bbar == 1.0 and down == C0 * math.exp(-eta * (1 - gamma)) and down < C0
    # eta = 0: unchanged, whatever the bits and the bit noise; no draw
    assert dr.clip_update(C0, 3, m, gamma, 0.0, 7.0, seed=5) == (0.3, C0)
    # bit noise: the draw is lane 0 of counter 0 under the bit stream word
    xi = float(pr.gauss4(5, (1 << 64) - 2, 0)[0])
    bbar, nxt = dr.clip_update(C0, 4, m, gamma, eta, 0.5, seed=5)
    assert bbar == (4 + 0.5 * xi) / m and nxt == C0 * math.exp(-eta * (bbar - gamma))
    assert xi != float(pr.gauss4(5, (1 << 64) - 1, 0)[0])  # not the aggregate's stream
    assert xi != float(pr.gauss4(6, (1 << 64) - 2, 0)[0])  # and keyed by the round


def test_z_delta_identity_and_refusal():
    for z, sb in ((1.0, 0.6), (1.1, 5.0), (4.0, 2.5), (0.5, 50.0)):
        zd = dr.z_delta(z, 0.2, sb)
        assert zd > z
        assert math.isclose(zd ** -2 + (2 * sb) ** -2, z ** -2, rel_tol=1e-14)
        assert math.isclose(dpfedavg.delta_noise_multiplier(z, sb), zd, rel_tol=1e-15)
        assert dr.z_delta(z, 0.0, sb) == z  # a fixed clip norm spends nothing on the count
    assert dr.z_delta(0.0, 0.2, 0.0) == 0.0 and dpfedavg.delta_noise_multiplier(0.0, 0.0) == 0.0
    for z, sb in ((1.0, 0.5), (1.0, 0.25), (2.0, 0.0)):
        with pytest.raises(ValueError):
            dr.z_delta(z, 0.2, sb)
        with pytest.raises(ValueError):
            dpfedavg.delta_noise_multiplier(z, sb)
        with pytest.raises(ValueError):
            dpfedavg.CentralDPConfig(z, 1.0, bit_noise=sb)
        dpfedavg.CentralDPConfig(z, 1.0, bit_noise=sb, clip_lr=0.0)  # fixed norm: no count
    # bit_noise None: m / 20 when the norm adapts
    cfg = dpfedavg.CentralDPConfig(1.0, 1.0)
    assert cfg.resolve(100) == (dr.z_delta(1.0, 0.2, 5.0), 5.0)
    with pytest.raises(ValueError):
        cfg.resolve(10)  # 2 * 10 / 20 = 1 <= z
    assert dpfedavg.CentralDPConfig(1.0, 1.0, clip_lr=0.0).resolve(10) == (1.0, 0.0)
    for bad in (dict(noise_multiplier=-1.0, clip_norm=1.0), dict(noise_multiplier=1.0, clip_norm=0.0),
                dict(noise_multiplier=1.0, clip_norm=float("inf")),
                dict(noise_multiplier=1.0, clip_norm=1.0, target_quantile=1.5),
                dict(noise_multiplier=1.0, clip_norm=1.0, clip_lr=-0.1)):
        with pytest.raises(ValueError):
            dpfedavg.CentralDPConfig(**bad)


@pytest.mark.parametrize("z,T,delta", [(1.0, 1, 1e-5), (1.1, 100, 1e-5), (4.0, 1000, 1e-6)])
def test_gaussian_epsilon_is_the_minimum_over_the_renyi_orders(z, T, delta):
    alpha = 1.0 + np.linspace(1e-4, 40.0, 4_000_001)
    grid = float((T * alpha / (2 * z * z) + math.log(1 / delta) / (alpha - 1)).min())
    for eps in (dr.gaussian_epsilon(z, T, delta), dpfedavg.gaussian_epsilon(z, T, delta)):
        assert eps <= grid                       # never above the grid minimum
        assert grid - eps <= 1e-6 * grid         # and within 1e-6 relative below it
    assert dr.gaussian_epsilon(z, T, delta) == dpfedavg.gaussian_epsilon(z, T, delta)
    with pytest.raises(ValueError):
        dpfedavg.gaussian_epsilon(0.0, T, delta)
    with pytest.raises(ValueError):
        dpfedavg.gaussian_epsilon(z, T, 1.0)


def test_wrong_variants_are_noticed():
    C, P = 5, 1001
    rows, g = _seeded(C, P, 9)
    sq = dr.sqnorms(rows, g)
    clip = float(np.median(np.sqrt(sq)))
    bits, s = dr.clip_coef(sq, clip, C)
    noise = (0.01 * np.random.default_rng(10).standard_normal(P)).astype(F)
    want = dr.clipped_sum(rows, s, g, noise=noise)
    assert dr.same_bits(want, dr.clipped_sum(rows, s, g, noise=noise))
    for wrong in ("fma", "reverse", "noise_first"):
        assert not dr.same_bits(want, dr.clipped_sum(rows, s, g, noise=noise, wrong=wrong)), wrong
    # the clip applied after the weight: c * (w * d) instead of (c * w) * d
    n = np.sqrt(sq)
    c = np.where(n > clip, clip / n, 1.0).astype(F)
    assert dr.same_bits(s, c * (F(1) / F(C)))
    assert not dr.same_bits(dr.clipped_sum(rows, s, g), dr.clip_after_weight_sum(rows, c, C, g))
    # the noise: another stream word, another seed, a rotated lane
    G0 = dr.gauss(77, P)
    assert np.array_equal(G0, pr.gauss_row(77, (1 << 64) - 1, P))
    assert not np.array_equal(G0, pr.gauss_row(77, (1 << 64) - 2, P))
    assert not np.array_equal(G0, pr.gauss_row(78, (1 << 64) - 1, P))
    assert not np.array_equal(G0, pr.gauss_row(77, (1 << 64) - 1, P, lane_rot=1))
    # the round key is RankRound's
    assert dr.round_key(5, 3, 1) == dpfedavg.round_key(5, 3, 1) \
        == (5 * 6364136223846793005 + 3 * 1442695040888963407 + 1) % (1 << 64)


def test_ops_constants_are_the_headers():
    """fedhip.ops restates the FH_DPFA_* defines of include/fedhip.h (state slots, stream words,
    flags): parsed here so the two cannot drift."""
    from fedhip import ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "fedhip.h")).read()
    defs = {k: int(v.rstrip("uUlL"), 0)
            for k, v in re.findall(r"^#define\s+FH_(DPFA_\w+)\s+(0[xX][0-9a-fA-F]+[uUlL]*|\d+)\b",
                                   src, flags=re.M)}
    assert len(defs) == 11, sorted(defs)
    for name, value in defs.items():
        assert getattr(ops, name) == value, name
    assert {n for n in dir(ops) if n.startswith("DPFA_")} == set(defs)
    assert (ops.DPFA_STREAM_NOISE, ops.DPFA_STREAM_BIT) == (dr.STREAM_NOISE, dr.STREAM_BIT)
