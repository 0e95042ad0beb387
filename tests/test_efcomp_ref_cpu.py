"""tests/efcomp_ref.py against itself, on inputs where fp32 arithmetic is exact or the property
is one of the definition: the telescoping identity of error feedback, the two-neighbour rule
and the range of stochastic rounding, and its unbiasedness against a derived bound (which the
deterministic quantiser misses).  CPU only; tests/test_efcomp_gpu.py holds the device to the
same restatement bit for bit."""
import numpy as np

import efcomp_ref as er
from oracle import compress_ref

F = np.float32
SEG = [3, 4, 11, 1011, 1411]   # a lead of 3, segments of 1, 7, 1000 and 400 elements


def int_rows(rng, shape, bound):
    return rng.integers(-bound + 1, bound, size=shape).astype(F)


def test_error_feedback_telescopes_and_plain_topk_does_not():
    """R = 4 rounds of integer deltas, |delta| < 2^10: everything stays an integer below 2^24,
    so fp32 is exact and  sum_t sent_t + resid_R == sum_t delta_t  holds bit for bit.  Without
    the residual the same sum is short somewhere (ratio 0.9 drops 90 %)."""
    rng = np.random.default_rng(1)
    C, W, R, ratio = 3, SEG[-1] + 5, 4, 0.9
    a, e = SEG[0], SEG[-1]
    base = int_rows(rng, (1, W), 1 << 12)
    resid = np.zeros((C, W), F)
    total = np.zeros((C, W), np.float64)
    sent = np.zeros((C, W), np.float64)
    sent_plain = np.zeros((C, W), np.float64)
    for _ in range(R):
        delta = int_rows(rng, (C, W), 1 << 10)
        x = (base + delta).astype(F)
        x_out, resid, keep, v = er.ef_topk_round(x, base, resid, SEG, ratio)
        assert np.array_equal(x_out[:, :a], x[:, :a]) and np.array_equal(x_out[:, e:], x[:, e:])
        total += delta
        sent += x_out.astype(np.float64) - base
        for z in range(C):
            for s0, s1 in zip(SEG[:-1], SEG[1:]):
                sent_plain[z, s0:s1] += compress_ref.topk_dense(delta[z, s0:s1], ratio)
    assert np.array_equal((sent + resid)[:, a:e], total[:, a:e])
    assert not resid[:, :a].any() and not resid[:, e:].any()
    assert (sent_plain[:, a:e] != total[:, a:e]).any()
    assert np.abs(resid).max() > 0          # the identity is not trivially 0 == 0


def test_fold_and_finish_definitions():
    v = er.fold(F([1.5, -2.0, 3.0]), F([0.5, 1.0, -1.0]), F([0.25, 0.0, -4.0]))
    assert np.array_equal(v, F([1.25, -3.0, 0.0]))
    x_out, r = er.topk_finish(F([10, 20, -0.0]), F([1, -2, 3]), np.array([1, 0, 0], np.uint8))
    assert np.array_equal(x_out.view(np.uint32), F([11, 20, 0.0]).view(np.uint32))
    assert np.array_equal(r.view(np.uint32), F([0.0, -2, 3]).view(np.uint32))
    x_out, r = er.quant_finish(F([10, 20]), F([1.5, -2]), F([1.0, -2.5]))
    assert np.array_equal(x_out, F([11, 17.5])) and np.array_equal(r, F([0.5, 0.5]))


def test_stochastic_rounding_takes_a_neighbour():
    rng = np.random.default_rng(2)
    v = (rng.standard_normal(5000) * 0.3).astype(F)
    r = rng.integers(0, 1 << 32, size=v.size, dtype=np.uint64).astype(np.uint32)
    for bits in (2, 4, 8, 16):
        for sym in (True, False):
            g = er.squant_segment(v, r, bits, sym)
            fl = np.floor(g["t"]).astype(np.int64)
            lo_q, hi_q = (-(2 ** (bits - 1) - 1), 2 ** (bits - 1) - 1) if sym else (0, 2 ** bits - 1)
            down, up = np.clip(fl, lo_q, hi_q), np.clip(fl + 1, lo_q, hi_q)
            assert ((g["q"] == down) | (g["q"] == up)).all()
            assert (g["q"] == down).any() and (g["q"] == up).any()
            assert g["q"].min() >= lo_q and g["q"].max() <= hi_q
            if bits <= 8:
                assert np.array_equal(g["codes"].astype(np.int64), g["q"] + (hi_q if sym else 0))


def test_grid_points_never_move():
    """scale is a power of two and every value a multiple of it: t is an integer, the
    threshold is 0 and no random word rounds up."""
    for bits, sym in ((4, True), (8, True), (4, False), (8, False)):
        top = 2 ** (bits - 1) - 1 if sym else 2 ** bits - 1
        k = np.arange(-top, top + 1) if sym else np.arange(0, top + 1)
        v = (k * 0.125).astype(F) + (F(0.0) if sym else F(3.0))
        for r in (np.zeros(v.size, np.uint32), np.full(v.size, 0xFFFFFFFF, np.uint32)):
            g = er.squant_segment(v, r, bits, sym)
            assert float(g["scale"]) == 0.125
            assert np.array_equal(g["deq"].view(np.uint32), v.view(np.uint32))
            assert np.array_equal(g["q"], k)


def test_codes_stay_in_range_when_the_top_rounds_above_qmax():
    """a / fl32(a / qmax) can round above qmax; with the smallest random word such an element
    would round up to qmax + 1 if it were not clamped."""
    qmax = 7
    rng = np.random.default_rng(3)
    cand = (rng.random(20000).astype(F) + F(0.5))
    t_top = (cand / (cand / F(qmax)).astype(F)).astype(F)
    hit = cand[t_top > qmax]
    assert hit.size > 0
    a = hit[0]
    v = np.array([a, -a, a / 2, 0.0], F)
    g = er.squant_segment(v, np.zeros(4, np.uint32), 4, True)
    assert g["t"][0] > qmax and g["t"][1] < -qmax
    assert g["q"][0] == qmax and g["q"][1] >= -qmax
    assert g["codes"].max() <= 2 * qmax


def test_constant_segments_pass_through():
    r = np.zeros(6, np.uint32)
    z = er.squant_segment(np.zeros(6, F), r, 4, True)
    assert float(z["scale"]) == 0 and not z["deq"].any() and not z["codes"].any()
    c = er.squant_segment(np.full(6, 2.5, F), r, 4, False)
    assert float(c["scale"]) == 0 and (c["deq"] == 2.5).all() and not c["codes"].any()
    one = er.squant_segment(F([-3.0]), r[:1], 8, False)
    assert float(one["scale"]) == 0 and one["deq"][0] == -3.0


def test_words_follow_the_philox_layout():
    import philox_ref
    w = er.squant_words(77, 9, np.arange(5, 14))
    blk = philox_ref.philox4x32_10(77, 9 | (1 << 62), np.array([1, 2, 3], np.uint64))
    flat = np.stack(blk, axis=-1).reshape(-1)      # counters 1..3 = elements 4..15
    assert np.array_equal(w, flat[1:10])
    assert not np.array_equal(w, er.squant_words(77, 10, np.arange(5, 14)))


def unbiased_mean(run):
    """float64 mean over the fixed keys of run(key) -> deq [n]."""
    acc = np.zeros(er.UNBIASED_N, np.float64)
    for key in er.UNBIASED_KEYS:
        acc += run(key)
    return acc / len(er.UNBIASED_KEYS)


def test_stochastic_rounding_is_unbiased_and_round_to_nearest_is_not():
    v = er.unbiased_vector()
    idx = np.arange(v.size)
    bits = er.UNBIASED_BITS
    scale = er.squant_segment(v, np.zeros(v.size, np.uint32), bits, True)["scale"]
    bound = er.unbiased_bound(v, scale)
    assert len(set(er.UNBIASED_KEYS)) == er.UNBIASED_KEYS_N

    def run(key):
        return er.squant_segment(v, er.squant_words(key, er.UNBIASED_ID, idx), bits, True)["deq"]
    err = np.abs(unbiased_mean(run) - v)
    print("max |mean - v| / scale =", err.max() / float(scale), "bound / scale =",
          bound / float(scale))
    assert err.max() <= bound
    det = er.quant_dense(v, bits, True)
    assert np.abs(det.astype(np.float64) - v).max() > bound
