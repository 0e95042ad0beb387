"""tests/philox_ref.py pinned on the CPU: the published Random123 philox4x32_10 known-answer
vectors, the end points of u01, gauss4 finite everywhere, the key-block rules, and the
DISCRIMINATING POWER of a comparison against it.

Discriminating power: the project's code is never altered; the reference takes test-only
parameters that build a wrong generator (9 rounds, counter halves swapped, counter + 1, lanes
rotated by one, the seed cut to 32 bits).  Each wrong generator must differ from the true one
by more than TEN times the Gaussian tolerance of tests/test_philox_streams_gpu.py (per unit
sigma; the factor covers the consumers' own roundings that those comparisons also allow) on at
least 99 % of the elements, and on at least 25 % of the keep-mask bits at p = 0.5 (two
independent fair masks differ on 50 %).  So a kernel with one of these defects fails the GPU
comparisons, which allow no exception at all."""
import numpy as np
import pytest

import philox_ref as pr

SEED = (0x5EED << 32) | 0x1234ABCD  # >= 2^32: the 32-bit cut changes it
ROW = (7 << 32) | 3

# (counter words c0..c3, key words k0 k1) -> output words; Random123 kat_vectors, philox4x32 10
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

# What a GPU comparison allows per unit sigma: GAUSS_TOL plus the consumer's own roundings,
# 2^-24 of operands that reach a few units over a noise scale of 0.28 or more in those tests
# (a few 1e-6) -- 10 GAUSS_TOL is above all of it.
NOTICED = 10.0 * pr.GAUSS_TOL

PERTURBATIONS = [dict(rounds=9), dict(swap_halves=True), dict(lo_offset=1), dict(lane_rot=1),
                 dict(seed_bits=32)]


def _pack(ctr, key):
    return key[0] | (key[1] << 32), ctr[2] | (ctr[3] << 32), ctr[0] | (ctr[1] << 32)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_published_known_answers(ctr, key, want):
    seed, hi, lo = _pack(ctr, key)
    got = pr.philox4x32_10(seed, hi, lo)
    assert all(r.dtype == np.uint32 for r in got)
    assert tuple(int(r) for r in got) == want


def test_known_answers_vectorised():
    """The three vectors in one call: broadcasting does not mix the lanes of different counters."""
    seeds, his, los = zip(*(_pack(c, k) for c, k, _ in KAT))
    got = pr.philox4x32_10(np.array(seeds, dtype=np.uint64), np.array(his, dtype=np.uint64),
                           np.array(los, dtype=np.uint64))
    for w in range(4):
        assert [int(v) for v in got[w]] == [k[2][w] for k in KAT]


def test_u01_end_points():
    assert pr.u01(np.uint32(0)) == 2.0 ** -24
    assert pr.u01(np.uint32(0xFFFFFFFF)) == 1.0
    assert pr.u01(np.uint32(0xFF)) == 2.0 ** -24 and pr.u01(np.uint32(0x100)) == 2.0 ** -23
    x = np.arange(0, 1 << 32, 65537, dtype=np.uint64).astype(np.uint32)
    u = pr.u01(x)
    assert u.min() > 0.0 and u.max() <= 1.0
    assert np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))  # multiples of 2^-24: exact


def test_gauss4_finite_on_a_sweep():
    n = 1 << 22
    g = pr.gauss4(SEED, ROW, np.arange(n // 4, dtype=np.uint64))
    assert g.shape == (n // 4, 4) and np.isfinite(g).all()
    assert np.abs(g).max() <= pr.R_MAX
    assert abs(g.mean()) < 5.0 / np.sqrt(n) and abs(g.std() - 1.0) < 5.0 / np.sqrt(2 * n)
    # the largest radius the generator can produce at all: u01 = 2^-24
    assert np.isclose(np.sqrt(-2.0 * np.log(pr.u01(np.uint32(0)))), pr.R_MAX)


def test_gauss_row_is_lane_j_mod_4_of_counter_j_div_4():
    g4 = pr.gauss4(SEED, ROW, np.arange(3, dtype=np.uint64))
    for n in (1, 5, 6, 7, 12):
        row = pr.gauss_row(SEED, ROW, n)
        assert row.shape == (n,)
        assert all(row[j] == g4[j // 4, j % 4] for j in range(n))


def test_tolerance_figure():
    """The derived bound: about 1e-5 per unit sigma, and far above the error of an fp32
    evaluation with correctly rounded steps (numpy), far below the size of a draw."""
    assert 9e-6 < pr.GAUSS_TOL < 1.2e-5
    r0, r1, _, _ = pr.philox4x32_10(SEED, ROW, np.arange(1 << 18, dtype=np.uint64))
    u1, u2 = pr.u01(r0).astype(np.float32), pr.u01(r1).astype(np.float32)
    g32 = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.2831853071795864) * u2)
    g64 = pr.gauss4(SEED, ROW, np.arange(1 << 18, dtype=np.uint64))[:, 0]
    assert g32.dtype == np.float32
    assert np.abs(g32.astype(np.float64) - g64).max() <= pr.GAUSS_TOL


def test_key_block_rules():
    assert pr.row_key(None, 5) == 5
    blk = pr.key_block(17)
    assert blk.dtype == np.uint64 and list(blk) == [17, 0]
    assert pr.row_key(blk, 2) == 2 and pr.effective_seed(4, blk) == 21
    big = (1 << 32) | 5
    blk = pr.key_block((1 << 64) - 3, [9, big, 5])
    assert [pr.row_key(blk, z) for z in range(3)] == [9, big, 5]
    assert pr.effective_seed(10, blk) == 7          # wraps mod 2^64
    assert pr.effective_seed((1 << 64) + 4) == 4    # the C ABI takes 64 bits
    assert pr.effective_seed(-1) == (1 << 64) - 1


def test_crop_flip_ranges_and_formula():
    b = np.arange(4096)
    d = pr.crop_flip(SEED, ROW, b, 4)
    assert d.dtype == np.uint8 and d.shape == (4096, 3)
    assert d[:, :2].max() == 8 and d[:, :2].min() == 0 and set(d[:, 2]) == {0, 1}
    r0, r1, r2, _ = pr.philox4x32_10(SEED, ROW, b)
    assert [int(v) for v in d[:5, 0]] == [(int(r) * 9) >> 32 for r in r0[:5]]
    assert [int(v) for v in d[:5, 1]] == [(int(r) * 9) >> 32 for r in r1[:5]]
    assert [int(v) for v in d[:5, 2]] == [int(r) >> 31 for r in r2[:5]]
    assert not pr.crop_flip(SEED, ROW, b, 0)[:, :2].any()  # no padding: no offset


def test_keep_mask_threshold():
    """u01 <= 1 - p on the 2^-24 grid: p = 0.5 keeps exactly the words below 2^31."""
    r0 = pr.philox4x32_10(SEED, ROW, np.arange(4096, dtype=np.uint64))[0]
    assert np.array_equal(pr.keep_mask(SEED, ROW, 4096, 0.5), (r0 < (1 << 31)).astype(np.uint8))
    assert pr.keep_mask(SEED, ROW, 4096, 0.0).all()
    for p in (0.25, 0.3):
        assert abs(pr.keep_mask(SEED, ROW, 1 << 16, p).mean() - (1 - p)) < 0.01


@pytest.mark.parametrize("kw", PERTURBATIONS, ids=lambda k: next(iter(k)))
def test_a_wrong_generator_is_noticed(kw):
    n = 1 << 16
    good, bad = pr.gauss_row(SEED, ROW, n), pr.gauss_row(SEED, ROW, n, **kw)
    assert (np.abs(good - bad) > NOTICED).mean() >= 0.99
    mg, mb = pr.keep_mask(SEED, ROW, n, 0.5), pr.keep_mask(SEED, ROW, n, 0.5, **kw)
    assert (mg != mb).mean() >= 0.25
    # and at the odd lengths the GPU tests use: the tail draws are wrong too
    for m in (1, 5, 6, 7):
        assert (np.abs(good[:m] - bad[:m]) > NOTICED).all()


def test_the_true_generator_is_not_noticed():
    n = 1 << 12
    assert np.array_equal(pr.gauss_row(SEED, ROW, n), pr.gauss_row(SEED, ROW, n, rounds=10))
    assert np.array_equal(pr.gauss_row(5, ROW, n), pr.gauss_row(5, ROW, n, seed_bits=32))


def test_high_words_select_other_streams():
    """The same low words with and without high words: seed, row and counter each."""
    n = 4096
    base = pr.gauss_row(0x1234, 7, n)
    assert (np.abs(base - pr.gauss_row((5 << 32) | 0x1234, 7, n)) > pr.GAUSS_TOL).mean() >= 0.99
    assert (np.abs(base - pr.gauss_row(0x1234, (3 << 32) | 7, n)) > pr.GAUSS_TOL).mean() >= 0.99
    lo = np.arange(64, dtype=np.uint64)
    a, b = pr.philox4x32_10(1, 2, lo), pr.philox4x32_10(1, 2, lo + np.uint64(1 << 32))
    assert all((x != y).mean() > 0.9 for x, y in zip(a, b))
