"""tests/quantpack_ref.py, the host restatement of csrc/quantpack.hip, against the oracle's
quantiser (oracle/compress_ref.py) and against the reference itself
(tests/golden/quant_codes.json, written by tests/golden/make_quant_codes.py).  No GPU.

No tolerances: floats are compared by their int32 view."""
import json
import os

import numpy as np
import pytest

import quantpack_ref as qr
from oracle import compress_ref

F = np.float32
BITS = [1, 2, 3, 4, 8]
LENS = [1, 7, 8191, 8193, 300]
SEG = np.concatenate([[5], 5 + np.cumsum(LENS)]).tolist()
W = SEG[-1] + 9
NEG0 = np.array([0x80000000], np.uint32).view(F)[0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_codes.json")


def i32(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    return np.array_equal(i32(a), i32(b))


@pytest.mark.parametrize("bits,cw", [(1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (6, 8), (7, 8),
                                     (8, 8)])
def test_code_width_and_offsets(bits, cw):
    assert qr.code_width(bits) == cw
    bo, nb = qr.boff(SEG, bits), qr.seg_bytes(SEG, bits)
    assert nb == [-(-n * cw // 8) for n in LENS]
    assert bo[0] == 0 and all(o % 16 == 0 for o in bo)
    assert all(b - a >= n and b - a < n + 16 for a, b, n in zip(bo[:-1], bo[1:], nb))
    # a chunk of the segment plan starts on a 16-byte boundary of its segment's codes
    assert (8192 * cw // 8) % 16 == 0


@pytest.mark.parametrize("cw", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 15, 16, 17, 300, 8191, 8193])
def test_pack_and_unpack_are_inverse_on_the_codes(cw, n):
    rng = np.random.default_rng(n * 10 + cw)
    codes = rng.integers(0, 2 ** cw, size=n).astype(np.uint8)
    raw = qr.pack_codes(codes, cw)
    assert raw.size == -(-n * cw // 8)
    assert np.array_equal(qr.unpack_codes(raw, cw, n), codes)
    used = (n * cw) % 8
    if used:                      # the unused high bits of the last byte are zero
        assert raw[-1] >> used == 0
    # the position rule itself, element by element
    for j in {0, n // 2, n - 1}:
        assert (raw[(j * cw) // 8] >> ((j * cw) % 8)) & ((1 << cw) - 1) == codes[j]
    if used:                      # ... and the unpack does not look at them
        dirty = raw.copy()
        dirty[-1] |= (0xFF << used) & 0xFF
        assert np.array_equal(qr.unpack_codes(dirty, cw, n), codes)


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("bits", BITS)
def test_unpack_of_pack_is_the_oracles_dequantised_tensor(bits, symmetric):
    rng = np.random.default_rng(bits + 10 * symmetric)
    x = (rng.standard_normal((2, W)) * 0.05).astype(F)
    q = qr.quantize_rows(x, None, SEG, bits, symmetric)
    packed = qr.pack_rows(q["codes"], SEG, bits)
    assert packed.shape == (2, qr.boff(SEG, bits)[-1])
    assert np.array_equal(qr.unpack_code_rows(packed, SEG, bits, W)[:, SEG[0]:SEG[-1]],
                          q["codes"][:, SEG[0]:SEG[-1]])
    out = qr.unpack_rows(packed, q["scale"], q["zp"], q["passv"], None, SEG, bits,
                         np.zeros((2, W), F))
    for z in range(2):
        for s, (a, e) in enumerate(zip(SEG[:-1], SEG[1:])):
            v = x[z, a:e]
            if not symmetric and e - a == 1:     # constant: passed through, flagged
                assert q["zp"][z, s] == qr.INT64_MIN and same(out[z, a:e], v)
                continue
            codes, scale, zp = compress_ref.quantize(v, bits, symmetric)
            assert np.array_equal(q["codes"][z, a:e], codes)
            assert q["scale"][z, s] == scale and q["zp"][z, s] == zp
            assert same(out[z, a:e], compress_ref.dequantize(codes, scale, zp))
    assert not qr.validate(packed, q["scale"], q["zp"], q["passv"], SEG, bits).any()
    assert not out[:, :SEG[0]].any() and not out[:, SEG[-1]:].any()


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_all_zero_symmetric_segment_gives_minus_zero(bits):
    codes, scale, zp, pv, d = qr.quantize_segment(np.zeros(7, F), bits, True)
    assert scale == 0.0 and zp == (2 ** bits - 1) // 2 and not codes.any()
    assert np.array_equal(i32(d), i32(np.full(7, NEG0)))      # (0 - zp) * 0
    assert same(qr.dequant(qr.unpack_codes(qr.pack_codes(codes, qr.code_width(bits)),
                                           qr.code_width(bits), 7), scale, zp), d)


def test_pass_through_reproduces_a_constant_segment_with_both_zeros():
    v = np.array([0.0, -0.0, -0.0, 0.0, 0.0, -0.0, 0.0], F)
    for bits in BITS:
        codes, scale, zp, pv, d = qr.quantize_segment(v, bits, False)
        assert zp == qr.INT64_MIN and same(d, v)
        cw = qr.code_width(bits)
        back = qr.unpack_codes(qr.pack_codes(codes, cw), cw, v.size)
        assert same(qr.dequant(back, scale, zp, pv), v)
    c = np.full(5, F(-0.375))
    codes, scale, zp, pv, d = qr.quantize_segment(c, 8, False)
    assert zp == qr.INT64_MIN and codes.all() and same(d, c) and same(pv, c[0])


def test_validate_flags():
    bits = 3
    x = (np.random.default_rng(0).standard_normal((2, W)) * 0.05).astype(F)
    q = qr.quantize_rows(x, None, SEG, bits, False)
    packed = qr.pack_rows(q["codes"], SEG, bits)
    bo = qr.boff(SEG, bits)
    p = packed.copy()
    p[1, bo[2] + 10] |= 0x80                       # a code >= 8 in segment 2 of client 1
    p[0, bo[1] + 3] = 0xF0                         # element 7 of a 7-element segment: padding
    p[0, bo[1] + 4:bo[2]] = 0xFF                   # padding bytes
    want = np.zeros((2, len(LENS)), np.int32)
    want[1, 2] = 1
    assert np.array_equal(qr.validate(p, q["scale"], q["zp"], q["passv"], SEG, bits), want)
    for v in (np.nan, np.inf, -1.0):
        sc = q["scale"].copy()
        sc[0, 4] = v
        want = np.zeros((2, len(LENS)), np.int32)
        want[0, 4] = 1
        assert np.array_equal(qr.validate(packed, sc, q["zp"], q["passv"], SEG, bits), want)
    pv = q["passv"].copy()
    pv[1, 0], pv[1, 3] = np.inf, np.nan           # segment 0 is flagged, segment 3 is not
    want = np.zeros((2, len(LENS)), np.int32)
    want[1, 0] = 1
    assert np.array_equal(qr.validate(packed, q["scale"], q["zp"], pv, SEG, bits), want)


def test_fedavg_is_the_sequential_sum_over_the_unpacked_rows():
    rng = np.random.default_rng(3)
    base = (rng.integers(-256, 257, size=(1, W)) * 2.0 ** -10).astype(F)
    x = (base + (rng.standard_normal((3, W)) * 0.05).astype(F)).astype(F)
    q = qr.quantize_rows(x, base, SEG, 4, False)
    packed = qr.pack_rows(q["codes"], SEG, 4)
    rows = qr.unpack_rows(packed, q["scale"], q["zp"], q["passv"], base, SEG, 4, np.zeros((3, W), F))
    w = [0.3, 0.45, 0.25]
    start = rng.standard_normal(W).astype(F)
    got = qr.quant_fedavg(packed, q["scale"], q["zp"], q["passv"], w, base[0], SEG, 4, start,
                          row_index=[2, 0, 1], accumulate=True)
    acc = start.copy()
    for r, wk in zip([2, 0, 1], w):
        acc = (acc + (F(wk) * rows[r]).astype(F)).astype(F)
    a, e = SEG[0], SEG[-1]
    assert same(got[a:e], acc[a:e]) and same(got[:a], start[:a]) and same(got[e:], start[e:])


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_covers_what_it_should():
    g = _golden()
    names = set(g["cases"])
    for n in (1, 7, 300):
        for bits in BITS:
            assert f"n{n}_b{bits}_sym" in names
            assert (f"n{n}_b{bits}_asym" in names) == (n > 1)
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("name", sorted(_golden()["cases"]))
def test_helper_reproduces_the_reference(name):
    g = _golden()
    c = g["cases"][name]
    x = np.array(g["inputs_u32"][str(c["numel"])], np.uint32).view(F)
    codes, scale, zp, pv, d = qr.quantize_segment(x, c["bits"], c["symmetric"])
    assert np.array_equal(codes, np.array(c["codes"], np.uint8))
    assert float(scale).hex() == c["scale_hex"] and int(zp) == c["zero_point"]
    assert np.array_equal(d.view(np.uint32), np.array(c["dense_u32"], np.uint32))
    # through the packed form: nothing is lost
    cw = qr.code_width(c["bits"])
    back = qr.unpack_codes(qr.pack_codes(codes, cw), cw, x.size)
    assert np.array_equal(qr.dequant(back, scale, zp).view(np.uint32),
                          np.array(c["dense_u32"], np.uint32))
