"""Case builders for the compression edge tests (csrc/compress.hip) — pure numpy, no GPU.

Top-k: segments whose top-k cut falls inside a tie at the threshold magnitude T, with
the tied elements placed where the apply kernel's three rank computations meet their
edges (wave, 256-element pass, 8192-element chunk), plus decoys that share T's low key
byte or its 24-bit prefix but not both.  Quantiser: inputs whose scaled values sit
exactly on halves (the rounding rule), degenerate segments, a zero point that is not
an fp32 integer, and the bit widths at both ends of the accepted range.

Every builder returns the input together with the facts the case is built to have;
tests/test_compress_cases_cpu.py asserts those facts from the data alone, so the GPU
test (tests/test_compress_edges_gpu.py) cannot go vacuous when a builder is edited.
"""
from __future__ import annotations

import numpy as np

CHUNK = 8192     # fh_compress_chunk_elems(): elements per workgroup
PASS = 256       # elements per pass of a workgroup (one per thread)
WAVE = 64
N3 = 3 * CHUNK + 100  # four chunks, the last one ragged

# 0.3f = 0x3E99999A: low key byte 0x9A, neither 0x00 nor 0xFF, so nextafter() in either
# direction keeps the 24-bit prefix; 2T and T/2 change only the exponent.
T_DEFAULT = np.float32(0.3)


def topk_k(numel: int, sparsity_ratio: float) -> int:
    """k = int(n * (1 - ratio)), at least 1 (as oracle/compress_ref.topk_k)."""
    r = max(0.0, min(1.0, sparsity_ratio))
    k = int(numel * (1 - r))
    return 1 if k == 0 else k


def key_of(v) -> np.ndarray:
    """The kernel's 31-bit magnitude key."""
    return np.asarray(v, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def where_of(idx):
    """(chunk, pass within the chunk, wave within the pass, lane) of segment indices."""
    i = np.asarray(idx, np.int64)
    return i // CHUNK, (i % CHUNK) // PASS, (i % PASS) // WAVE, i % WAVE


def tie_facts(v: np.ndarray, k: int) -> dict:
    """What the data itself says: T = the k-th largest magnitude, how many magnitudes lie
    strictly above it, where the ones equal to it sit, and how many of those the cut keeps."""
    a = np.abs(np.asarray(v, np.float32).reshape(-1))
    T = np.sort(a)[::-1][k - 1]
    n_above = int((a > T).sum())
    ties = np.nonzero(a == T)[0]
    return {"T": np.float32(T), "n_above": n_above, "ties": ties, "cut": k - n_above}


def _decoy_slots(n: int, first_tie: int):
    """Four indices at the head of every chunk that lies wholly or partly below the first
    tie (lower indices only)."""
    slots = []
    for c in range(-(-n // CHUNK)):
        if c * CHUNK + 4 <= first_tie:
            slots.append(c * CHUNK + np.arange(4))
    return slots


def topk_tie_case(name, n, ratio, ties, cut, seed, T=T_DEFAULT, decoys=True, expect=None):
    """A length-n segment whose top-k cut keeps exactly `cut` of the elements tied at |v| == T.

    k - cut magnitudes lie strictly above T (decoys included), the tied elements have
    alternating sign, everything else lies strictly below.  Decoys (lower indices than the
    first tie, one set at the head of each chunk up to the tie's): nextafter(T, inf) and
    2T above, nextafter(T, 0) and T/2 below.  `expect` names the chunks / passes / waves
    the ties are meant to occupy."""
    T = np.float32(T)
    ties = np.asarray(ties, np.int64)
    k = topk_k(n, ratio)
    rng = np.random.default_rng(seed)
    v = np.zeros(n, np.float32)
    used = np.zeros(n, bool)
    used[ties] = True
    n_above = 0
    decoy_idx = []
    if decoys:
        for sl in _decoy_slots(n, int(ties.min())):
            v[sl] = [np.nextafter(T, np.float32(np.inf)), -np.nextafter(T, np.float32(0)),
                     np.float32(2) * T, -T / np.float32(2)]
            used[sl] = True
            n_above += 2
            decoy_idx.extend(sl.tolist())
    free = np.nonzero(~used)[0]
    want_above = k - cut - n_above
    assert 0 <= want_above <= free.size and 1 <= cut <= ties.size, name
    above = rng.choice(free, size=want_above, replace=False)
    is_above = np.zeros(n, bool)
    is_above[above] = True
    sign = np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    hi = (T * (np.float32(1.25) + np.float32(2.5) * rng.random(n).astype(np.float32)))
    lo = (T * np.float32(0.75) * rng.random(n).astype(np.float32))
    fill = np.where(is_above, hi, lo).astype(np.float32) * sign
    v[~used] = fill[~used]
    v[ties] = np.where(np.arange(ties.size) % 2 == 0, T, -T)
    return {"name": name, "n": n, "ratio": ratio, "k": k, "v": v, "T": T, "cut": cut,
            "ties": ties, "n_above": k - cut, "decoys": np.asarray(decoy_idx, np.int64),
            "expect": expect or {}}


def all_equal_case(name, n, ratio, seed):
    """Every magnitude equal (random signs): the whole segment is one tie, the first k kept."""
    rng = np.random.default_rng(seed)
    T = np.float32(0.0625)
    v = np.where(rng.random(n) < 0.5, -T, T).astype(np.float32)
    k = topk_k(n, ratio)
    return {"name": name, "n": n, "ratio": ratio, "k": k, "v": v, "T": T, "cut": k,
            "ties": np.arange(n), "n_above": 0, "decoys": np.zeros(0, np.int64), "expect": {}}


def zeros_case(name, n, ratio, nonzero, seed):
    """Signed zeros plus a few non-zeros: T = 0 and the cut falls among the zeros."""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    nonzero = np.asarray(nonzero, np.int64)
    v[nonzero] = (rng.standard_normal(nonzero.size).astype(np.float32) + np.float32(3)) \
        * np.where(np.arange(nonzero.size) % 2 == 0, np.float32(1), np.float32(-1))
    k = topk_k(n, ratio)
    ties = np.setdiff1d(np.arange(n), nonzero)
    return {"name": name, "n": n, "ratio": ratio, "k": k, "v": v, "T": np.float32(0),
            "cut": k - nonzero.size, "ties": ties, "n_above": int(nonzero.size),
            "decoys": np.zeros(0, np.int64), "expect": {}}


# 0x0040019A: subnormal (below 2**-126), low key byte 0x9A; 2T = 0x0080 0334 is normal,
# so the decoys are left out and every magnitude stays subnormal.
T_SUBNORMAL = np.array([0x0040019A], np.uint32).view(np.float32)[0]


def subnormal_case(name, n, ratio, ties, cut, seed):
    """topk_tie_case with every magnitude below 2**-126 (T itself subnormal)."""
    T = T_SUBNORMAL
    ties = np.asarray(ties, np.int64)
    k = topk_k(n, ratio)
    rng = np.random.default_rng(seed)
    Tk = int(key_of(T))
    keys = rng.integers(1, Tk, size=n).astype(np.uint32)            # strictly below T
    free = np.setdiff1d(np.arange(n), ties)
    above = rng.choice(free, size=k - cut, replace=False)
    keys[above] = rng.integers(Tk + 1, 0x00800000, size=above.size).astype(np.uint32)
    keys[ties] = Tk
    sign = (rng.random(n) < 0.5).astype(np.uint32) << np.uint32(31)
    sign[ties] = (np.arange(ties.size) % 2).astype(np.uint32) << np.uint32(31)
    v = (keys | sign).view(np.float32)
    return {"name": name, "n": n, "ratio": ratio, "k": k, "v": v, "T": T, "cut": cut,
            "ties": ties, "n_above": k - cut, "decoys": np.zeros(0, np.int64), "expect": {}}


def _r(a, b):
    return np.arange(a, b + 1)


def topk_cases() -> dict:
    """name -> case.  Three groups that share (n, ratio), so that three of a group can sit
    in the three client rows of one packed plan."""
    C = {}

    def add(c):
        assert c["name"] not in C
        C[c["name"]] = c

    n, r = 1000, 0.9  # k = 100: one chunk, four passes (the last ragged)
    add(topk_tie_case("single_wave", n, r, _r(70, 89), 7, 11,
                      expect={"chunks": {0}, "passes": {0}, "waves": {1}}))
    add(topk_tie_case("wave_boundary", n, r, _r(60, 69), 6, 12,
                      expect={"chunks": {0}, "passes": {0}, "waves": {0, 1}}))
    add(topk_tie_case("wave_boundary_cut_at_edge", n, r, _r(60, 69), 4, 13,
                      expect={"chunks": {0}, "passes": {0}, "waves": {0, 1}}))
    add(topk_tie_case("pass_boundary", n, r, _r(250, 261), 9, 14,
                      expect={"chunks": {0}, "passes": {0, 1}, "waves": {3, 0}}))
    add(topk_tie_case("pass_boundary_cut_at_edge", n, r, _r(250, 261), 6, 15,
                      expect={"chunks": {0}, "passes": {0, 1}, "waves": {3, 0}}))
    # all 64 lanes of wave 1 and lane 0 of wave 2: the (1 << lane) - 1 mask at lanes 63 / 0
    add(topk_tie_case("full_wave_cut63", n, r, _r(64, 128), 63, 16,
                      expect={"chunks": {0}, "passes": {0}, "waves": {1, 2}}))
    add(topk_tie_case("full_wave_cut64", n, r, _r(64, 128), 64, 17,
                      expect={"chunks": {0}, "passes": {0}, "waves": {1, 2}}))
    add(topk_tie_case("whole_tie_kept", n, r, _r(60, 69), 10, 18,
                      expect={"chunks": {0}, "passes": {0}, "waves": {0, 1}}))
    add(topk_tie_case("one_tie_kept", n, r, _r(250, 261), 1, 19,
                      expect={"chunks": {0}, "passes": {0, 1}, "waves": {3, 0}}))

    n = N3            # k = 2467: chunks 0..3, chunk 3 has 100 elements
    add(topk_tie_case("chunk0_only", n, r, _r(100, 119), 5, 21, expect={"chunks": {0}}))
    straddle = _r(8185, 8199)  # 7 ties in chunk 0, 8 in chunk 1
    for cut, tag in [(3, "earlier_gt_cut"), (7, "earlier_eq_cut"), (10, "later_keeps_some"),
                     (15, "whole_kept")]:
        add(topk_tie_case(f"chunk_straddle_{tag}", n, r, straddle, cut, 22 + cut,
                          expect={"chunks": {0, 1}}))
    add(topk_tie_case("chunk2_pass_boundary", n, r, 2 * CHUNK + _r(250, 261), 9, 40,
                      expect={"chunks": {2}, "passes": {0, 1}, "waves": {3, 0}}))
    # 3 ties in chunk 0, 4 in chunk 1, 5 across a wave boundary of chunk 2, the last element
    spread = np.concatenate([_r(8000, 8002), CHUNK + _r(5000, 5003), 2 * CHUNK + _r(62, 66),
                             [n - 1]])
    for cut, tag in [(2, "earlier_gt_cut"), (3, "earlier_eq_cut"), (5, "chunk1_keeps_some"),
                     (12, "all_but_last"), (13, "whole_kept")]:
        add(topk_tie_case(f"chunk_spread_{tag}", n, r, spread, cut, 50 + cut,
                          expect={"chunks": {0, 1, 2, 3}}))
    add(topk_tie_case("last_elements", n, r, _r(n - 3, n - 1), 2, 70, expect={"chunks": {3}}))

    n, r = 1000, 0.5  # k = 500
    add(all_equal_case("all_equal", n, r, 81))
    add(zeros_case("zeros_tie", n, r, [3, 64, 255, 256, 300, 511, 512, 700, 901, 999], 82))
    add(subnormal_case("subnormals", n, r, _r(250, 261), 9, 83))
    return C


# Three cases per launch (one per client row); every case appears exactly once.
TOPK_GROUPS = {
    "small_a": ["single_wave", "wave_boundary", "pass_boundary"],
    "small_b": ["full_wave_cut63", "full_wave_cut64", "wave_boundary_cut_at_edge"],
    "small_c": ["whole_tie_kept", "one_tie_kept", "pass_boundary_cut_at_edge"],
    "chunks_a": ["chunk0_only", "chunk_straddle_earlier_gt_cut", "chunk_straddle_earlier_eq_cut"],
    "chunks_b": ["chunk_straddle_later_keeps_some", "chunk_straddle_whole_kept",
                 "chunk2_pass_boundary"],
    "chunks_c": ["chunk_spread_earlier_gt_cut", "chunk_spread_earlier_eq_cut",
                 "chunk_spread_chunk1_keeps_some"],
    "chunks_d": ["chunk_spread_all_but_last", "chunk_spread_whole_kept", "last_elements"],
    "special": ["all_equal", "zeros_tie", "subnormals"],
}
# cases whose deltas only survive a base of zeros (signed zeros, subnormals)
ZERO_BASE_CASES = {"zeros_tie", "subnormals"}


# ------------------------------------------------------------------ quantiser
def _tile(vals, n):
    vals = np.asarray(vals, np.float32)
    return np.tile(vals, -(-n // vals.size))[:n].copy()


def quant_tie_cases() -> dict:
    """Inputs whose scale is exactly 1.0 and whose values sit on halves, so x / scale + zp
    lands on k + 0.5 for every element but the extremes' partners.  `codes_of` maps a value
    to the code round-half-to-even gives it (hand-derived: the even neighbour)."""
    C = {}
    s8 = [127.5, -127.5, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]
    C["sym8"] = {"x": _tile(s8, 306), "bits": 8, "symmetric": True, "scale": 1.0, "zp": 127,
                 "codes_of": {127.5: 254, -127.5: 0, 0.5: 128, 1.5: 128, 2.5: 130, -0.5: 126,
                              -1.5: 126, -2.5: 124, 3.5: 130}}
    s4 = [7.5, -7.5, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]
    C["sym4"] = {"x": _tile(s4, 306), "bits": 4, "symmetric": True, "scale": 1.0, "zp": 7,
                 "codes_of": {7.5: 14, -7.5: 0, 0.5: 8, 1.5: 8, 2.5: 10, -0.5: 6, -1.5: 6,
                              -2.5: 4, 3.5: 10}}
    halves = np.arange(255, dtype=np.float32) + np.float32(0.5)      # 0.5 .. 254.5
    a = np.concatenate([[0.0, 255.0], halves]).astype(np.float32)
    C["asym8_0_255"] = {"x": _tile(a, 320), "bits": 8, "symmetric": False, "scale": 1.0,
                        "zp": 0, "codes_of": None}
    C["asym8_m64_191"] = {"x": _tile(a - np.float32(64), 320), "bits": 8, "symmetric": False,
                          "scale": 1.0, "zp": 64, "codes_of": None}
    return C


def half_even_codes(x, zp, levels):
    """Codes of round-half-to-even at scale 1.0, by integer arithmetic on 2x (no rounding
    call): t = 2 * (x + zp) is an integer; t even -> t / 2, t odd -> the even neighbour."""
    t = np.rint(2.0 * (np.asarray(x, np.float64) + zp)).astype(np.int64)
    assert np.array_equal(t / 2.0, np.asarray(x, np.float64) + zp)
    lo = t >> 1                                   # floor((x + zp))
    q = np.where(t & 1, lo + (lo & 1), lo)
    return np.clip(q, 0, levels - 1)


def narrow_range(seed=91, n=300) -> np.ndarray:
    """1000.37 + 3e-3 * U[0, 1): at 8 bits asymmetric the zero point is about -8.5e7 and
    odd, so it is no fp32 integer (fp32 spacing there is 8)."""
    rng = np.random.default_rng(seed)
    return (np.float32(1000.37) + np.float32(3e-3) * rng.random(n).astype(np.float32)).astype(np.float32)


def wide16(seed=92, n=64) -> np.ndarray:
    """A spread of values for the 16-bit fixture: codes on both sides of 32768."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 2).astype(np.float32)


# segment kinds of the packed quantiser rows: (name, length)
def quant_segments(bits: int, symmetric: bool):
    segs = [("random", 700), ("multichunk", CHUNK + 17), ("small", 5)]
    if symmetric:
        segs.append(("zero", 300))
        if bits == 8:
            segs.append(("tie:sym8", 306))
        if bits == 4:
            segs.append(("tie:sym4", 306))
    else:
        segs += [("const", 300), ("one", 1), ("narrow", 300)]
        if bits == 8:
            segs += [("tie:asym8_0_255", 320), ("tie:asym8_m64_191", 320)]
    if bits == 16:
        segs.append(("wide16", 64))
    return segs


def quant_segment_data(kind: str, length: int, z: int, seed: int) -> np.ndarray:
    """Delta values of one (client z, segment).  Client 0 holds the canonical inputs (the
    ones recorded in compress_edges.json); other clients hold rotations / other draws."""
    rng = np.random.default_rng(1000 * seed + z)
    if kind == "random":
        return (rng.standard_normal(length) * 0.05).astype(np.float32)
    if kind == "multichunk":
        return (rng.standard_normal(length) * 0.01 + 0.003).astype(np.float32)
    if kind == "small":
        return rng.standard_normal(length).astype(np.float32)
    if kind == "zero":
        return np.zeros(length, np.float32)
    if kind == "const":
        return np.full(length, [0.75, -2.5, 1.0][z % 3], np.float32)
    if kind == "one":
        return np.array([[-3.0, 0.5, 7.25][z % 3]], np.float32)
    if kind == "narrow":
        return narrow_range(91 + z, length)
    if kind == "wide16":
        return wide16(92 + z, length)
    if kind.startswith("tie:"):
        x = quant_tie_cases()[kind[4:]]["x"]
        assert x.size == length
        return np.roll(x, 7 * z)
    raise KeyError(kind)


QUANT_CONFIGS = [(8, True), (4, True), (8, False), (1, True), (1, False), (16, True),
                 (16, False)]
# kinds whose deltas need a base of zeros to come out of fl32(x - base) unchanged
ZERO_BASE_KINDS = {"narrow", "wide16"}
# asymmetric kinds the reference raises on: pass-through, zp_out = INT64_MIN
PASSTHROUGH_KINDS = {"const", "one"}


def fixture_inputs() -> dict:
    """name -> (x, bits, symmetric) of every record in tests/golden/compress_edges.json."""
    out = {k: (c["x"], c["bits"], c["symmetric"]) for k, c in quant_tie_cases().items()}
    out["narrow8_asym"] = (narrow_range(), 8, False)
    out["wide16_sym"] = (wide16(), 16, True)
    out["wide16_asym"] = (wide16(), 16, False)
    return out
