"""The compression edge cases (tests/compress_cases.py) pinned without a GPU.

Every built case must have the facts it states — how many magnitudes lie strictly above
the threshold T, where the ties sit (chunk, pass, wave), that k cuts inside the tie by
exactly `cut`, which decoys share T's low key byte or its 24-bit prefix — and the oracle
(oracle/compress_ref.py) must agree with an independent restatement (stable argsort for
top-k, torch CPU fp32 for the quantiser) and with the reference's own outputs recorded
in tests/golden/compress_edges.json.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

import compress_cases as cc
from oracle import compress_ref

HERE = os.path.dirname(os.path.abspath(__file__))
EDGES = json.load(open(os.path.join(HERE, "golden", "compress_edges.json")))["cases"]
TOPK = cc.topk_cases()
QTIES = cc.quant_tie_cases()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ top-k builders
def test_groups_cover_every_case_once():
    names = [n for g in cc.TOPK_GROUPS.values() for n in g]
    assert sorted(names) == sorted(TOPK)
    for g in cc.TOPK_GROUPS.values():
        assert len(g) == 3
        assert len({(TOPK[n]["n"], TOPK[n]["ratio"]) for n in g}) == 1  # one plan per group


@pytest.mark.parametrize("name", sorted(TOPK))
def test_topk_case_has_its_stated_facts(name):
    c = TOPK[name]
    v, k = c["v"], c["k"]
    assert v.dtype == np.float32 and v.shape == (c["n"],) and np.isfinite(v).all()
    assert k == compress_ref.topk_k(c["n"], c["ratio"])
    f = cc.tie_facts(v, k)
    assert u32(f["T"]) == u32(c["T"])
    assert f["n_above"] == c["n_above"] == k - c["cut"]
    assert np.array_equal(f["ties"], np.sort(c["ties"]))
    assert f["cut"] == c["cut"] and 1 <= c["cut"] <= c["ties"].size
    assert int((np.abs(v) < c["T"]).sum()) == c["n"] - c["n_above"] - c["ties"].size
    if name not in ("all_equal", "zeros_tie"):   # alternating sign along the tie
        assert np.array_equal(np.signbit(v[c["ties"]]), np.arange(c["ties"].size) % 2 == 1)
    ch, ps, wv, _ = cc.where_of(c["ties"])
    for key, got in (("chunks", ch), ("passes", ps), ("waves", wv)):
        if key in c["expect"]:
            assert set(got.tolist()) == c["expect"][key], key


def test_topk_layouts_sit_where_the_kernel_changes_path():
    ch, ps, wv, ln = cc.where_of(TOPK["wave_boundary"]["ties"])
    assert wv.tolist() == [0] * 4 + [1] * 6 and ln.tolist() == [60, 61, 62, 63, 0, 1, 2, 3, 4, 5]
    assert TOPK["wave_boundary"]["cut"] > 4 == TOPK["wave_boundary_cut_at_edge"]["cut"]
    ch, ps, wv, ln = cc.where_of(TOPK["pass_boundary"]["ties"])
    assert ps.tolist() == [0] * 6 + [1] * 6
    assert TOPK["pass_boundary"]["cut"] > 6 == TOPK["pass_boundary_cut_at_edge"]["cut"]
    ch, ps, wv, ln = cc.where_of(TOPK["full_wave_cut64"]["ties"])
    assert ln[wv == 1].tolist() == list(range(64)) and ln[wv == 2].tolist() == [0]
    assert TOPK["full_wave_cut63"]["cut"] == 63 and TOPK["full_wave_cut64"]["cut"] == 64
    c = TOPK["whole_tie_kept"]
    assert c["cut"] == c["ties"].size               # kr == cnt_eq: the non-ranked path
    assert TOPK["one_tie_kept"]["cut"] == 1
    # chunk straddle: 7 ties in chunk 0, 8 in chunk 1; cuts below / at / above / all
    cuts = {}
    for tag in ("earlier_gt_cut", "earlier_eq_cut", "later_keeps_some", "whole_kept"):
        c = TOPK[f"chunk_straddle_{tag}"]
        chunks = cc.where_of(c["ties"])[0]
        assert np.bincount(chunks).tolist() == [7, 8] and c["n"] == cc.N3
        cuts[tag] = c["cut"]
    assert cuts["earlier_gt_cut"] < 7 == cuts["earlier_eq_cut"] < cuts["later_keeps_some"] < 15
    assert cuts["whole_kept"] == 15
    cuts = {}
    for tag in ("earlier_gt_cut", "earlier_eq_cut", "chunk1_keeps_some", "all_but_last",
                "whole_kept"):
        c = TOPK[f"chunk_spread_{tag}"]
        assert np.bincount(cc.where_of(c["ties"])[0]).tolist() == [3, 4, 5, 1]
        assert c["ties"][-1] == c["n"] - 1
        cuts[tag] = c["cut"]
    assert cuts["earlier_gt_cut"] < 3 == cuts["earlier_eq_cut"] < cuts["chunk1_keeps_some"] < 7
    assert cuts["all_but_last"] == 12 and cuts["whole_kept"] == 13
    c = TOPK["chunk2_pass_boundary"]
    assert set(cc.where_of(c["decoys"])[0].tolist()) == {0, 1, 2}   # decoys in earlier chunks
    c = TOPK["last_elements"]
    assert c["ties"].tolist() == [c["n"] - 3, c["n"] - 2, c["n"] - 1]
    assert cc.N3 % cc.CHUNK == 100


@pytest.mark.parametrize("name", sorted(n for n in TOPK if TOPK[n]["decoys"].size))
def test_topk_decoys_split_low_byte_and_prefix(name):
    c = TOPK[name]
    Tk = int(cc.key_of(c["T"]))
    d = c["decoys"]
    assert d.size % 4 == 0 and d.max() < c["ties"].min()
    keys = cc.key_of(c["v"][d]).astype(np.int64).reshape(-1, 4)
    for up, down, twice, half in keys:
        assert up == Tk + 1 and down == Tk - 1            # same 24-bit prefix, other low byte
        assert up >> 8 == Tk >> 8 == down >> 8
        for kk in (twice, half):                          # same low byte, other prefix
            assert kk & 255 == Tk & 255 and kk >> 8 != Tk >> 8
        assert twice > Tk > half


def test_special_cases_are_what_they_claim():
    v = TOPK["all_equal"]["v"]
    assert np.unique(np.abs(v)).size == 1 and 0 < np.signbit(v).sum() < v.size
    c = TOPK["zeros_tie"]
    z = c["v"][c["ties"]]
    assert (z == 0).all() and 0 < np.signbit(z).sum() < z.size   # both +0.0 and -0.0
    assert c["T"] == 0 and 0 < c["cut"] < c["ties"].size
    c = TOPK["subnormals"]
    a = np.abs(c["v"])
    assert (a > 0).all() and (a < np.float32(2.0 ** -126)).all()
    assert (cc.key_of(c["v"]) < 0x00800000).all()


@pytest.mark.parametrize("name", sorted(TOPK))
def test_topk_oracle_matches_stable_argsort(name):
    c = TOPK[name]
    v, k = c["v"], c["k"]
    order = np.argsort(-np.abs(v).astype(np.float64), kind="stable")
    idx = np.sort(order[:k])
    assert np.array_equal(compress_ref.topk_indices(v, k), idx)
    exp = np.zeros_like(v)
    exp[idx] = v[idx]
    assert np.array_equal(u32(compress_ref.topk_dense(v, c["ratio"])), u32(exp))
    # the kept set: everything above T and the first `cut` ties
    kept = np.zeros(v.size, bool)
    kept[np.abs(v) > c["T"]] = True
    kept[np.sort(c["ties"])[:c["cut"]]] = True
    assert np.array_equal(np.nonzero(kept)[0], idx)


# ------------------------------------------------------------------ quantiser builders
def torch_quant(x, bits, symmetric):
    """Independent restatement on CPU torch, fp32: parameters from min / max, then
    round(x / scale + zp).clamp(0, L - 1) and (q - zp) * scale."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    L = 2 ** bits
    if symmetric:
        scale = 2 * t.abs().max().item() / (L - 1)
        zp = (L - 1) // 2
    else:
        lo, hi = t.min().item(), t.max().item()
        scale = (hi - lo) / (L - 1)
        zp = -round(lo / scale)
    q = torch.round(t / scale + zp).clamp(0, L - 1)
    codes = q.to(torch.uint8 if bits <= 8 else torch.int16)
    dense = (codes.float() - zp) * scale
    return codes.numpy(), scale, zp, dense.numpy()


@pytest.mark.parametrize("name", sorted(QTIES))
def test_quant_tie_case_sits_on_halves(name):
    c = QTIES[name]
    x, L = c["x"], 2 ** c["bits"]
    assert x.size >= 300 and x.size > 4 * cc.WAVE
    scale, zp = compress_ref.quant_params(x, c["bits"], c["symmetric"])
    assert scale == 1.0 == c["scale"] and zp == c["zp"]
    t = x.astype(np.float64) + zp
    on_half = (t - np.floor(t)) == 0.5
    assert on_half.sum() >= x.size - 4 * (x.size // 9 + 1) and on_half.sum() >= 250
    waves = set((np.nonzero(on_half)[0] // cc.WAVE).tolist())
    assert len(waves) >= 4                                   # halves on several waves
    codes, _, _ = compress_ref.quantize(x, c["bits"], c["symmetric"])
    assert np.array_equal(codes, cc.half_even_codes(x, zp, L))
    if c["codes_of"]:
        for val, code in c["codes_of"].items():
            assert (codes[x == np.float32(val)] == code).all(), val
    # round-half-away gives another code wherever half-to-even rounds a positive half down
    # (even + 0.5): about every other element, spread over all waves
    t32 = x + np.float32(zp)
    away = np.clip(np.sign(t32) * np.floor(np.abs(t32) + np.float32(0.5)), 0, L - 1)
    differs = away != codes
    assert np.array_equal(differs, on_half & (np.floor(t) % 2 == 0) & (t > 0))
    assert differs.sum() >= x.size // 3
    assert set((np.nonzero(differs)[0] // cc.WAVE).tolist()) == waves


@pytest.mark.parametrize("bits,symmetric", cc.QUANT_CONFIGS)
def test_quant_oracle_matches_torch_restatement(bits, symmetric):
    for kind, length in cc.quant_segments(bits, symmetric):
        if kind in cc.PASSTHROUGH_KINDS or kind == "zero":
            continue
        for z in range(3):
            x = cc.quant_segment_data(kind, length, z, seed=bits * 2 + symmetric)
            codes, scale, zp = compress_ref.quantize(x, bits, symmetric)
            dense = compress_ref.dequantize(codes, scale, zp)
            tc, ts, tz, td = torch_quant(x, bits, symmetric)
            assert (scale, zp) == (ts, tz), (kind, z)
            assert codes.dtype == tc.dtype and np.array_equal(codes, tc), (kind, z)
            assert np.array_equal(u32(dense), u32(td)), (kind, z)


def test_quant_degenerate_segments():
    for z in range(3):                    # the reference raises: D14 passes them through
        for kind, n in (("const", 300), ("one", 1)):
            x = cc.quant_segment_data(kind, n, z, seed=0)
            assert x.min() == x.max() != 0
            with pytest.raises(ZeroDivisionError):
                compress_ref.quant_params(x, 8, False)
    codes, scale, zp = compress_ref.quantize(np.zeros(300, np.float32), 8, True)
    assert scale == 0.0 and zp == 127 and not codes.any()
    x = cc.narrow_range()
    scale, zp = compress_ref.quant_params(x, 8, False)
    assert -1e9 < zp < -5e7 and int(np.float32(zp)) != zp     # no fp32 integer
    for bits in (1, 16):                  # a 1-bit symmetric max lands on 0.5 -> code 0
        x = cc.quant_segment_data("random", 700, 0, seed=bits * 2 + 1)
        codes, scale, zp = compress_ref.quantize(x, bits, True)
        if bits == 1:
            assert zp == 0 and codes[np.argmax(np.abs(x))] == 0 and set(codes.tolist()) <= {0, 1}
        else:
            assert codes.dtype == np.int16 and (codes < 0).any()   # wrapped codes >= 32768


@pytest.mark.parametrize("name", sorted(EDGES))
def test_oracle_reproduces_reference_fixture(name):
    exp = EDGES[name]
    x, bits, sym = cc.fixture_inputs()[name]
    assert (bits, sym, x.size) == (exp["bits"], exp["symmetric"], exp["numel"])
    codes, scale, zp = compress_ref.quantize(x, bits, sym)
    assert scale == exp["scale"] and zp == exp["zero_point"]
    assert str(codes.dtype) == exp["codes_dtype"]
    assert codes.tolist() == exp["codes"]
    dense = compress_ref.dequantize(codes, scale, zp)
    assert u32(dense).tolist() == exp["dense_u32"]


def test_fixture_covers_the_builders():
    assert sorted(EDGES) == sorted(cc.fixture_inputs())
    assert set(QTIES) <= set(EDGES)
