"""fh_topk_rows / fh_quantize_rows at their edges, bit for bit against the oracle.

Top-k: every tie layout of tests/compress_cases.py (ties across a wave, a 256-element
pass, an 8192-element chunk; cuts before, at and after each boundary; decoys that share
the threshold's low key byte or its prefix; all-equal, signed-zero and subnormal
segments) inside a packed plan of 4 segments x 3 clients whose tied segment is not the
first, in place and out of place, without a base, with a broadcast base and with a
per-client base.  Quantiser: values on exact halves (the rounding rule), degenerate
segments (DESIGN.md D14 pass-through), a zero point that is no fp32 integer, 1 and 16
bits, against the oracle and the reference's own outputs (golden/compress_edges.json).

Addressing: seg_offsets[0] = 64, every tensor has its own row stride, all outputs are
pre-filled with a poison pattern and every byte outside the plan's range must keep it.

No tolerances: floats are compared by their uint32 view.  The only values left
uncompared are the codes of the asymmetric pass-through segments (unspecified)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import compress_cases as cc
from fedhip.compress import SegmentPlan, quantize_rows, topk_rows
from oracle import compress_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HERE = os.path.dirname(os.path.abspath(__file__))
EDGES = json.load(open(os.path.join(HERE, "golden", "compress_edges.json")))["cases"]
TOPK = cc.topk_cases()

C = 3
LEAD, TAIL = 64, 37                       # row elements before / after the plan's range
PAD_X, PAD_OUT, PAD_BYTES, PAD_BASE = 96, 160, 32, 224   # row stride = width + pad
POISON_I32 = 0xDEADBEEF - (1 << 32)       # a finite float, -6.26e18
POISON_U8 = 0xA5
INT64_MIN = -(1 << 63)
BASE_MODES = ["none", "broadcast", "per_client"]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def poisoned(rows, stride, dtype):
    """[rows, stride] tensor over one flat poisoned allocation."""
    if dtype == torch.uint8:
        return torch.full((rows, stride), POISON_U8, dtype=torch.uint8, device=DEV)
    return torch.full((rows, stride), POISON_I32, dtype=torch.int32, device=DEV).view(torch.float32)


def upload(rows_np, lo, hi, pad):
    """Poisoned [C, W + pad] buffer holding rows_np[:, lo:hi] in place; everything else
    (lead, tail, the space between rows) stays poison."""
    W = rows_np.shape[1]
    buf = poisoned(rows_np.shape[0], W + pad, torch.float32)
    buf[:, lo:hi] = torch.from_numpy(np.ascontiguousarray(rows_np[:, lo:hi])).to(DEV)
    return buf


def assert_poison_outside(buf, lo, hi):
    """Every element of the allocation outside columns [lo, hi) of each row is poison."""
    a = buf.cpu()
    if a.dtype == torch.uint8:
        a, p = a.numpy(), POISON_U8
    else:
        a, p = a.view(torch.int32).numpy(), POISON_I32
    assert (a[:, :lo] == p).all() and (a[:, hi:] == p).all()


def grid_base(rng, shape, step, amp):
    """Base values on a coarse grid (multiples of `step`, |b| <= amp) so that base + delta
    and back is exact for the deltas that must survive unchanged."""
    m = int(round(amp / step))
    return (rng.integers(-m, m + 1, size=shape).astype(np.float64) * step).astype(np.float32)


def make_base(mode, rng, W, step, amp, zero_cols):
    """None, one broadcast row [W] or per-client rows [C, W]; zero_cols: per client the
    column ranges that need a base of zeros."""
    if mode == "none":
        return None
    if mode == "broadcast":
        b = grid_base(rng, (1, W), step, amp)
        for z in range(C):
            for a, e in zero_cols[z]:
                b[0, a:e] = 0
        return b
    b = grid_base(rng, (C, W), step, amp)
    for z in range(C):
        for a, e in zero_cols[z]:
            b[z, a:e] = 0
    return b


def base_row(base, z):
    return None if base is None else base[0 if base.shape[0] == 1 else z]


def base_tensor(base, W):
    """Device base and the allocation to check afterwards: the broadcast row has stride 0,
    the per-client rows a stride of their own."""
    if base is None:
        return None, None
    if base.shape[0] == 1:
        t = torch.from_numpy(base).to(DEV)
        return t.expand(C, -1), t
    buf = upload(base, 0, W, PAD_BASE)
    return buf[:, :W], buf


# ------------------------------------------------------------------ top-k
@functools.lru_cache(maxsize=None)
def topk_problem(group, mode):
    names = cc.TOPK_GROUPS[group]
    cases = [TOPK[n] for n in names]
    n, ratio = cases[0]["n"], cases[0]["ratio"]
    lens = [300, n, cc.CHUNK + 17, 1] if n <= cc.CHUNK else [cc.CHUNK + 5, n, 300, 1]
    seg = np.concatenate([[LEAD], LEAD + np.cumsum(lens)]).tolist()
    W = seg[-1] + TAIL
    rng = np.random.default_rng(sum(map(ord, group)))
    delta = (rng.standard_normal((C, W)) * 0.05).astype(np.float32)
    for z, c in enumerate(cases):
        delta[z, seg[1]:seg[2]] = c["v"]
    zero_cols = [[(seg[1], seg[2])] if names[z] in cc.ZERO_BASE_CASES else [] for z in range(C)]
    # 2**-22 grid, |b| <= 2**-6: exact with T = 0.3, its neighbours, 2T, T/2 and 2**-4
    base = make_base(mode, rng, W, 2.0 ** -22, 2.0 ** -6, zero_cols)
    x = delta if base is None else (base + delta).astype(np.float32)
    for z in range(C):       # over a base of +0.0 the row is the delta itself (-0.0 kept)
        for a, e in zero_cols[z]:
            x[z, a:e] = delta[z, a:e]
    exp_out = np.zeros((C, W), np.float32)
    exp_keep = np.zeros((C, W), np.uint8)
    ks = [compress_ref.topk_k(e - a, ratio) for a, e in zip(seg[:-1], seg[1:])]
    for z in range(C):
        b = base_row(base, z)
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            d = x[z, a:e] if b is None else (x[z, a:e] - b[a:e]).astype(np.float32)
            dense = compress_ref.topk_dense(d, ratio)
            exp_out[z, a:e] = dense if b is None else (b[a:e] + dense).astype(np.float32)
            exp_keep[z, a + compress_ref.topk_indices(d, ks[s])] = 1
            if s == 1:   # the delta the kernel sees still has the case's facts
                c, f = cases[z], cc.tie_facts(d, ks[s])
                assert u32(f["T"]) == u32(c["T"]) and f["n_above"] == c["n_above"]
                assert np.array_equal(f["ties"], np.sort(c["ties"])) and f["cut"] == c["cut"]
                assert np.array_equal(u32(d[c["ties"]]), u32(c["v"][c["ties"]]))
    for a in (x, exp_out, exp_keep):
        a.setflags(write=False)
    return {"seg": seg, "W": W, "ratio": ratio, "ks": ks, "x": x, "base": base,
            "exp_out": exp_out, "exp_keep": exp_keep}


def run_topk(p, inplace):
    seg, W = p["seg"], p["W"]
    lo, hi = seg[0], seg[-1]
    plan = SegmentPlan(seg, DEV)
    assert plan.chunk_offsets[1].item() > 0          # the tied segment is not the first
    xb = upload(p["x"], lo, hi, PAD_X)
    x_before = xb.clone()
    base, base_alloc = base_tensor(p["base"], W)
    base_before = None if base_alloc is None else base_alloc.clone()
    ob = xb if inplace else poisoned(C, W + PAD_OUT, torch.float32)
    kb = poisoned(C, W + PAD_BYTES, torch.uint8)
    x, out, keep = xb[:, :W], ob[:, :W], kb[:, :W]
    strides = {x.stride(0), keep.stride(0)} | ({out.stride(0)} if not inplace else set())
    if base is not None:
        strides.add(base.stride(0))
    assert len(strides) == 2 + (not inplace) + (base is not None)   # all different
    topk_rows(plan, x, C, p["ratio"], base=base, out=out, keep=keep)
    torch.cuda.synchronize()
    if not inplace:
        assert torch.equal(xb.view(torch.int32), x_before.view(torch.int32))
    if base_alloc is not None:
        assert torch.equal(base_alloc.view(torch.int32), base_before.view(torch.int32))
    return ob, kb


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("mode", BASE_MODES)
@pytest.mark.parametrize("group", sorted(cc.TOPK_GROUPS))
def test_topk_tie_layouts_match_oracle(group, mode, inplace):
    p = topk_problem(group, mode)
    seg = p["seg"]
    lo, hi = seg[0], seg[-1]
    ob, kb = run_topk(p, inplace)
    assert_poison_outside(ob, lo, hi)
    assert_poison_outside(kb, lo, hi)
    keep = kb.cpu().numpy()[:, lo:hi]
    out = ob.cpu().numpy()[:, lo:hi]
    for z in range(C):           # the invariant a rank slip breaks first
        for s, (a, e) in enumerate(zip(seg[:-1], seg[1:])):
            assert int(keep[z, a - lo:e - lo].sum()) == p["ks"][s], (z, s)
    assert np.array_equal(keep, p["exp_keep"][:, lo:hi])
    assert np.array_equal(u32(out), u32(p["exp_out"][:, lo:hi]))


def test_topk_signed_zeros_and_subnormals_survive():
    """Without a base the kept elements are the input's own bits: -0.0 stays -0.0, a
    subnormal stays subnormal (no flush), a dropped element is +0.0."""
    p = topk_problem("special", "none")
    ob, kb = run_topk(p, inplace=False)
    a, e = p["seg"][1], p["seg"][2]
    out = ob.cpu().numpy()[:, a:e]
    keep = kb.cpu().numpy()[:, a:e].astype(bool)
    names = cc.TOPK_GROUPS["special"]
    zz, zs = names.index("zeros_tie"), names.index("subnormals")
    x = p["x"][:, a:e]
    for z in (zz, zs):
        assert np.array_equal(u32(out[z])[keep[z]], u32(x[z])[keep[z]])
        assert not u32(out[z])[~keep[z]].any()
    kept_zero = keep[zz] & (x[zz] == 0)
    assert (u32(out[zz])[kept_zero] == 0x80000000).any() and (u32(out[zz])[kept_zero] == 0).any()
    assert (np.abs(out[zs])[keep[zs]] > 0).all() and keep[zs].sum() == p["ks"][1]


def test_topk_is_deterministic():
    """The histograms use atomics (integer: order-free): two runs of the largest case into
    separate buffers give the same bytes."""
    p = topk_problem("chunks_c", "per_client")
    o1, k1 = run_topk(p, inplace=False)
    o2, k2 = run_topk(p, inplace=False)
    assert o1.data_ptr() != o2.data_ptr()
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(k1, k2)


# ------------------------------------------------------------------ quantiser
def fixture_name(kind, bits, sym):
    if kind.startswith("tie:"):
        return kind[4:]
    if kind == "narrow" and bits == 8 and not sym:
        return "narrow8_asym"
    if kind == "wide16":
        return f"wide16_{'sym' if sym else 'asym'}"
    return None


@functools.lru_cache(maxsize=None)
def quant_problem(bits, sym, mode):
    segs = cc.quant_segments(bits, sym)
    lens = [n for _, n in segs]
    seg = np.concatenate([[LEAD], LEAD + np.cumsum(lens)]).tolist()
    W = seg[-1] + TAIL
    rng = np.random.default_rng(100 * bits + sym)
    delta = np.zeros((C, W), np.float32)
    for z in range(C):
        for (kind, n), a in zip(segs, seg[:-1]):
            delta[z, a:a + n] = cc.quant_segment_data(kind, n, z, seed=bits * 2 + sym)
    zero_cols = [[(a, e) for (kind, _), a, e in zip(segs, seg[:-1], seg[1:])
                  if kind in cc.ZERO_BASE_KINDS]] * C
    # 2**-10 grid, |b| <= 0.25: exact with the halves up to 255 and the constants
    base = make_base(mode, rng, W, 2.0 ** -10, 0.25, zero_cols)
    x = delta if base is None else (base + delta).astype(np.float32)
    exp = []      # per client, per segment: dict(out, codes | None, scale, zp)
    for z in range(C):
        b = base_row(base, z)
        row = []
        for (kind, n), a, e in zip(segs, seg[:-1], seg[1:]):
            d = x[z, a:e] if b is None else (x[z, a:e] - b[a:e]).astype(np.float32)
            if kind.startswith("tie:") or kind in cc.ZERO_BASE_KINDS or kind in ("const", "zero"):
                assert np.array_equal(u32(d), u32(delta[z, a:e])), kind   # delta came through
            if not sym and kind in cc.PASSTHROUGH_KINDS:
                assert d.min() == d.max()
                r = {"dense": d, "codes": None, "scale": 0.0, "zp": INT64_MIN}
            else:
                codes, scale, zp = compress_ref.quantize(d, bits, sym)
                r = {"dense": compress_ref.dequantize(codes, scale, zp), "codes": codes,
                     "scale": scale, "zp": zp}
                fx = fixture_name(kind, bits, sym) if z == 0 else None
                if fx:   # the reference's own numbers for the canonical input
                    g = EDGES[fx]
                    r = {"dense": np.array(g["dense_u32"], np.uint32).view(np.float32),
                         "codes": np.array(g["codes"], codes.dtype), "scale": g["scale"],
                         "zp": g["zero_point"], "fixture": fx}
                    assert np.array_equal(r["codes"], codes) and r["scale"] == scale
            r["out"] = r["dense"] if b is None else (b[a:e] + r["dense"]).astype(np.float32)
            row.append(r)
        exp.append(row)
    x.setflags(write=False)
    return {"segs": segs, "seg": seg, "W": W, "x": x, "base": base, "exp": exp}


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("mode", BASE_MODES)
@pytest.mark.parametrize("bits,sym", cc.QUANT_CONFIGS,
                         ids=[f"{b}bit_{'sym' if s else 'asym'}" for b, s in cc.QUANT_CONFIGS])
def test_quantize_edges_match_oracle(bits, sym, mode, inplace):
    p = quant_problem(bits, sym, mode)
    segs, seg, W = p["segs"], p["seg"], p["W"]
    lo, hi = seg[0], seg[-1]
    nseg = len(segs)
    plan = SegmentPlan(seg, DEV)
    assert plan.nchunks > nseg                       # one multi-chunk segment at least
    xb = upload(p["x"], lo, hi, PAD_X)
    x_before = xb.clone()
    base, base_alloc = base_tensor(p["base"], W)
    base_before = None if base_alloc is None else base_alloc.clone()
    ob = xb if inplace else poisoned(C, W + PAD_OUT, torch.float32)
    cb = poisoned(C, W + PAD_BYTES, torch.uint8) if bits <= 8 else None
    scale = torch.full((C, nseg), float("nan"), dtype=torch.float64, device=DEV)
    zp = torch.full((C, nseg), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    quantize_rows(plan, xb[:, :W], C, bits, sym, base=base, out=ob[:, :W],
                  codes=None if cb is None else cb[:, :W], scale_out=scale, zp_out=zp)
    torch.cuda.synchronize()
    if not inplace:
        assert torch.equal(xb.view(torch.int32), x_before.view(torch.int32))
    if base_alloc is not None:
        assert torch.equal(base_alloc.view(torch.int32), base_before.view(torch.int32))
    assert_poison_outside(ob, lo, hi)
    if cb is not None:
        assert_poison_outside(cb, lo, hi)
    out = ob.cpu().numpy()
    codes = None if cb is None else cb.cpu().numpy()
    scale, zp = scale.cpu().numpy(), zp.cpu().numpy()
    for z in range(C):
        for s, ((kind, n), a, e) in enumerate(zip(segs, seg[:-1], seg[1:])):
            r = p["exp"][z][s]
            tag = (z, kind, r.get("fixture"))
            assert scale[z, s] == r["scale"] and int(zp[z, s]) == r["zp"], tag
            assert np.array_equal(u32(out[z, a:e]), u32(r["out"])), tag
            if codes is not None and r["codes"] is not None:   # pass-through: unspecified
                assert np.array_equal(codes[z, a:e], r["codes"]), tag


def test_quantize_fixture_cases_all_ran():
    """Every record of compress_edges.json is reached by some configuration above."""
    seen = set()
    for bits, sym in cc.QUANT_CONFIGS:
        for row in quant_problem(bits, sym, "none")["exp"]:
            seen |= {r["fixture"] for r in row if "fixture" in r}
    assert seen == set(EDGES)
