"""Exact-integer conv / linear tests across the lane fill fractions.

Every split planner of csrc/conv.hip is a function of the packed client count and of the
thread-local fill fraction (fh_set_fill_fraction); fedhip/lanes.py issues its lanes at 0.25,
0.5 and 0.75, a single lane at 1.0.  Here every kernel family runs at all four, on ragged
lanes of 1, 2-3, 8-9 and 23 clients, with small-integer operands: every product and partial
sum is exact in fp32, so whatever the split plan (number of splits, stages or K-steps per
split, a short last split) the result must equal the fp64 reference bit for bit, and a
dropped or doubled term is an integer error at a named (shape, fraction, client count).

Case tables, operands and references: tests/conv_fill_ref.py.  The tests without the gpu
mark need only the built library (size queries, the fill-fraction accessors, the magnitude
bound that makes `torch.equal` the right assertion).
"""
import threading

import pytest
import torch

import conv_fill_ref as cf
from fedhip import _lib, ops

gpu = pytest.mark.gpu
DEV = "cuda"

CONV_IDS = [f"{n}-{cf.case_id(c)}" for n, c in cf.CONV_CASES]
LIN_IDS = [cf.case_id(c) for c in cf.LINEAR_CASES]
S2_CASES = cf.FAMILY["s2_3x3"].cases


# ------------------------------------------------------------------ CPU tier: the table itself
def test_operand_magnitudes_stay_exact():
    """|any result or partial sum| <= VMAX^2 x reduction length + bias + accumulate base
    stays below 2^24 for every case, so fp32 holds every intermediate exactly."""
    for name, case in cf.CONV_CASES:
        f = cf.FAMILY[name]
        for what, bound in cf.conv_magnitude_bounds(case, f.k, f.stride, f.pad).items():
            assert bound < cf.EXACT_LIMIT, (name, case, what, bound)
    for case in cf.LINEAR_CASES:
        for what, bound in cf.linear_magnitude_bounds(case).items():
            assert bound < cf.EXACT_LIMIT, (case, what, bound)


def test_lane_widths_and_ragged_counts():
    """The table covers the KT cut's lane widths (1, 8-9, 23) and a small middle lane; client
    0 is full, and a case of >= 3 clients has a client with exactly one image."""
    for cases in ([c for _, c in cf.CONV_CASES], cf.LINEAR_CASES):
        widths = {c[0] for c in cases}
        assert 1 in widths and widths & {2, 3} and widths & {8, 9} and 23 in widths
        for c in cases:
            counts = cf.ragged_counts(c[0], c[1]).tolist()
            assert counts[0] == c[1] and all(1 <= n <= c[1] for n in counts)
            assert c[0] < 3 or 1 in counts


def _groups():
    out = {}
    for f in cf.FAMILIES:
        out.setdefault(f.group, []).append(f)
    return out


@pytest.mark.parametrize("group", sorted(_groups()))
def test_workspace_sizes_move_with_the_fraction(group):
    """The sweep must not degenerate into twelve copies of one plan: per family and operation
    with a split path, some case's queried workspace takes at least two distinct non-zero
    sizes over the four fractions, and some (case, fraction) reports the unsplit size.

    The limit of this guard: a public query is the LARGEST slab of every plan its entry point
    may take (WGRAD: the direct kernel's plan and plan_wgrad's; stride-2 DGRAD: the direct
    kernel's slab and the packed weights + plan_dgrad_s2's), so a size that moves, or equals
    the unsplit size, may describe the implicit-GEMM plan beside the kernel that is launched.
    It catches a table gone flat; that the launched kernels' own plans change is derived per
    case in the comments of tests/conv_fill_ref.py, not established here."""
    lib = _lib.load()
    fams = _groups()[group]
    for op in ("fwd", "dgrad", "wgrad"):
        if not any(op in f.split_ops for f in fams):
            continue
        moved, unsplit, seen = False, False, {}
        for f in fams:
            for case in f.cases:
                sizes = cf.sweep_sizes(
                    lib, lambda: cf.conv_query(lib, op, case, f.k, f.stride, f.pad))
                seen[case] = [sizes[fr] for fr in cf.FRACTIONS]
                moved |= len({v for v in sizes.values() if v}) >= 2
                unsplit |= cf.conv_no_split_bytes(op, case, f.k, f.stride,
                                                  f.slab_wgrad) in sizes.values()
        print(group, op, seen)
        assert moved, f"{group} {op}: every case has one plan at all fractions: {seen}"
        assert unsplit, f"{group} {op}: no (case, fraction) is unsplit: {seen}"


def test_linear_workspace_sizes_move_with_the_fraction():
    """As above for fh_linear_fwd_workspace / _dgrad_workspace, which see the implicit-GEMM
    plans only (plan_mn; the case that runs them is 23x4x520x512).  The FWD query cannot show
    plan_lin_fwd moving: it sizes the skinny kernel's slab with the whole-chip plan whatever
    the fraction, so its byte counts prove nothing about linear_fwd_skinny_kernel; that the
    skinny plan changes (23x4x1024x256, 23x4x2048x512) is derived in tests/conv_fill_ref.py.

    Linear WGRAD is exempt from both conditions, a deliberate loosening: fh_linear_wgrad does
    have a split path, the implicit-GEMM WGRAD at batch >= 256 (K = batch in runs of at least
    128; batch <= 32 takes the skinny kernel), which no lane reaches and which the igemm
    family covers as a conv.  Its query is only required to be 0 for this table."""
    lib = _lib.load()
    for op in ("fwd", "dgrad"):
        seen = {c: cf.sweep_sizes(lib, lambda: cf.linear_query(lib, op, c))
                for c in cf.LINEAR_CASES}
        print("linear", op, seen)
        assert any(len({v for v in s.values() if v}) >= 2 for s in seen.values()), (op, seen)
        assert any(0 in s.values() for s in seen.values()), (op, seen)
    for c in cf.LINEAR_CASES:
        assert set(cf.sweep_sizes(lib, lambda: cf.linear_query(lib, "wgrad", c)).values()) == {0}


def test_fill_fraction_accessors():
    """fh_get_fill_fraction returns what fh_set_fill_fraction stored; the value is per thread
    (a new thread starts at 1.0 whatever its parent set: fedhip/lanes.py sets it on each
    issuing thread); values outside (0, 1] are refused with FH_E_INVALID and change nothing."""
    lib = _lib.load()
    try:
        for fr in cf.FRACTIONS:
            _lib.call("fh_set_fill_fraction", fr)
            assert lib.fh_get_fill_fraction() == fr  # quarters: exact in fp32
        _lib.call("fh_set_fill_fraction", 0.25)
        seen = []
        t = threading.Thread(target=lambda: seen.append(lib.fh_get_fill_fraction()))
        t.start()
        t.join()
        assert seen == [1.0]
        assert lib.fh_get_fill_fraction() == 0.25
        for bad in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(_lib.FedHipError, match=r"rc=-1\).*fill fraction"):
                _lib.call("fh_set_fill_fraction", bad)
            assert lib.fh_get_fill_fraction() == 0.25
    finally:
        lib.fh_set_fill_fraction(1.0)
    assert lib.fh_get_fill_fraction() == 1.0


# ------------------------------------------------------------------ GPU tier
class _Fill:
    """ops.set_fill_fraction(fraction) for a block, 1.0 restored after it."""

    def __init__(self, fraction):
        self.fraction = fraction

    def __enter__(self):
        ops.set_fill_fraction(self.fraction)

    def __exit__(self, *exc):
        ops.set_fill_fraction(1.0)


def _eq(got, ref, what):
    got = got.cpu().double()
    if not torch.equal(got, ref):
        d = (got - ref).abs()
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.numel()} elements differ, "
                             f"max |diff| {d.max().item():g}")


def _run_conv(name, case, fwd=True, dgrad=True, wgrad=True, tag=""):
    """FWD, DGRAD (plain and accumulate) and WGRAD of one case at the current fraction against
    the shared fp64 reference."""
    f = cf.FAMILY[name]
    C, B, cin, h, cout = case
    k, s, p = f.k, f.stride, f.pad
    pr = cf.conv_problem(name, case)
    oh, counts = pr["oh"], pr["counts"]
    cd = counts.to(DEV)
    xd, wd, bd, dyd = (pr[n].to(DEV) for n in ("x", "w", "bias", "dy"))
    y = torch.zeros(C, B, cout, oh, oh, device=DEV)
    dx = torch.zeros(C, B, cin, h, h, device=DEV)
    acc = pr["base"].to(DEV)
    dw = torch.zeros(C, cout, cin, k, k, device=DEV)
    db = torch.zeros(C, cout, device=DEV)
    if fwd:
        ops.conv2d_fwd(xd, wd, bd, y, C, B, cin, h, h, cout, k, s, p, counts=cd)
    if dgrad:
        ops.conv2d_dgrad(dyd, wd, dx, C, B, cin, h, h, cout, k, s, p, counts=cd)
        ops.conv2d_dgrad(dyd, wd, acc, C, B, cin, h, h, cout, k, s, p, counts=cd,
                         accumulate=True)
    if wgrad:
        ops.conv2d_wgrad(xd, dyd, dw, db, C, B, cin, h, h, cout, k, s, p, counts=cd)
    torch.cuda.synchronize()
    for z in range(C):
        n = int(counts[z])
        yr, dxr, dwr, dbr = pr["ref"][z]
        where = f"{tag}{name} {case} z={z} (count {n})"
        if fwd:
            _eq(y[z, :n], yr, f"fwd {where}")
        if dgrad:
            _eq(dx[z, :n], dxr, f"dgrad {where}")
            _eq(acc[z, :n], dxr + pr["base"][z, :n].double(), f"dgrad accumulate {where}")
            assert torch.equal(acc[z, n:].cpu(), pr["base"][z, n:]), f"dgrad tail {where}"
        if wgrad:
            _eq(dw[z], dwr, f"wgrad {where}")
            _eq(db[z], dbr, f"bgrad {where}")


@gpu
@pytest.mark.parametrize("fraction", cf.FRACTIONS)
@pytest.mark.parametrize("name,case", cf.CONV_CASES, ids=CONV_IDS)
def test_conv_fill_exact(name, case, fraction):
    with _Fill(fraction):
        _run_conv(name, case, tag=f"fill {fraction} ")


@gpu
@pytest.mark.parametrize("fraction", cf.FRACTIONS)
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", S2_CASES, ids=cf.case_id)
def test_dgrad_s2_shortcut_fill_exact(case, accumulate, fraction):
    """fh_conv2d_dgrad_s2_shortcut (3x3/s2 DGRAD + the 1x1/s2 projection shortcut's in one
    launch) == the fp64 sum of both input gradients (+ the prior dx when accumulating);
    images past a client's count keep their prior values."""
    C, B, cin, h, cout = case
    pr = cf.conv_problem("s2_3x3", case)
    sc = cf.shortcut_problem(case)
    counts = pr["counts"]
    prior = pr["base"] if accumulate else torch.full_like(pr["base"], 9.0)
    dx = prior.to(DEV)
    with _Fill(fraction):
        assert ops.conv2d_dgrad_s2_shortcut(pr["dy"].to(DEV), pr["w"].to(DEV),
                                            sc["dy_sc"].to(DEV), sc["w_sc"].to(DEV), dx, C, B,
                                            cin, h, h, cout, counts=counts.to(DEV),
                                            accumulate=accumulate)
    torch.cuda.synchronize()
    for z in range(C):
        n = int(counts[z])
        ref = pr["ref"][z][1] + sc["ref"][z]
        if accumulate:
            ref = ref + prior[z, :n].double()
        _eq(dx[z, :n], ref, f"fill {fraction} {case} z={z} (count {n})")
        assert torch.equal(dx[z, n:].cpu(), prior[z, n:]), f"tail z={z}"


@gpu
@pytest.mark.parametrize("fraction", cf.FRACTIONS)
@pytest.mark.parametrize("case", cf.LINEAR_CASES, ids=LIN_IDS)
def test_linear_fill_exact(case, fraction):
    """linear_fwd (with and without ReLU), linear_dgrad, linear_wgrad and linear_bwd_fused
    (plain, and with a fixed keep-mask at p_drop = 0.5: dx * mask * 2, still exact)."""
    C, B, in_f, out_f = case
    pr = cf.linear_problem(case)
    counts = pr["counts"]
    cd = counts.to(DEV)
    xd, wd, bd, dyd, md = (pr[n].to(DEV) for n in ("x", "w", "bias", "dy", "mask"))
    z_ = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    y, yrelu, dx = z_(C, B, out_f), z_(C, B, out_f), z_(C, B, in_f)
    dw, db = z_(C, out_f, in_f), z_(C, out_f)
    dwf, dbf, dxf = z_(C, out_f, in_f), z_(C, out_f), z_(C, B, in_f)
    dwm, dbm, dxm = z_(C, out_f, in_f), z_(C, out_f), z_(C, B, in_f)
    with _Fill(fraction):
        ops.linear_fwd(xd, wd, bd, y, C, B, in_f, out_f, counts=cd)
        ops.linear_fwd(xd, wd, bd, yrelu, C, B, in_f, out_f, relu=True, counts=cd)
        ops.linear_dgrad(dyd, wd, dx, C, B, in_f, out_f, counts=cd)
        ops.linear_wgrad(xd, dyd, dw, db, C, B, in_f, out_f, counts=cd)
        fused = ops.linear_bwd_fused(xd, dyd, wd, dwf, dbf, dxf, C, B, in_f, out_f, counts=cd)
        masked = ops.linear_bwd_fused(xd, dyd, wd, dwm, dbm, dxm, C, B, in_f, out_f, mask=md,
                                      p_drop=0.5, counts=cd)
    torch.cuda.synchronize()
    # the fused kernel covers batch <= 32, in_f % 32 == 0, out_f % 32 == 0 (ops.linear_bwd_fused)
    assert fused == masked == (in_f % 32 == 0 and out_f % 32 == 0)
    for z in range(C):
        n = int(counts[z])
        yr, dxr, dwr, dbr = pr["ref"][z]
        where = f"fill {fraction} {case} z={z} (count {n})"
        _eq(y[z, :n], yr, f"linear fwd {where}")
        _eq(yrelu[z, :n], torch.relu(yr), f"linear fwd relu {where}")
        _eq(dx[z, :n], dxr, f"linear dgrad {where}")
        _eq(dw[z], dwr, f"linear wgrad {where}")
        _eq(db[z], dbr, f"linear bgrad {where}")
        if fused:
            _eq(dxf[z, :n], dxr, f"fused dx {where}")
            _eq(dwf[z], dwr, f"fused dw {where}")
            _eq(dbf[z], dbr, f"fused db {where}")
            _eq(dxm[z, :n], dxr * pr["mask"][z, :n].double() * 2.0, f"fused masked dx {where}")
            _eq(dwm[z], dwr, f"fused masked dw {where}")
            _eq(dbm[z], dbr, f"fused masked db {where}")


# ------------------------------------------------------------------ no-workspace fallback
# One case per FWD / DGRAD runner whose plan splits at the fraction used (asserted through the
# size query): a caller of the C ABI may pass no workspace, or too small a one, and gets the
# single-pass launch (include/fedhip.h).  ops.py always passes the queried size.
FALLBACK = [
    # runner, family, case, fraction, operations that split there
    ("run_mn", "igemm3x3", (1, 3, 32, 14, 64), 1.0, ("fwd", "dgrad")),
    ("run_dgrad_s2", "s2_1x1", (8, 3, 64, 32, 128), 1.0, ("dgrad",)),
    ("run_dconv", "direct3x3", (1, 32, 32, 32, 32), 1.0, ("fwd", "dgrad")),
    ("run_dconv_dgrad_s2", "s2_3x3", (1, 6, 32, 16, 64), 1.0, ("fwd", "dgrad")),
]


def _splits_there(name, case, op):
    f = cf.FAMILY[name]
    need = cf.conv_query(_lib.load(), op, case, f.k, f.stride, f.pad)
    return need > cf.conv_no_split_bytes(op, case, f.k, f.stride, f.slab_wgrad)


@gpu
@pytest.mark.parametrize("runner,name,case,fraction,split_ops", FALLBACK,
                         ids=[r[0] for r in FALLBACK])
def test_no_workspace_falls_back_to_single_pass(monkeypatch, runner, name, case, fraction,
                                                split_ops):
    monkeypatch.setattr(ops, "_ws_for", lambda fn_name, device, *args: (None, 0))
    with _Fill(fraction):
        for op in split_ops:
            assert _splits_there(name, case, op), (runner, op)
        _run_conv(name, case, fwd="fwd" in split_ops, dgrad="dgrad" in split_ops, wgrad=False,
                  tag=f"no workspace, {runner}: ")


@gpu
def test_short_workspace_falls_back_to_single_pass(monkeypatch):
    """A workspace one byte smaller than the query disables the split as a missing one does."""
    def short(fn_name, device, *args):
        need = getattr(_lib.load(), fn_name)(*args)
        assert need > 0
        return torch.empty(need, dtype=torch.uint8, device=device), need - 1
    monkeypatch.setattr(ops, "_ws_for", short)
    _run_conv("direct3x3", (1, 32, 32, 32, 32), dgrad=False, wgrad=False, tag="short workspace: ")


@gpu
@pytest.mark.parametrize("name,case", [("direct3x3", (1, 32, 32, 32, 32)),
                                       ("rgb", (1, 9, 3, 32, 32)),
                                       ("s2_3x3", (1, 6, 32, 16, 64)),
                                       ("c1", (1, 17, 1, 28, 32)),
                                       ("igemm3x3", (2, 3, 32, 14, 64))],
                         ids=["quadrant", "rgb", "s2", "c1", "igemm"])
def test_wgrad_refuses_a_missing_workspace(monkeypatch, name, case):
    """WGRAD has no single-pass fallback: a split plan without its slab is FH_E_INVALID
    ("workspace 0 < need"), raised on the host before any launch; dW / db stay untouched."""
    f = cf.FAMILY[name]
    C, B, cin, h, cout = case
    pr = cf.conv_problem(name, case)
    assert cf.conv_query(_lib.load(), "wgrad", case, f.k, f.stride, f.pad) > 0
    monkeypatch.setattr(ops, "_ws_for", lambda fn_name, device, *args: (None, 0))
    dw = torch.full((C, cout, cin, f.k, f.k), 7.0, device=DEV)
    db = torch.full((C, cout), 7.0, device=DEV)
    with pytest.raises(_lib.FedHipError, match=r"rc=-1\).*conv2d_wgrad: workspace 0 < "):
        ops.conv2d_wgrad(pr["x"].to(DEV), pr["dy"].to(DEV), dw, db, C, B, cin, h, h, cout, f.k,
                         f.stride, f.pad, counts=pr["counts"].to(DEV))
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((db == 7.0).all())
