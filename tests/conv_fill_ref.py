"""Case tables, operands and fp64 references of the fill-fraction sweep — TEST HELPER (not a
test).

tests/test_conv_fill_gpu.py runs every conv / linear kernel family at the four fill fractions
fedhip/lanes.py deploys (0.25 a lone outlier client, 0.5, 0.75 the widest lane, 1.0 a single
lane) and at the lane widths of the KT cut [0, 1, 9, 32] (1, 8-9 and 23 clients, plus a small
middle lane of 2-3).  Operands are integers in [-2, 2], so every product and every partial sum
of any split plan is exact in fp32 and the result must equal the fp64 reference bit for bit.

A family is one conv geometry (k, stride, pad) and the kernels its shapes reach; a case is
(nclients, batch, cin, h, cout) on square maps.  Linear cases are (nclients, batch, in_f,
out_f).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

FRACTIONS = (0.25, 0.5, 0.75, 1.0)
EXACT_LIMIT = 1 << 24  # integers of smaller magnitude are exact in fp32
VMAX = 2               # |x|, |w|, |bias|, |dy| <= VMAX
BASE_MAX = 3           # |prior dx| of an accumulate run


class Family:
    def __init__(self, name, k, stride, pad, cases, split_ops, group=None, slab_wgrad=True):
        self.name, self.k, self.stride, self.pad = name, k, stride, pad
        self.cases = cases
        self.split_ops = split_ops    # operations whose kernels have a split path here
        self.group = group or name    # the coverage guards run per group
        self.slab_wgrad = slab_wgrad  # False: the unsplit WGRAD writes dW in place (igemm)


# The first cases of every family are the small shapes that reach each kernel's split logic.
# Most of them sit so far below the planners' workgroup targets that every fraction gives the
# same, fully split plan (the caps: kDconvMaxSplits, one stage or four K-steps per split), so
# each family also carries cases "on the edge": tiles x clients close to fill(target), where
# the want = ceil(fill(target) / tiles) term differs between fractions, and one case whose
# plan cannot split.  The comments name the planner term that makes the difference.
FAMILIES = [
    # direct FWD / DGRAD (dconv_kernel, split over reduction channels) and the quadrant-wave
    # WGRAD (dwgrad_q_kernel, split over 128-pixel stages): cin % 32 == 0, cout % 32 == 0.
    # (2, 5, 64, 8, 64): 5 * 64 pixels = 2.5 stages, the last stage half full.
    Family("direct3x3", 3, 1, 1, [
        (1, 32, 32, 32, 32), (3, 7, 32, 16, 64), (2, 5, 64, 8, 64), (8, 4, 64, 16, 32),
        (23, 3, 32, 8, 32),
        # plan_dconv: 2 pixel tiles x 4 (FWD: cout / 32; DGRAD: cin / 32) x 23 = 184 blocks
        # against fill(kDconvSplitBelow) = 128 / 256 / 384 / 512 and want = fill(1024) / 184
        # = 2 / 3 / 4: unsplit, 2, 4 and 4 splits of the 32 reduction channels
        (23, 5, 32, 8, 128), (23, 5, 128, 8, 32),
        # plan_dwq: 3 tiles, 88 stages: want = fill(1024) / 3 = 86 at 0.25 (2 stages per
        # split, 44 splits) and >= 88 above (one stage per split)
        (1, 11, 96, 32, 32),
        # plan_dwq: 2 * 64 pixels are ONE stage (nst = 1 caps the splits): dW written directly
        (2, 2, 32, 8, 32)],
           ("fwd", "dgrad", "wgrad")),
    # RGB first layer: dconv_wgrad_small_kernel.  Its FWD has 3 reduction channels, one
    # channel chunk (plan_dconv: chunks == 1), so only DGRAD and WGRAD can split.
    Family("rgb", 3, 1, 1, [
        (1, 9, 3, 32, 32), (8, 2, 3, 32, 64),
        # plan_dwgrad_small: 16 tiles, 9 stages: want = fill(512) / 16 = 8 at 0.25 (5 splits
        # of 2 stages, the last one short) and 9 above
        (8, 17, 3, 8, 64),
        # plan_dconv (DGRAD, 32 reduction channels): 8 x 1 x 23 = 184 blocks, as direct3x3
        (23, 29, 3, 8, 32),
        # plan_dwgrad_small: one stage, one split (the kernel still writes its slab)
        (2, 2, 3, 8, 32)],
           ("dgrad", "wgrad")),
    # 3x3 / s2 / p1: direct FWD (S = 2), direct DGRAD (dconv_dgrad_s2_kernel), 64 x 32-tile WGRAD
    Family("s2_3x3", 3, 2, 1, [
        (1, 6, 32, 16, 64), (3, 5, 32, 32, 64), (9, 3, 64, 16, 128),
        # plan_dconv (FWD): 1 x 8 x 23 = 184 blocks: unsplit at 0.25, then 3 and 4 splits
        (23, 1, 32, 16, 256),
        # plan_dconv_dgrad_s2: 23 blocks < fill(kDs2Fill) = 64 / 128 / 192 / 256, want =
        # fill / 23 = 3 / 6 / 9 / 12 capped at cout / 32 = 4; the parity-phase igemm plan the
        # query also covers moves too
        (23, 1, 32, 16, 128),
        # plan_dconv_dgrad_s2: 3 x 1 x 23 = 69 blocks >= fill(kDs2Fill) = 64 at 0.25: the
        # direct DGRAD kernel unsplit (every other case here splits it at all four
        # fractions), 2 splits (the cout / 32 cap) above
        (23, 3, 32, 32, 64),
        # plan_dwgrad_s2: 8 tiles, 3 stages per image pair: one split at 0.25, then 2 and 3
        (8, 3, 64, 16, 256)],
           ("fwd", "dgrad", "wgrad")),
    # 1x1 / s2 / p0: pw_s2_fwd_kernel (never splits), parity-phase igemm DGRAD, igemm WGRAD
    Family("s2_1x1", 1, 2, 0, [
        (1, 6, 32, 16, 64), (8, 3, 64, 32, 128),
        # plan_mn over 4 phases x 23 clients = 92 tiles, K = cout = 512 (up to 8 splits of 4
        # K-steps): unsplit at 0.25 (92 >= fill(192)), then want = fill(768) / 92 = 5 / 7 / 8.
        # With cout <= 256 every split plan of this family sits at the K / 64 cap.  Its WGRAD
        # (K = 3 * 64 pixels < 256) cannot split: dW written in place, no workspace.
        (23, 3, 32, 16, 512),
        # plan_wgrad: 9 tiles, K = 29 * 256 pixels: want = fill(2048) / 9 = 57 at 0.25
        # against the K / 128 = 58 cap above
        (9, 29, 32, 32, 64)],
           ("dgrad", "wgrad"), slab_wgrad=False),
    # single input channel: conv_c1_fwd_kernel (never splits; 9 products per output) and
    # conv_c1_wgrad_mfma_kernel (4-row stages)
    Family("c1", 3, 1, 1, [
        (1, 17, 1, 28, 32), (9, 3, 1, 16, 64), (23, 2, 1, 28, 32),
        # plan_c1_mfma: 84 stages, want = fill(1024) / 9 = 29 at 0.25 (28 splits of 3 stages)
        # against the nst / kC1MinSps = 42 cap above (2 stages); the size query is the larger
        # slab of this plan and plan_wgrad's (49 / 59 splits), which moves with it
        (9, 12, 1, 28, 32),
        # plan_c1_mfma: 2 stages, nst / kC1MinSps = 1 split (the kernel still writes its slab)
        (3, 1, 1, 8, 32)],
           ("wgrad",)),
    # implicit GEMM only: odd maps, 1x1 / s1, channel counts off the tiles
    Family("igemm3x3", 3, 1, 1, [
        (2, 3, 32, 14, 64), (1, 2, 96, 7, 40),
        # plan_mn: 11 pixel tiles x 8 clients = 88 tiles: unsplit at 0.25 (88 >= fill(192)),
        # want = fill(768) / 88 = 5 / 7 / 9 above
        (8, 27, 96, 7, 24), (8, 27, 32, 7, 64)],
           ("fwd", "dgrad", "wgrad"), group="igemm", slab_wgrad=False),
    Family("igemm1x1", 1, 1, 0, [
        (2, 5, 16, 7, 24), (23, 2, 24, 8, 40),
        # plan_wgrad: 23 tiles, K = 19 * 196 pixels: want = fill(2048) / 23 = 23 at 0.25
        # against the K / 128 = 29 cap above
        (23, 19, 16, 14, 24)],
           ("fwd", "dgrad", "wgrad"), group="igemm", slab_wgrad=False),
]
FAMILY = {f.name: f for f in FAMILIES}
CONV_CASES = [(f.name, c) for f in FAMILIES for c in f.cases]

LINEAR_CASES = [
    # (in_f / 128) * nclients = 128 against fill(256) = 64 / 128 / 192 / 256: linear_dgrad and
    # linear_bwd_fused change kernels inside the sweep
    (8, 9, 2048, 64),
    (1, 32, 2048, 512),
    (3, 17, 3136, 128),  # in_f % 128 != 0: never the four-tile form
    (23, 4, 512, 10),    # out_f off every tile: igemm DGRAD, skinny FWD / WGRAD
    # in_f % 32 != 0: implicit-GEMM FWD and DGRAD (plan_mn: 92 / 115 tiles against
    # fill(192), want = fill(768) / tiles), the only linear DGRAD with a split path
    (23, 4, 520, 512),
    # plan_lin_fwd (linear_fwd_skinny_kernel + its split epilogue): the cases above sit at the
    # kb / (kLfMinKb * 4) cap (4, 4, 6 and 1 splits at every fraction).  Here want =
    # ceil(fill(kLfTarget) / tiles) crosses below the cap: 8 x 23 = 184 tiles, cap 2: 1 / 2 /
    # 2 / 2 splits (and (in_f / 128) * nclients = 184 against fill(256) flips the DGRAD /
    # fused-backward kernel choice between 0.5 and 0.75); 16 x 23 = 368 tiles, cap 4:
    # 1 / 1 / 2 / 2 splits
    (23, 4, 1024, 256),
    (23, 4, 2048, 512),
]


def case_id(case):
    return "x".join(str(v) for v in case)


def out_hw(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def ragged_counts(nclients, batch):
    """Client 0 full, the others B - (3 i) % min(B, 7); with >= 3 clients the last has ONE
    image (a count of 1 ends inside the first tile / stage of every kernel)."""
    c = [batch - (3 * i) % min(batch, 7) for i in range(nclients)]
    if nclients >= 3:
        c[-1] = 1
    return torch.tensor(c, dtype=torch.int32)


def conv_magnitude_bounds(case, k, stride, pad):
    """Largest possible |value| of each conv result (and so of any partial sum of it):
    VMAX^2 per product times the reduction length, plus the bias, plus the base of an
    accumulate run; the fused stride-2 shortcut adds the 1x1 conv's cout products."""
    C, B, cin, h, cout = case
    oh = out_hw(h, k, stride, pad)
    prod = VMAX * VMAX
    return {
        "fwd": prod * cin * k * k + VMAX,
        "dgrad": prod * cout * k * k + BASE_MAX,
        "dgrad_shortcut": prod * cout * (k * k + 1) + BASE_MAX,
        "wgrad": prod * B * oh * oh,
        "bgrad": VMAX * B * oh * oh,
    }


def linear_magnitude_bounds(case):
    """As conv_magnitude_bounds; the dropout variant of the fused backward scales dx by 2."""
    C, B, in_f, out_f = case
    prod = VMAX * VMAX
    return {"fwd": prod * in_f + VMAX, "dgrad": 2 * prod * out_f, "wgrad": prod * B,
            "bgrad": VMAX * B}


def _ints(shape, g, lim=VMAX):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


_CONV_CACHE: dict = {}


def conv_problem(fam_name, case):
    """Operands and fp64 references of one conv case (computed once, shared by every test
    and fraction; callers must not modify them).  ref[z] = (y, dx, dw, db) over client z's
    first counts[z] images."""
    key = (fam_name, case)
    if key in _CONV_CACHE:
        return _CONV_CACHE[key]
    f = FAMILY[fam_name]
    C, B, cin, h, cout = case
    k, s, p = f.k, f.stride, f.pad
    oh = out_hw(h, k, s, p)
    g = torch.Generator().manual_seed(sum(case) + 1000 * k + s)
    pr = {
        "x": _ints((C, B, cin, h, h), g), "w": _ints((C, cout, cin, k, k), g),
        "bias": _ints((C, cout), g), "dy": _ints((C, B, cout, oh, oh), g),
        "base": _ints((C, B, cin, h, h), g, BASE_MAX), "counts": ragged_counts(C, B),
        "oh": oh, "ref": [],
    }
    for z in range(C):
        n = int(pr["counts"][z])
        xr = pr["x"][z, :n].double().requires_grad_(True)
        wr = pr["w"][z].double().requires_grad_(True)
        br = pr["bias"][z].double().requires_grad_(True)
        yr = F.conv2d(xr, wr, br, stride=s, padding=p)
        yr.backward(pr["dy"][z, :n].double())
        pr["ref"].append((yr.detach(), xr.grad, wr.grad, br.grad))
    _CONV_CACHE[key] = pr
    return pr


_SC_CACHE: dict = {}


def shortcut_problem(case):
    """The 1x1 / s2 projection shortcut beside an s2_3x3 case: w_sc, dy_sc and the fp64 input
    gradient of the shortcut alone per client (added to conv_problem's dx reference)."""
    if case in _SC_CACHE:
        return _SC_CACHE[case]
    C, B, cin, h, cout = case
    oh = h // 2
    g = torch.Generator().manual_seed(sum(case) + 77)
    pr = {"w_sc": _ints((C, cout, cin, 1, 1), g), "dy_sc": _ints((C, B, cout, oh, oh), g),
          "ref": []}
    counts = ragged_counts(C, B)
    for z in range(C):
        n = int(counts[z])
        xr = torch.zeros(n, cin, h, h, dtype=torch.float64, requires_grad=True)
        F.conv2d(xr, pr["w_sc"][z].double(), stride=2).backward(pr["dy_sc"][z, :n].double())
        pr["ref"].append(xr.grad)
    _SC_CACHE[case] = pr
    return pr


_LIN_CACHE: dict = {}


def linear_problem(case):
    """Operands and fp64 references of one linear case: ref[z] = (y, dx, dw, db), y before
    the ReLU; mask is a fixed keep-mask for the p_drop = 0.5 variant (dx * mask * 2)."""
    if case in _LIN_CACHE:
        return _LIN_CACHE[case]
    C, B, in_f, out_f = case
    g = torch.Generator().manual_seed(sum(case))
    pr = {
        "x": _ints((C, B, in_f), g), "w": _ints((C, out_f, in_f), g), "bias": _ints((C, out_f), g),
        "dy": _ints((C, B, out_f), g),
        "mask": torch.randint(0, 2, (C, B, in_f), generator=g).to(torch.uint8),
        "counts": ragged_counts(C, B), "ref": [],
    }
    for z in range(C):
        n = int(pr["counts"][z])
        xr = pr["x"][z, :n].double().requires_grad_(True)
        wr = pr["w"][z].double().requires_grad_(True)
        br = pr["bias"][z].double().requires_grad_(True)
        yr = F.linear(xr, wr, br)
        yr.backward(pr["dy"][z, :n].double())
        pr["ref"].append((yr.detach(), xr.grad, wr.grad, br.grad))
    _LIN_CACHE[case] = pr
    return pr


# ------------------------------------------------------------------ workspace size queries
def _align256(n):
    return (n + 255) // 256 * 256


def conv_no_split_bytes(op, case, k, stride, slab_wgrad=True):
    """What the size query of an unsplit plan returns (the slab layouts of include/fedhip.h,
    not the planners): FWD / DGRAD need nothing, except that every stride-2 DGRAD query
    reserves the parity-phase packed weights [client][cin * cout * k * k] in front of its
    slab; a direct WGRAD kernel's family reports one [client][cout * cin * k * k] slab with
    the bias partials [client][cout] behind it (256-B aligned), the implicit-GEMM WGRAD
    (slab_wgrad False) writes dW in place."""
    C, B, cin, h, cout = case
    if op == "fwd":
        return 0
    if op == "dgrad":
        return _align256(C * cin * cout * k * k * 4) if stride == 2 else 0
    return _align256(C * cout * cin * k * k * 4) + C * cout * 4 if slab_wgrad else 0


def conv_query(lib, op, case, k, stride, pad):
    C, B, cin, h, cout = case
    return int(getattr(lib, f"fh_conv2d_{op}_workspace")(C, B, cin, h, h, cout, k, k, stride, pad))


def linear_query(lib, op, case):
    return int(getattr(lib, f"fh_linear_{op}_workspace")(*case))


def sweep_sizes(lib, query):
    """{fraction: query()} with the calling thread's fill fraction set to each of FRACTIONS in
    turn, restored to 1.0 afterwards."""
    out = {}
    try:
        for fr in FRACTIONS:
            assert lib.fh_set_fill_fraction(fr) == 0
            out[fr] = query()
    finally:
        lib.fh_set_fill_fraction(1.0)
    return out
