"""Depthwise 3x3 HIP kernels (csrc/dwconv.hip: fh_dwconv3x3_fwd / _dgrad / _wgrad) and the
pointwise / stem shapes LightweightMobileNet sends through the implicit-GEMM convolution.

Small-integer operands make every product and partial sum exact in fp32, so any summation
order gives the exact answer: the HIP results must equal the fp64 F.conv2d(groups=C) results
bit for bit.  The largest depthwise sum is 4 * 32 * 1024 < 2^24 (weight gradient, 32 images of
32x32), the largest pointwise sum 4 * 32 * 1024 as well.
"""
import pytest
import torch
import torch.nn.functional as F

from fedhip import ops
from fedhip._lib import FedHipError

pytestmark = pytest.mark.gpu
DEV = "cuda"

# clients, batch, C, h, stride
DW_CASES = [
    (1, 32, 32, 32, 1),
    (3, 17, 64, 32, 2),
    (2, 9, 128, 16, 1),
    (2, 8, 128, 16, 2),
    (5, 32, 256, 8, 1),
    (2, 13, 256, 8, 2),
    (32, 4, 16, 32, 1),
    (1, 1, 8, 8, 2),
    (2, 5, 8, 32, 1),
]
PACKED_CASE = (2, 9, 128, 16, 1)  # w / dW as views into [clients, Ppad] rows at an odd offset


def _counts(nc, B):
    return torch.tensor([B - (3 * z) % min(B, 7) for z in range(nc)], dtype=torch.int32)


def _reference(x, w, dy, counts, s):
    """fp64 forward / input gradient / weight gradient per client over its valid images."""
    out = []
    for z in range(x.shape[0]):
        n = int(counts[z])
        C = x.shape[2]
        xr = x[z, :n].double().requires_grad_(True)
        wr = w[z].double().reshape(C, 1, 3, 3).requires_grad_(True)
        yr = F.conv2d(xr, wr, None, stride=s, padding=1, groups=C)
        yr.backward(dy[z, :n].double())
        out.append((yr.detach(), xr.grad, wr.grad.reshape(C * 9)))
    return out


@pytest.mark.parametrize("case", DW_CASES)
def test_dwconv_exact_integer(case):
    nc, B, C, h, s = case
    ho = h // s
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randint(-2, 3, (nc, B, C, h, h), generator=g).float()
    w = torch.randint(-2, 3, (nc, C * 9), generator=g).float()
    dy = torch.randint(-2, 3, (nc, B, C, ho, ho), generator=g).float()
    counts = _counts(nc, B)
    cd = counts.to(DEV)
    ref = _reference(x, w, dy, counts, s)
    # images >= count hold NaN on the device: nothing valid may depend on them
    xd, dyd = x.to(DEV), dy.to(DEV)
    for z in range(nc):
        xd[z, int(counts[z]):] = float("nan")
        dyd[z, int(counts[z]):] = float("nan")
    if case == PACKED_CASE:
        Ppad = 64 * ((C * 9 + 37 + 63) // 64) + 64
        rows = torch.full((nc, Ppad), float("nan"), device=DEV)
        grows = torch.full((nc, Ppad), 7.0, device=DEV)
        wd, dw = rows[:, 37:37 + C * 9], grows[:, 37:37 + C * 9]
        wd.copy_(w)
        assert wd.data_ptr() % 8 == 4 and not wd.is_contiguous()
    else:
        wd, dw = w.to(DEV), torch.full((nc, C * 9), 7.0, device=DEV)
    y = torch.full((nc, B, C, ho, ho), 5.0, device=DEV)
    dx = torch.full((nc, B, C, h, h), 5.0, device=DEV)
    ops.dwconv3x3_fwd(xd, wd, y, nc, B, C, h, s, counts=cd)
    ops.dwconv3x3_dgrad(dyd, wd, dx, nc, B, C, h, s, counts=cd)
    ops.dwconv3x3_wgrad(xd, dyd, dw, nc, B, C, h, s, counts=cd)
    torch.cuda.synchronize()
    for z in range(nc):
        n = int(counts[z])
        yr, dxr, dwr = ref[z]
        assert torch.equal(y[z, :n].cpu().double(), yr), f"fwd z={z}"
        assert torch.equal(dx[z, :n].cpu().double(), dxr), f"dgrad z={z}"
        assert torch.equal(dw[z].cpu().double(), dwr), f"wgrad z={z}"
        # images past the count are left alone
        assert bool((y[z, n:] == 5.0).all()) and bool((dx[z, n:] == 5.0).all())
    if case == PACKED_CASE:  # nothing outside the dW view was written
        assert bool((grows[:, :37] == 7.0).all()) and bool((grows[:, 37 + C * 9:] == 7.0).all())


@pytest.mark.parametrize("case", [(3, 32, 32, 32, 1), (1, 32, 64, 32, 2), (2, 7, 256, 8, 1)])
def test_dwconv_wgrad_deterministic(case):
    """Random fp32 data: two calls give identical bits (split and unsplit sums), and the
    result is the fp64 sum to fp32 accuracy."""
    nc, B, C, h, s = case
    ho = h // s
    g = torch.Generator().manual_seed(11)
    x = torch.randn(nc, B, C, h, h, generator=g)
    dy = torch.randn(nc, B, C, ho, ho, generator=g)
    counts = _counts(nc, B)
    xd, dyd, cd = x.to(DEV), dy.to(DEV), counts.to(DEV)
    a = torch.zeros(nc, C * 9, device=DEV)
    b = torch.ones(nc, C * 9, device=DEV)
    ops.dwconv3x3_wgrad(xd, dyd, a, nc, B, C, h, s, counts=cd)
    ops.dwconv3x3_wgrad(xd, dyd, b, nc, B, C, h, s, counts=cd)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ref = _reference(x, torch.zeros(nc, C * 9), dy, counts, s)
    for z in range(nc):
        K = int(counts[z]) * ho * ho
        r = ref[z][2]
        # K products of N(0,1) pairs summed in fp32 blocks: error << eps * sqrt(K) * |sum|-scale
        tol = 4 * torch.finfo(torch.float32).eps * K ** 0.5 * (K ** 0.5)
        assert (a[z].cpu().double() - r).abs().max().item() <= tol


@pytest.mark.parametrize("case", [(2, 9, 32, 32, 1), (3, 5, 64, 16, 2), (1, 4, 8, 8, 2)])
def test_dwconv_dgrad_accumulate(case):
    """accumulate=True is dx += (the plain call's result), bit for bit; images past the count
    keep their values."""
    nc, B, C, h, s = case
    ho = h // s
    g = torch.Generator().manual_seed(3)
    w = torch.randn(nc, C * 9, generator=g).to(DEV)
    dy = torch.randn(nc, B, C, ho, ho, generator=g).to(DEV)
    base = torch.randn(nc, B, C, h, h, generator=g).to(DEV)
    cd = _counts(nc, B).to(DEV)
    dx = torch.zeros_like(base)
    ops.dwconv3x3_dgrad(dy, w, dx, nc, B, C, h, s, counts=cd)
    acc = base.clone()
    ops.dwconv3x3_dgrad(dy, w, acc, nc, B, C, h, s, counts=cd, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(acc, base + dx)


def test_dwconv_unsupported_shapes_return_errors():
    """h = 28, k != 3, C = 12: a returned error with a message, nothing launched."""
    nc, B = 1, 2

    def run(C, h, **kw):
        x = torch.zeros(nc, B, C, h, h, device=DEV)
        w = torch.zeros(nc, C * 25, device=DEV)
        y = torch.zeros(nc, B, C, h, h, device=DEV)
        for fn in (lambda: ops.dwconv3x3_fwd(x, w, y, nc, B, C, h, 1, **kw),
                   lambda: ops.dwconv3x3_dgrad(y, w, x, nc, B, C, h, 1, **kw),
                   lambda: ops.dwconv3x3_wgrad(x, y, w, nc, B, C, h, 1, **kw)):
            with pytest.raises(FedHipError, match="unsupported shape"):
                fn()

    run(16, 28)
    run(16, 16, k=5, pad=2)
    run(16, 16, k=1, pad=0)
    run(12, 16)
    # more clients than a launch grid holds: refused on the host, with a message
    x = torch.zeros(1, 1, 8, 8, 8, device=DEV)
    w = torch.zeros(1, 72, device=DEV)
    for fn in (lambda: ops.dwconv3x3_fwd(x, w, x, 70000, 1, 8, 8, 1),
               lambda: ops.dwconv3x3_dgrad(x, w, x, 70000, 1, 8, 8, 1),
               lambda: ops.dwconv3x3_wgrad(x, x, w, 70000, 1, 8, 8, 1)):
        with pytest.raises(FedHipError, match="too many clients"):
            fn()
    torch.cuda.synchronize()


# ---- the pointwise and stem layers on the implicit-GEMM / direct convolution ---------------
PW_CASES = [(32, 64, 32), (64, 128, 16), (128, 256, 8), (256, 512, 4), (16, 32, 32),
            (128, 256, 4)]


def _conv_exact(cin, cout, h, k, pad, nc=2, B=5):
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randint(-2, 3, (nc, B, cin, h, h), generator=g).float()
    wt = torch.randint(-2, 3, (nc, cout, cin, k, k), generator=g).float()
    dy = torch.randint(-2, 3, (nc, B, cout, h, h), generator=g).float()
    counts = torch.tensor([B, B - 2], dtype=torch.int32)
    cd = counts.to(DEV)
    y = torch.zeros(nc, B, cout, h, h, device=DEV)
    dx = torch.zeros(nc, B, cin, h, h, device=DEV)
    dw = torch.zeros(nc, cout, cin, k, k, device=DEV)
    xd, wd, dyd = x.to(DEV), wt.to(DEV), dy.to(DEV)
    ops.conv2d_fwd(xd, wd, None, y, nc, B, cin, h, h, cout, k, 1, pad, counts=cd)
    ops.conv2d_dgrad(dyd, wd, dx, nc, B, cin, h, h, cout, k, 1, pad, counts=cd)
    ops.conv2d_wgrad(xd, dyd, dw, None, nc, B, cin, h, h, cout, k, 1, pad, counts=cd)
    torch.cuda.synchronize()
    for z in range(nc):
        n = int(counts[z])
        xr = x[z, :n].double().requires_grad_(True)
        wr = wt[z].double().requires_grad_(True)
        yr = F.conv2d(xr, wr, None, stride=1, padding=pad)
        yr.backward(dy[z, :n].double())
        assert torch.equal(y[z, :n].cpu().double(), yr.detach()), f"fwd z={z}"
        assert torch.equal(dx[z, :n].cpu().double(), xr.grad), f"dgrad z={z}"
        assert torch.equal(dw[z].cpu().double(), wr.grad), f"wgrad z={z}"


@pytest.mark.parametrize("cin,cout,h", PW_CASES)
def test_pointwise_exact_integer(cin, cout, h):
    _conv_exact(cin, cout, h, 1, 0)


@pytest.mark.parametrize("cin,cout", [(3, 16), (1, 32)])
def test_stem_exact_integer(cin, cout):
    _conv_exact(cin, cout, 32, 3, 1)
