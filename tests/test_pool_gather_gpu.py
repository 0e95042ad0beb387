"""fh_avgpool_fwd / fh_avgpool_bwd and fh_gather_batch against plain references
(tests/small_ref.py, pinned to torch's CPU operators by test_small_ref_cpu.py).

Average pool (one wave per plane, lanes stride the map by 64; the backward is elementwise):
* integer-valued inputs: every partial sum is exact in any order, so y is within 1 ulp of
  float32(sum / HW), and equal to it when HW is a power of two;
* normal inputs: |y - fp64| <= HW * 2^-24 * mean|x| per plane — HW - 1 fp32 additions and
  one division, each with relative error 2^-24 (the standard summation bound);
* backward: dx == dy[plane] * fl32(1 / HW) bit for bit (addressing: the e / HW plane index,
  counts, strides), and within 2^-22 relative of fp64 dy / HW (one rounding of the
  reciprocal, one of the product);
* <fwd(x), dy> == <x, bwd(dy)> in fp64 within the sum of the two bounds;
* maps of 1 .. 196 pixels (partial last wave, more than one stride step), and plane /
  element counts above the 2048-block grid cap (the grid-stride loops wrap).

Gather: a copy — x compared as int32 bit patterns (NaN payloads, -0.0, denormals must
survive), labels exact, repeated / reversed / first / last indices, an index row stride
larger than the batch, and the batch sizes at which the 4-way unrolled body does work in
every lane (> 2048 * 256 elements) and takes a second pass (> 4 x that).

Outputs sit in sentinel-filled wider buffers: rows past a client's count and the padding
between clients must come back bit for bit."""
import numpy as np
import pytest
import torch

import small_ref as sr
from fedhip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HWS = [1, 3, 16, 49, 63, 64, 65, 196]
CS = [1, 24, 256]
U = 2.0 ** -24
GRID_ELEMS = 2048 * 256  # elements one pass of the capped elementwise grid covers


def _pool_fwd(x, counts, C, HW):
    """x [nc, B, C, HW] (CPU) -> y [nc, B, C] (CPU), guards checked."""
    nc, B = x.shape[:2]
    xb, xv = sr.padded(nc, B * C * HW, torch.float32, DEV, pad=7)
    xv.copy_(x.reshape(nc, -1))
    yb, yv = sr.padded(nc, B * C, torch.float32, DEV)
    before = yb.clone()
    ops.avgpool_fwd(xv, yv, nc, B, C, HW, counts=torch.tensor(counts, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert sr.untouched_outside(yb, before, [n * C for n in counts])
    return yv.cpu().contiguous().view(nc, B, C)


def _pool_bwd(dy, counts, C, HW):
    """dy [nc, B, C] (CPU) -> dx [nc, B, C, HW] (CPU), guards checked."""
    nc, B = dy.shape[:2]
    db, dv = sr.padded(nc, B * C, torch.float32, DEV, pad=7)
    dv.copy_(dy.reshape(nc, -1))
    xb, xv = sr.padded(nc, B * C * HW, torch.float32, DEV)
    before = xb.clone()
    ops.avgpool_bwd(dv, xv, nc, B, C, HW, counts=torch.tensor(counts, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert sr.untouched_outside(xb, before, [n * C * HW for n in counts])
    return xv.cpu().contiguous().view(nc, B, C, HW)


def _check_fwd_integer(x, y, counts, HW):
    for z, n in enumerate(counts):
        ref = np.float32(x[z, :n].double().sum(dim=-1).numpy() / HW)
        got = y[z, :n].numpy()
        if HW & (HW - 1) == 0:
            assert np.array_equal(got, ref), z
        else:
            assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= sr.ulp32(ref)).all(), z


def _fwd_bound(x, HW):
    return HW * U * x.double().abs().mean(dim=-1)


def _check_fwd_normal(x, y, counts, HW):
    for z, n in enumerate(counts):
        err = (y[z, :n].double() - sr.avgpool_fwd(x[z, :n], HW)).abs()
        assert (err <= _fwd_bound(x[z, :n], HW)).all(), (z, err.max().item())


def _check_bwd(dy, dx, counts, HW):
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(HW), dtype=torch.float32)
    for z, n in enumerate(counts):
        want = (dy[z, :n] * inv).unsqueeze(-1).expand(-1, -1, HW)
        assert sr.same_bits(dx[z, :n], want), z
        ref = sr.avgpool_bwd(dy[z, :n], HW)
        assert ((dx[z, :n].double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all(), z


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_avgpool_fwd(C, HW):
    nc, B = 3, 8
    counts = sr.ragged_counts(nc, B, C + HW)
    g = torch.Generator().manual_seed(C * 1000 + HW)
    xi = torch.randint(-8, 9, (nc, B, C, HW), generator=g).float()
    _check_fwd_integer(xi, _pool_fwd(xi, counts, C, HW), counts, HW)
    xn = torch.randn(nc, B, C, HW, generator=g)
    _check_fwd_normal(xn, _pool_fwd(xn, counts, C, HW), counts, HW)


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_avgpool_bwd_and_adjoint(C, HW):
    nc, B = 3, 8
    counts = sr.ragged_counts(nc, B, C + HW + 1)
    g = torch.Generator().manual_seed(C * 1000 + HW + 1)
    x = torch.randn(nc, B, C, HW, generator=g)
    dy = torch.randn(nc, B, C, generator=g)
    dx = _pool_bwd(dy, counts, C, HW)
    _check_bwd(dy, dx, counts, HW)
    y = _pool_fwd(x, counts, C, HW)
    for z, n in enumerate(counts):
        lhs = (y[z, :n].double() * dy[z, :n].double()).sum().item()
        rhs = (x[z, :n].double() * dx[z, :n].double()).sum().item()
        bound = (dy[z, :n].double().abs() * _fwd_bound(x[z, :n], HW)).sum().item() + \
            (x[z, :n].double().abs() * (2.0 ** -22 * sr.avgpool_bwd(dy[z, :n], HW).abs())).sum().item()
        assert abs(lhs - rhs) <= bound, (z, lhs, rhs, bound)


def test_avgpool_fwd_grid_wraps():
    """More than 8192 planes: four planes per block, 2048 blocks at most."""
    nc, B, C, HW = 2, 40, 256, 4
    assert B * C > 8192
    counts = [40, 37]  # the second client's planes end inside the wrapped pass
    g = torch.Generator().manual_seed(1)
    xi = torch.randint(-8, 9, (nc, B, C, HW), generator=g).float()
    _check_fwd_integer(xi, _pool_fwd(xi, counts, C, HW), counts, HW)
    xn = torch.randn(nc, B, C, HW, generator=g)
    _check_fwd_normal(xn, _pool_fwd(xn, counts, C, HW), counts, HW)


def test_avgpool_bwd_grid_wraps():
    nc, B, C, HW = 2, 10, 256, 243
    counts = [10, 9]  # the second client's elements end inside the wrapped pass
    assert counts[1] * C * HW > GRID_ELEMS
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(nc, B, C, generator=g)
    _check_bwd(dy, _pool_bwd(dy, counts, C, HW), counts, HW)


# ------------------------------------------------------------------ fh_gather_batch
def _gather_case(E, B, counts, N, seed, with_labels=True):
    nc = len(counts)
    bits = sr.awkward_bits(N * E, seed).view(N, E)
    labels = torch.arange(N, dtype=torch.int64) * 7 - 3
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randint(0, N, (nc, B), generator=g)
    idx[0, :min(B, N)] = torch.arange(N - 1, -1, -1)[:min(B, N)]  # reversed, from the last sample
    idx[0, B - 1] = 0                                             # ... to the first
    if B >= 4:
        idx[nc - 1, :4] = torch.tensor([N - 1, N - 1, 0, 0])      # repeats of both ends
    ib, iv = sr.padded(nc, B, torch.int64, DEV, fill=0, pad=9)    # idx row stride > batch
    iv.copy_(idx)
    xb, xv = sr.padded(nc, B * E, torch.float32, DEV)
    yb, yv = sr.padded(nc, B, torch.int64, DEV, fill=-99, pad=4)
    xb0, yb0 = xb.clone(), yb.clone()
    data = bits.to(DEV).view(torch.float32)
    ops.gather_batch(data, labels.to(DEV) if with_labels else None, iv, xv,
                     yv if with_labels else None, E, nc, B,
                     counts=torch.tensor(counts, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert sr.untouched_outside(xb, xb0, [n * E for n in counts])
    assert sr.untouched_outside(yb, yb0, counts if with_labels else [0] * nc)
    got = xv.cpu().contiguous().view(torch.int32).view(nc, B, E)
    for z, n in enumerate(counts):
        wx, wy = sr.gather(bits, labels, idx[z, :n])
        assert torch.equal(got[z, :n], wx), z
        if with_labels:
            assert torch.equal(yv[z, :n].cpu(), wy), z


@pytest.mark.parametrize("E", [1, 3, 784, 3072, 3073])
def test_gather_batch(E):
    _gather_case(E, 13, sr.ragged_counts(3, 13, E), 29, E)


def test_gather_batch_without_labels():
    _gather_case(784, 13, sr.ragged_counts(3, 13, 4), 29, 5, with_labels=False)


@pytest.mark.parametrize("B,short", [(176, 173), (700, 690)])
def test_gather_batch_unrolled_lanes_and_second_pass(B, short):
    """176 x 3072 > 2048 * 256 elements: the unrolled lanes u >= 1 copy; 700 x 3072 > 4 x
    that: a second outer pass.  The second client's count ends inside that work."""
    E = 3072
    passes = 1 if B == 176 else 4
    assert B * E > passes * GRID_ELEMS and short * E > passes * GRID_ELEMS
    _gather_case(E, B, [B, short], 64, B)
