"""tests/bn_ref.py against torch's own fp64 CPU operators (F.batch_norm, F.max_pool2d and
autograd), its edge branches against hand-computed values, and the input conditions of every
case tests/test_bn_tiles_gpu.py runs: no ReLU pre-activation inside the decision margin, at
most 0.5 % of the pooling windows excluded as near-ties."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_cases
import bn_ref


def _rand_client(seed, B=6, C=5, H=4, W=6):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, H, W, generator=g) * 1.7 + 0.4).double()
    gamma = (torch.rand(C, generator=g) + 0.5).double()
    gamma[1] *= -1
    beta = (torch.randn(C, generator=g) * 0.3).double()
    rm = (torch.randn(C, generator=g) * 0.1).double()
    rv = (torch.rand(C, generator=g) + 0.5).double()
    res = torch.randn(B, C, H, W, generator=g).double()
    dy = torch.randn(B, C, H, W, generator=g).double()
    return x, gamma, beta, rm, rv, res, dy


@pytest.mark.parametrize("n", [6, 4, 1])
@pytest.mark.parametrize("relu,residual", [(False, False), (True, False), (True, True),
                                           (False, True)])
def test_stats_apply_bwd_match_torch(n, relu, residual):
    x, gamma, beta, rm, rv, res, dy = _rand_client(n + 2 * relu + 4 * residual)
    st = bn_ref.train_stats(x, gamma, beta, rm, rv, n)
    y = bn_ref.apply(x[:n], st.scale, st.shift, res[:n] if residual else None, relu)
    xr = x[:n].clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rmt, rvt = rm.clone(), rv.clone()
    out = F.batch_norm(xr, rmt, rvt, gr, br, training=True, momentum=0.1, eps=1e-5)
    if residual:
        out = out + res[:n]
    if relu:
        out = F.relu(out)
    out.backward(dy[:n])
    tol = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(y, out.detach(), **tol)
    torch.testing.assert_close(st.rmean, rmt, **tol)
    torch.testing.assert_close(st.rvar, rvt, **tol)
    xc = x[:n].permute(1, 0, 2, 3).reshape(x.shape[1], -1)
    torch.testing.assert_close(st.mean, xc.mean(1), **tol)
    torch.testing.assert_close(st.var, xc.var(1, unbiased=False), **tol)
    torch.testing.assert_close(st.invstd, 1 / torch.sqrt(xc.var(1, unbiased=False) + 1e-5), **tol)
    g = dy[:n] * (y > 0) if relu else dy[:n]
    dx, dgamma, dbeta = bn_ref.bwd(g, x, st.mean, st.invstd, gamma, n)
    torch.testing.assert_close(dx, xr.grad, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(dgamma, gr.grad, rtol=1e-9, atol=1e-11)
    torch.testing.assert_close(dbeta, br.grad, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (8, 8)])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_pool_matches_torch(hw, p_drop):
    H, W = hw
    g = torch.Generator().manual_seed(H * 10 + W)
    v = torch.rand(3, 4, H, W, generator=g, dtype=torch.float64) + 0.1  # positive, no ties
    mask = (torch.rand(3, 4, H // 2, W // 2, generator=g) < 0.5).to(torch.uint8) if p_drop else None
    y, idx = bn_ref.pool_fwd(v, mask, p_drop)
    vr = v.clone().requires_grad_(True)
    q, flat = F.max_pool2d(vr, 2, 2, return_indices=True)
    code = ((flat // W) & 1) * 2 + ((flat % W) & 1)
    assert torch.equal(idx.long(), code)
    keep = 1.0 if mask is None else mask.double() / (1.0 - p_drop)
    torch.testing.assert_close(y, q.detach() * keep, rtol=0, atol=0)
    dq = torch.randn(q.shape, generator=g, dtype=torch.float64)
    (q * keep).backward(dq)
    assert torch.equal(bn_ref.pool_route(dq, idx, mask, p_drop, H, W), vr.grad)


def test_pool_ties_and_zero_windows():
    v = torch.tensor([[0.0, 0.0, 2.0, 2.0, 1.0, 3.0],
                      [0.0, 0.0, 1.0, 2.0, 3.0, 3.0]], dtype=torch.float64).reshape(1, 1, 2, 6)
    y, idx = bn_ref.pool_fwd(v)
    assert idx.flatten().tolist() == [0, 0, 1]     # four zeros -> 0; first of the tied maxima
    assert y.flatten().tolist() == [0.0, 2.0, 3.0]
    near = bn_ref.near_tie_windows(v, torch.tensor([1e-3], dtype=torch.float64))
    assert near.flatten().tolist() == [False, True, True]   # both-zero window is decided
    dq = torch.tensor([5.0, 7.0, 11.0], dtype=torch.float64).reshape(1, 1, 1, 3)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8).reshape(1, 1, 1, 3)
    r = bn_ref.pool_route(dq, idx, mask, 0.5, 2, 6)
    assert r.flatten().tolist() == [10.0, 0, 0, 0, 0, 22.0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("B,n,H,W", [(5, 3, 6, 6), (40, 40, 4, 4), (9, 0, 2, 2), (70, 33, 4, 4)])
def test_tiles_sum_to_whole_tensor_moments(B, n, H, W):
    g = torch.Generator().manual_seed(B + n)
    C = 3
    x = torch.randn(B, C, H, W, generator=g)
    x[n:] = float("nan")
    part = bn_ref.fwd_tiles(x, n)
    assert part.shape == (C, (B * H * W + 255) // 256, 2) and not torch.isnan(part).any()
    xs = x[:n].double().permute(1, 0, 2, 3).reshape(C, -1)
    torch.testing.assert_close(part[..., 0].sum(1), xs.sum(1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(part[..., 1].sum(1), (xs * xs).sum(1), rtol=1e-12, atol=1e-12)
    if n:  # tile t holds elements [256 t, 256 t + 256) of the img*HW + p stream
        assert part[0, 0, 0].item() == pytest.approx(xs[0, :256].sum().item(), rel=1e-12)
    used = (n * H * W + 255) // 256
    assert bool((part[:, used:] == 0).all())
    # backward pair, full-resolution and pooled grid
    dy = torch.randn(B, C, H, W, generator=g)
    dy[n:] = float("nan")
    mean = torch.randn(C, generator=g)
    bp = bn_ref.bwd_tiles(dy, x, mean, n)
    xc = xs - mean.double()[:, None]
    gs = dy[:n].double().permute(1, 0, 2, 3).reshape(C, -1)
    torch.testing.assert_close(bp[..., 0].sum(1), gs.sum(1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bp[..., 1].sum(1), (xc * gs).sum(1), rtol=1e-12, atol=1e-12)
    dq = torch.randn(B, C, H // 2, W // 2, generator=g)
    idx = torch.randint(0, 4, dq.shape, generator=g).to(torch.uint8)
    msk = (torch.rand(dq.shape, generator=g) < 0.5).to(torch.uint8)
    keep = torch.rand(B, C, H, W, generator=g) < 0.7
    pp = bn_ref.bwd_pool_tiles(dq, idx, msk, 0.5, x, keep, mean, n)
    assert pp.shape == (C, (B * (H // 2) * (W // 2) + 255) // 256, 2)
    full = bn_ref.pool_route(dq[:n], idx[:n], msk[:n], 0.5, H, W) * keep[:n]
    fs = full.permute(1, 0, 2, 3).reshape(C, -1)
    torch.testing.assert_close(pp[..., 0].sum(1), fs.sum(1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pp[..., 1].sum(1), (xc * fs).sum(1), rtol=1e-12, atol=1e-12)
    if n:  # pooled tile 0 of channel 0: the first 256 pooled elements' routed gradients
        ohw = (H // 2) * (W // 2)
        first = min(256, n * ohw)
        imgs = -(-first // ohw)
        w = sum(bn_ref._windows(full[:imgs, :1])).reshape(-1)[:first]
        assert pp[0, 0, 0].item() == pytest.approx(w.sum().item(), rel=1e-12, abs=1e-12)


def test_edge_branches_by_hand():
    gamma, beta = torch.tensor([2.0, -1.0]), torch.tensor([0.5, 0.25])
    rm, rv = torch.tensor([0.3, -0.2]), torch.tensor([1.5, 0.7])
    # n == 0: mean 0, invstd 0, running statistics unchanged, no dx
    x = torch.full((3, 2, 1, 1), float("nan"))
    st = bn_ref.train_stats(x, gamma, beta, rm, rv, 0)
    assert st.mean.tolist() == [0, 0] and st.invstd.tolist() == [0, 0]
    assert torch.equal(st.rmean, rm.double()) and torch.equal(st.rvar, rv.double())
    assert st.scale.abs().tolist() == [0, 0] and torch.equal(st.shift, beta.double())
    dx, dg, db = bn_ref.bwd(x, x, st.mean, st.invstd, gamma, 0)
    assert dx is None and dg.tolist() == [0, 0] and db.tolist() == [0, 0]
    # n == 1 (one image, HW == 1): variance 0, unbiased = biased, invstd = 1/sqrt(eps)
    x[0, :, 0, 0] = torch.tensor([4.0, -3.0])
    st = bn_ref.train_stats(x, gamma, beta, rm, rv, 1)
    assert st.mean.tolist() == [4.0, -3.0] and st.var.tolist() == [0, 0]
    inv = 1 / math.sqrt(1e-5)
    assert st.invstd.tolist() == pytest.approx([inv, inv], rel=1e-15)
    assert st.rmean.tolist() == pytest.approx([0.1 * 4 + 0.9 * float(rm[0]),
                                               0.1 * -3 + 0.9 * float(rm[1])], rel=1e-15)
    assert st.rvar.tolist() == pytest.approx([0.9 * float(rv[0]), 0.9 * float(rv[1])], rel=1e-15)
    assert st.scale.tolist() == pytest.approx([2 * inv, -inv], rel=1e-15)
    assert st.shift.tolist() == pytest.approx([0.5 - 8 * inv, 0.25 - 3 * inv], rel=1e-15)
    # two elements 1 and 3: mean 2, biased variance 1, unbiased 2
    x2 = torch.tensor([1.0, 3.0]).reshape(2, 1, 1, 1)
    st = bn_ref.train_stats(x2, gamma[:1], beta[:1], rm[:1], rv[:1], 2)
    assert st.mean.item() == 2.0 and st.var.item() == 1.0
    assert st.rvar.item() == pytest.approx(0.1 * 2.0 + 0.9 * 1.5, rel=1e-15)
    # dx of the two elements with g = (1, 0): dbeta 1, dot -1, hand-expanded formula
    g = torch.tensor([1.0, 0.0]).reshape(2, 1, 1, 1)
    dx, dg, db = bn_ref.bwd(g, x2, st.mean, st.invstd, gamma[:1], 2)
    i = 1 / math.sqrt(1 + 1e-5)
    k = -1 * i * i / 2
    assert db.item() == 1.0 and dg.item() == pytest.approx(-i, rel=1e-15)
    want = [((1 - 0.5) + k) * i * 2, ((0 - 0.5) - k) * i * 2]
    assert dx.flatten().tolist() == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("case", bn_cases.CASES, ids=bn_cases.case_id)
def test_input_conditions(case):
    """After nudging no pre-activation lies inside the ReLU margin (no element is excluded
    from any comparison); the near-tie windows excluded from the argmax comparison are at most
    0.5 % of a case's windows; the ill-conditioned channels are what they claim to be."""
    shape, counts = case
    c = bn_cases.build(shape, counts)
    nc, B, C, H, W = shape
    ties = windows = 0
    for z, n in enumerate(counts):
        assert bn_ref.min_preact_ratio(c.x[z], n, c.gamma[z], c.beta[z]) >= 1.0
        if n == 0:
            continue
        st = c.stats[z]
        assert st.var[0].item() == 0.0
        assert st.invstd[0].item() == pytest.approx(1 / math.sqrt(1e-5), rel=1e-15)
        assert abs(st.mean[1].item() - 100.0) < 0.02
        if n * H * W >= 64:
            assert 0.005 < math.sqrt(st.var[1].item()) < 0.02
        if case in bn_cases.POOL_CASES:
            _, _, near = c.pool_ref(z, None, 0.0)
            ties += int(near.sum())
            windows += near.numel()
    if windows:
        assert ties <= 0.005 * windows, (ties, windows)
    total = sum(counts) * C * H * W
    assert c.moved <= 0.05 * total + 8, (c.moved, total)   # the inputs stay what they were


def test_ill_channel_fp32_error_in_ulps_of_the_shift():
    """The float32 figure that bounds the kernels' y on the mean-100 channel
    (bn_cases.cpu_fp32_y_units / cpu_fp32_pool_units).  fl(mean) and fl(shift) each move
    every y of a client by at most half an ulp of its shift, the remaining roundings by
    2^-24 |y|: the largest error over all clients lies below 1.1 ulp, and with dozens of
    clients not far below it.  One client alone measures nothing: the same operator on the
    same input in channels_last exceeds four times the contiguous error for some client."""
    for relu, res in ((False, False), (True, False), (True, True), (False, True)):
        assert 0.4 < bn_cases.cpu_fp32_y_units(relu, res) < 1.1
    for drop in (False, True):
        assert 0.4 < bn_cases.cpu_fp32_pool_units(drop) < 1.1
    over = 0
    for shape, counts in bn_cases.CASES:
        c = bn_cases.build(shape, counts)
        for z, n in enumerate(counts):
            if n:
                ref = c.y_ref(z, False, False)
                xl = c.x[z, :n].contiguous(memory_format=torch.channels_last)
                yl = bn_cases._batch_norm(xl, c.gamma[z], c.beta[z])
                over += (bn_cases.ill_units(c, z, yl, ref)
                         > 4 * bn_cases.ill_units(c, z, c.y_f32(z, False, False), ref))
    assert over > 0
