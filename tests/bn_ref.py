"""Plain fp64 reference of client-packed BatchNorm2d — TEST HELPER (not a test).

Written from the definitions with elementary torch arithmetic on the CPU; no project code.
Every function works on ONE client, over that client's n valid images only:

    train_stats   mean, biased variance, invstd = 1/sqrt(var + eps), running statistics
                  (momentum update, unbiased variance n/(n-1)), scale = invstd*gamma,
                  shift = beta - mean*scale.  No element (n == 0): mean 0, invstd 0, running
                  statistics unchanged.  One element: unbiased variance = biased variance.
    apply         y = [relu](x*scale + shift [+ res])
    bwd           dbeta = sum g, dgamma = sum((x-mean) g) * invstd,
                  dx = ((g - mean(g)) - (x-mean)*k) * invstd * gamma, k = dgamma*invstd/n;
                  no dx when n == 0
    pool_fwd      2x2 max of the ReLU output; argmax code (y&1)*2 + (x&1), first index wins
                  ties, four zeros give 0; then the supplied keep byte times 1/(1-p)
    pool_route    the pooled gradient back at full resolution (max-pool backward)
    fwd_tiles / bwd_tiles / bwd_pool_tiles
                  the per-tile fp64 partial sums part[C][SP][2] the tile kernels merge: tile t
                  of a channel covers elements [256 t, 256 t + 256) of the channel's
                  img*HW + p stream (pooled grid: img*HW/4 + pooled p), zeros past the count

tests/test_bn_ref_cpu.py pins these to F.batch_norm / F.max_pool2d and autograd in fp64.

Two helpers condition test inputs so that an fp32 kernel and this fp64 reference cannot take
different DECISIONS (a ReLU mask recomputed from x, a window argmax):

    relu_margin   per channel 2^-20 * (1 + |shift| + |scale| max|x|).  The kernel evaluates
                  x*alpha + beta' with alpha = fl(fl(invstd)*gamma), beta' = fl(beta -
                  fl(fl(mean)*alpha)): five roundings and two rounded inputs, each at most
                  2^-24 of a magnitude below |shift| + |scale| max|x|, together under
                  2^-21.5 of it.  The margin is more than twice that.
    tie_margin    per channel 2^-21 * (1 + |shift| + |scale| max|x|).  Two values of one
                  channel share alpha and beta', so their order can only change through the
                  roundings of the two products and the two sums (4 * 2^-24 of the magnitude,
                  2^-22); the margin is twice that.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

SENTINEL = -12345.678  # fp32 fill of every output buffer: a kernel never produces it
EPS = 1e-5
MOMENTUM = 0.1
TILE = 256


class Stats(NamedTuple):
    mean: torch.Tensor
    var: torch.Tensor
    invstd: torch.Tensor
    rmean: torch.Tensor
    rvar: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


def _bc(v):
    """[C] -> [1, C, 1, 1]"""
    return v.reshape(1, -1, 1, 1)


def _stream(t):
    """[n, C, h, w] -> [C, n*h*w]: a channel's elements in img*hw + p order."""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def train_stats(x, gamma, beta, rmean, rvar, n, eps=EPS, momentum=MOMENTUM):
    """x [batch, C, H, W], the first n images valid; the parameters [C]."""
    C = x.shape[1]
    g, b = gamma.double(), beta.double()
    rm, rv = rmean.double().clone(), rvar.double().clone()
    m = n * x.shape[2] * x.shape[3]
    if m == 0:
        mean = torch.zeros(C, dtype=torch.float64)
        var = torch.zeros(C, dtype=torch.float64)
        invstd = torch.zeros(C, dtype=torch.float64)
    else:
        xc = _stream(x[:n].double())
        mean = xc.sum(1) / m
        var = ((xc - mean[:, None]) ** 2).sum(1) / m
        invstd = 1.0 / torch.sqrt(var + eps)
        unb = var * m / (m - 1) if m > 1 else var
        rm = momentum * mean + (1.0 - momentum) * rm
        rv = momentum * unb + (1.0 - momentum) * rv
    scale = invstd * g
    shift = b - mean * scale
    return Stats(mean, var, invstd, rm, rv, scale, shift)


def apply(x, scale, shift, res=None, relu=False):
    """x [n, C, H, W] -> y fp64."""
    y = x.double() * _bc(scale.double()) + _bc(shift.double())
    if res is not None:
        y = y + res.double()
    if relu:
        y = torch.clamp_min(y, 0.0)
    return y


def bwd(g, x, mean, invstd, gamma, n):
    """g: the gradient at the BN output (ReLU mask already applied).  -> dx [n, C, H, W] (None
    when n == 0), dgamma [C], dbeta [C]."""
    C = x.shape[1]
    if n == 0:
        z = torch.zeros(C, dtype=torch.float64)
        return None, z, z.clone()
    g = g[:n].double()
    xc = x[:n].double() - _bc(mean.double())
    m = n * x.shape[2] * x.shape[3]
    dbeta = g.sum((0, 2, 3))
    dot = (xc * g).sum((0, 2, 3))
    inv = invstd.double()
    dgamma = dot * inv
    k = dot * inv * inv / m
    dx = ((g - _bc(dbeta / m)) - xc * _bc(k)) * _bc(inv) * _bc(gamma.double())
    return dx, dgamma, dbeta


def _windows(v):
    """[n, C, H, W] -> the four window members in argmax-code order, each [n, C, H/2, W/2]."""
    return (v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2])


def pool_fwd(v, mask=None, p_drop=0.0):
    """v: the ReLU output (>= 0).  -> pooled y fp64, argmax code uint8."""
    w = _windows(v.double())
    m = w[0].clone()
    idx = torch.zeros(m.shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        better = w[k] > m
        m = torch.where(better, w[k], m)
        idx = torch.where(better, torch.full_like(idx, k), idx)
    if mask is not None:
        m = torch.where(mask != 0, m * (1.0 / (1.0 - p_drop)), torch.zeros_like(m))
    return m, idx


def pool_route(dpool, pidx, pmask, p_drop, H, W):
    """dpool, pidx, pmask [n, C, H/2, W/2] -> the gradient at full resolution [n, C, H, W]."""
    g = dpool.double()
    if pmask is not None:
        g = torch.where(pmask != 0, g * (1.0 / (1.0 - p_drop)), torch.zeros_like(g))
    out = torch.zeros(g.shape[0], g.shape[1], H, W, dtype=torch.float64)
    for k in range(4):
        out[:, :, (k >> 1)::2, (k & 1)::2] = torch.where(pidx == k, g, torch.zeros_like(g))
    return out


def tiles_per_client(batch, elems_per_image):
    return (batch * elems_per_image + TILE - 1) // TILE


def _tile_sums(s, sp):
    """[C, m] stream -> [C, sp] sums over consecutive 256-element tiles (zero padded)."""
    s = torch.nn.functional.pad(s, (0, sp * TILE - s.shape[1]))
    return s.reshape(s.shape[0], sp, TILE).sum(-1)


def fwd_tiles(x, n):
    """x [batch, C, H, W] -> part [C, SP, 2] = (sum x, sum x^2) per tile, SP over the batch."""
    sp = tiles_per_client(x.shape[0], x.shape[2] * x.shape[3])
    s = _stream(x[:n].double())
    return torch.stack((_tile_sums(s, sp), _tile_sums(s * s, sp)), dim=-1)


def bwd_tiles(g, x, save_mean_f32, n):
    """(sum g, sum (x - mean) g) per tile of the full-resolution grid."""
    sp = tiles_per_client(x.shape[0], x.shape[2] * x.shape[3])
    gs = _stream(g[:n].double())
    xs = _stream(x[:n].double() - _bc(save_mean_f32.double()))
    return torch.stack((_tile_sums(gs, sp), _tile_sums(xs * gs, sp)), dim=-1)


def bwd_pool_tiles(dpool, pidx, pmask, p_drop, x, keep, save_mean_f32, n):
    """The same pair over tiles of 256 POOLED elements: each pooled element contributes its
    routed gradient at its argmax position, where keep (bool [batch, C, H, W], the ReLU mask)
    allows it."""
    H, W = x.shape[2], x.shape[3]
    sp = tiles_per_client(x.shape[0], (H // 2) * (W // 2))
    g = pool_route(dpool[:n], pidx[:n], None if pmask is None else pmask[:n], p_drop, H, W)
    g = torch.where(keep[:n], g, torch.zeros_like(g))
    xg = (x[:n].double() - _bc(save_mean_f32.double())) * g
    gw = sum(_windows(g))     # one non-zero member per window
    xw = sum(_windows(xg))
    return torch.stack((_tile_sums(_stream(gw), sp), _tile_sums(_stream(xw), sp)), dim=-1)


# ------------------------------------------------------------------ input conditioning
def _magnitude(x, scale, shift):
    C = x.shape[1]
    xmax = _stream(x.double().abs()).max(1).values if x.shape[0] else torch.zeros(C)
    return 1.0 + shift.double().abs() + scale.double().abs() * xmax


def relu_margin(x, scale, shift):
    """[C]; x [n, C, H, W] the valid images."""
    return 2.0 ** -20 * _magnitude(x, scale, shift)


def tie_margin(x, scale, shift):
    return 2.0 ** -21 * _magnitude(x, scale, shift)


def nudge_preact(x, n, gamma, beta, eps=EPS, max_iter=50):
    """Move, in place, every element of x[:n] (fp32) whose pre-activation x*scale + shift
    (train statistics of x[:n] itself) lies inside relu_margin to twice the margin, same
    sign; repeat until none does (moving elements moves the statistics).  -> elements moved."""
    moved = 0
    if n == 0:
        return moved
    for _ in range(max_iter):
        st = train_stats(x, gamma, beta, torch.zeros_like(gamma), torch.ones_like(gamma), n, eps)
        pre = apply(x[:n], st.scale, st.shift)
        mg = _bc(relu_margin(x[:n], st.scale, st.shift))
        bad = pre.abs() < mg
        if not bool(bad.any()):
            return moved
        moved += int(bad.sum())
        target = torch.where(pre >= 0, 2.0 * mg, -2.0 * mg)
        step = (target - pre) / _bc(st.scale)
        x[:n] = torch.where(bad, x[:n].double() + step, x[:n].double()).float()
    raise RuntimeError("nudge_preact did not converge")


def min_preact_ratio(x, n, gamma, beta, eps=EPS):
    """min |pre-activation| / relu_margin over x[:n] (inf when n == 0): >= 1 after nudging."""
    if n == 0:
        return float("inf")
    st = train_stats(x, gamma, beta, torch.zeros_like(gamma), torch.ones_like(gamma), n, eps)
    pre = apply(x[:n], st.scale, st.shift)
    return float((pre.abs() / _bc(relu_margin(x[:n], st.scale, st.shift))).min())


def near_tie_windows(v, margin):
    """v [n, C, H, W] the ReLU output, margin [C] -> bool [n, C, H/2, W/2]: windows whose two
    largest values are closer than the margin.  A window of four zeros is decided (code 0)."""
    w = torch.stack(_windows(v.double()), dim=-1)
    top = torch.topk(w, 2, dim=-1).values
    return (top[..., 0] > 0) & ((top[..., 0] - top[..., 1]) < _bc(margin))
