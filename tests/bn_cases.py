"""Shapes, client counts and inputs of the BatchNorm reference tests — TEST HELPER (not a test).

Shared by tests/test_bn_ref_cpu.py (which checks the input conditions on the CPU) and
tests/test_bn_tiles_gpu.py (which runs the kernels).  Each case is built once and cached;
nothing here runs project code.

Every case carries two ill-conditioned channels:
    channel 0   constant 0.3: variance exactly 0, invstd = 1/sqrt(eps)
    channel 1   mean 100, standard deviation 0.01
Channel 1's y / dx / dgamma cannot meet an absolute fp32 bound (fl(mean) alone is off by up to
2^-18, 4e-4 standard deviations); the GPU tests bound them by the error of the same
computation in float32 on the CPU (Case.y_f32 / Case.bwd_f32 below).
"""
from __future__ import annotations

import functools

import torch

import bn_ref

ILL = 1  # the mean-100 channel

# (clients, batch, C, H, W)
SHAPES = [
    (1, 2, 5, 2, 2),       # SP = 1; C % 4 != 0: the c >= C guard of the 4-channel finalize
    (3, 8, 5, 3, 5),       # HW = 15: scalar path
    (2, 9, 8, 7, 7),       # HW = 49
    (4, 63, 4, 16, 16),    # SP = 63 / 64 / 65: merge()'s 64-lane stride
    (4, 64, 4, 16, 16),
    (4, 65, 4, 16, 16),
    (1, 32, 32, 32, 32),   # production shapes
    (3, 32, 64, 16, 16),
    (5, 32, 128, 8, 8),
    (3, 4, 5, 1, 1),       # HW = 1: a client with one image has n == 1
    (1, 57, 4, 6, 6),      # 2052 elements: the slice ends 4 past a 2048 boundary; W % 4 != 0
    (2, 5, 8, 6, 6),       # pooled scalar path, ragged
    (2, 63, 4, 32, 32),    # pooled grid: SP = 63 / 64 / 65 tiles of 256 pooled elements
    (2, 64, 4, 32, 32),
    (2, 65, 4, 32, 32),
]
EVAL_SHAPES = [(3, 8, 5, 3, 5), (4, 64, 4, 16, 16)]


def count_sets(nc, B):
    """Client counts: the full batch, a ragged value, 1, and 0 whenever there are >= 2 clients."""
    r = max(1, (B * 5) // 8)
    if nc == 1:
        sets = [[B], [r], [1]]
    elif nc == 2:
        sets = [[B, 0], [r, 1]]
    elif nc == 3:
        sets = [[B, r, 0], [1, 0, r]]
    else:
        sets = [[B, r, 1, 0] + [max(1, B - 3 - k) for k in range(nc - 4)]]
    out = []
    for s in sets:
        if s not in out:
            out.append(s)
    return out


CASES = [(s, tuple(c)) for s in SHAPES for c in count_sets(s[0], s[1])]
POOL_CASES = [(s, c) for s, c in CASES if s[3] % 2 == 0 and s[4] % 2 == 0]
EVAL_CASES = [(s, c) for s, c in CASES if s in EVAL_SHAPES]


def case_id(case):
    s, c = case
    return "x".join(map(str, s)) + "-n" + ".".join(map(str, c))


def geometry(nc, B, C, HW):
    """Slice count S and slice length of the (client, channel) reductions — mirrors the
    kernels' launch geometry ONLY to assert which branches a shape reaches."""
    nmax = B * HW
    want = -(-2048 // (C * max(nc, 1)))
    want = max(1, min(want, max(1, nmax // 2048)))
    chunk = -(-(-(-nmax // want)) // 4) * 4
    return -(-nmax // chunk), chunk


def slice_lengths(shape, counts):
    """Lengths of the non-empty slices of every client."""
    nc, B, C, H, W = shape
    S, chunk = geometry(nc, B, C, H * W)
    out = []
    for n in counts:
        m = n * H * W
        out += [min(m, (s + 1) * chunk) - s * chunk for s in range(S) if s * chunk < m]
    return out


def _batch_norm(x, w, b):
    """F.batch_norm in train mode; the operator itself, because the functional wrapper
    refuses a single value per channel (a client with one 1x1 image)."""
    return torch.batch_norm(x, w, b, None, None, True, bn_ref.MOMENTUM, bn_ref.EPS, False)


class Case:
    """Inputs (fp32, CPU) and fp64 reference statistics of one (shape, counts)."""

    def __init__(self, shape, counts):
        nc, B, C, H, W = shape
        self.shape, self.counts = shape, counts
        poolable = H % 2 == 0 and W % 2 == 0
        g = torch.Generator().manual_seed(1000 * sum(shape) + 10 * sum(counts))
        x = torch.randn(nc, B, C, H, W, generator=g) * 1.5 + 0.3
        x[:, :, 0] = 0.3
        x[:, :, ILL] = 100.0 + 0.01 * torch.randn(nc, B, H, W, generator=g)
        gamma = torch.rand(nc, C, generator=g) + 0.5
        gamma[:, 2::3] *= -1          # negative scales: the ReLU mask is not monotone in x
        # |beta| >= 0.05: the constant channel's pre-activation IS beta, out of the margin
        beta = (0.05 + 0.3 * torch.rand(nc, C, generator=g))
        beta *= torch.where(torch.rand(nc, C, generator=g) < 0.5, -1.0, 1.0)
        beta[:, ILL] = beta[:, ILL].abs()
        # the constant channel: ReLU output all zero (every window decided) where the shape
        # can be pooled, alternating sign otherwise
        beta[:, 0] = -beta[:, 0].abs()
        if not poolable:
            beta[1::2, 0] *= -1
        self.gamma, self.beta = gamma, beta
        self.rmean0 = torch.randn(nc, C, generator=g) * 0.1
        self.rvar0 = torch.rand(nc, C, generator=g) + 0.5
        self.res = torch.randn(nc, B, C, H, W, generator=g)
        self.dy = torch.randn(nc, B, C, H, W, generator=g)
        self.dpool = torch.randn(nc, B, C, H // 2, W // 2, generator=g)
        self.pmask = (torch.rand(nc, B, C, H // 2, W // 2, generator=g) < 0.5).to(torch.uint8)
        self.moved = 0
        for z in range(nc):
            self.moved += bn_ref.nudge_preact(x[z], counts[z], gamma[z], beta[z])
        self.x = x
        self.stats = [bn_ref.train_stats(x[z], gamma[z], beta[z], self.rmean0[z], self.rvar0[z],
                                         counts[z]) for z in range(nc)]

    # ---- fp64 reference
    def y_ref(self, z, relu, res):
        n, st = self.counts[z], self.stats[z]
        return bn_ref.apply(self.x[z, :n], st.scale, st.shift, self.res[z, :n] if res else None,
                            relu)

    def pool_ref(self, z, mask, p_drop):
        """(pooled y, argmax code, near-tie windows) of relu(bn(x)) for client z."""
        n, st = self.counts[z], self.stats[z]
        v = self.y_ref(z, True, False)
        y, idx = bn_ref.pool_fwd(v, None if mask is None else mask[z, :n], p_drop)
        near = bn_ref.near_tie_windows(v, bn_ref.tie_margin(self.x[z, :n], st.scale, st.shift))
        return y, idx, near

    # ---- the same computation in float32 on the CPU (F.batch_norm), for the ILL channel
    def y_f32(self, z, relu, res):
        n = self.counts[z]
        y = _batch_norm(self.x[z, :n], self.gamma[z], self.beta[z])
        if res:
            y = y + self.res[z, :n]
        return torch.relu(y) if relu else y

    def bwd_f32(self, z, g):
        """dx, dgamma of F.batch_norm in float32 for the output gradient g [n, C, H, W]."""
        n = self.counts[z]
        x = self.x[z, :n].clone().requires_grad_(True)
        w = self.gamma[z].clone().requires_grad_(True)
        _batch_norm(x, w, self.beta[z]).backward(g.float())
        return x.grad, w.grad


@functools.lru_cache(maxsize=None)
def build(shape, counts):
    return Case(shape, counts)


# ---- the float32 error of y on the mean-100 channel, measured on the CPU
#
# F.batch_norm in float32 evaluates x*alpha + beta' with beta' = beta - fl(mean)*alpha, the
# kernels' formulation.  On the mean-100 channel |beta'| = |shift| ~ 1e4 cancels x*alpha, so
# the error of every y of one (client, channel) is set by TWO roundings shared by all its
# elements: fl(mean) (up to 2^-24 |mean| alpha) and fl(beta') (up to 2^-24 |shift|).  The
# largest error of one client is therefore one draw from [0, ~1] ulp of its shift, not a
# statistic over its elements, and the ratio of two such draws is unbounded: F.batch_norm on
# the same input in channels_last (same arithmetic, another summation order) exceeds four
# times the contiguous result for 12 of the 48 clients below.  The float32 error is
# measured over the whole population instead, each client's error in units of one ulp of its
# own shift, which makes the draws comparable across shapes and counts.
def ill_unit(c, z):
    """One fp32 ulp of client z's shift on the mean-100 channel, as a bound: 2^-23 |shift|."""
    return 2.0 ** -23 * abs(c.stats[z].shift[ILL].item())


def ill_units(c, z, y, ref, gain=1.0):
    """Largest |y - ref| of client z on the mean-100 channel in ulps of its shift (times gain,
    the exact factor a dropout keep applies after the affine)."""
    return (y[:, ILL].double() - ref[:, ILL]).abs().max().item() / (gain * ill_unit(c, z))


@functools.lru_cache(maxsize=None)
def cpu_fp32_y_units(relu, res):
    """F.batch_norm in float32 against fp64, largest over every client of every case."""
    worst = 0.0
    for case in CASES:
        c = build(*case)
        for z, n in enumerate(c.counts):
            if n:
                worst = max(worst, ill_units(c, z, c.y_f32(z, relu, res), c.y_ref(z, relu, res)))
    return worst


@functools.lru_cache(maxsize=None)
def cpu_fp32_pool_units(drop):
    """The 2x2 max-pool (with the keep mask at p = 0.5 if drop) of relu(F.batch_norm) in
    float32 against fp64, largest over every client of every poolable case."""
    p = 0.5 if drop else 0.0
    worst = 0.0
    for case in POOL_CASES:
        c = build(*case)
        for z, n in enumerate(c.counts):
            if n:
                m = c.pmask[z, :n] if drop else None
                q32 = bn_ref.pool_fwd(c.y_f32(z, True, False), m, p)[0]
                q64 = bn_ref.pool_fwd(c.y_ref(z, True, False), m, p)[0]
                worst = max(worst, ill_units(c, z, q32, q64, 1.0 / (1.0 - p)))
    return worst
