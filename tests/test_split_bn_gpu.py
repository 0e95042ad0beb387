"""r06: a split direct FWD conv's reduction inside the BatchNorm call after it
(fh_conv_bn_defer, splitbn.h): one launch per (channel, client) instead of
splitk_epilogue_kernel + bn_finalize / maxpool2_bnfin.  Against the same calls unarmed (the two
launches): every stored tensor bit for bit — the convolution output, the BN affine, saved and
running statistics, the pooled output / argmax / keep-mask — on split plans (one or a few
clients, ragged counts, with and without dropout); the launches really fused
(fh_conv_bn_defer_status); whole CIFAR10CNN rounds bit-identical with the fusion on and off,
eager and replayed (with one block per stage no ResNet FWD conv takes the fusion; its rounds are
test_fuse_bn_gpu.py's test_split_plan_rounds_eager_equals_replayed).
Reference: BatchNorm2d after Conv2d, src/shared/models_pytorch.py:133-150, 189-194."""
import pytest
import torch

from fedhip import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = 32


@pytest.fixture(autouse=True)
def _whole_chip():
    ops.set_fill_fraction(1.0)  # the unit tests' split plans assume the whole-chip planner
    yield


def _counts(nc, seed):
    g = torch.Generator().manual_seed(seed)
    c = [B] + [int(v) for v in torch.randint(1, B + 1, (nc - 1,), generator=g)]
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _both(fn):
    """fn(armed) for armed = True, False: (results_armed, results_plain); the armed run fused."""
    d0, t0 = ops.bn_defer_status()
    on = fn(True)
    torch.cuda.synchronize()
    d1, t1 = ops.bn_defer_status()
    off = fn(False)
    torch.cuda.synchronize()
    d2, t2 = ops.bn_defer_status()
    assert d1 > d0 and t1 - t0 == d1 - d0, (d0, t0, d1, t1)  # deferred and all taken
    assert (d2, t2) == (d1, t1)
    return on, off


def _eq(a, b, cnt=None):
    if cnt is None:
        assert torch.equal(a, b)
        return
    for z in range(a.shape[0]):
        k = int(cnt[z])
        assert torch.equal(a[z, :k], b[z, :k]), z


def _arm(armed):
    if armed:
        prev = ops.SPLIT_BN[0]
        ops.SPLIT_BN[0] = True  # off by default: measured no faster (ops.SPLIT_BN)
        try:
            ops.conv_bn_defer(8192)  # every shape here, whatever the default policy
        finally:
            ops.SPLIT_BN[0] = prev


@pytest.mark.parametrize("nc,ci,co,hw,pool,dm", [
    (1, 64, 64, 16, False, False), (1, 64, 64, 16, True, True), (1, 64, 128, 8, False, False),
    (1, 128, 128, 8, True, True), (2, 64, 128, 8, True, False), (3, 32, 64, 16, False, False)])
def test_fwd_reduction_in_finalize_bitwise(nc, ci, co, hw, pool, dm):
    torch.manual_seed(nc * 7 + ci + hw)
    cnt = _counts(nc, ci + hw)
    x = torch.randn(nc, B, ci, hw, hw, device=DEV)
    w = torch.randn(nc, co, ci, 3, 3, device=DEV) / (3.0 * ci ** 0.5)
    b = torch.randn(nc, co, device=DEV) * 0.1
    gamma = torch.rand(nc, co, device=DEV) + 0.5
    beta = torch.randn(nc, co, device=DEV) * 0.2
    in_sc = torch.rand(nc, ci, device=DEV) + 0.5
    in_sh = torch.randn(nc, ci, device=DEV) * 0.1

    def run(armed):
        y = torch.full((nc, B, co, hw, hw), 7.0, device=DEV)
        part = torch.zeros(nc, co, ops.bnstats_tiles(B, hw, hw), 2, dtype=torch.float64,
                           device=DEV)
        rm, rv = torch.zeros(nc, co, device=DEV) + 0.3, torch.ones(nc, co, device=DEV)
        sm, si, sc, sh = (torch.zeros(nc, co, device=DEV) for _ in range(4))
        _arm(armed)
        ops.conv2d_fwd(x, w, b, y, nc, B, ci, hw, hw, co, 3, 1, 1, counts=cnt,
                       in_affine=(in_sc, in_sh), bn_stats=part)
        out = [y, rm, rv, sm, si, sc, sh]
        if pool:
            h2 = hw // 2
            q = torch.zeros(nc, B, co, h2, h2, device=DEV)
            idx = torch.zeros(nc, B, co, h2, h2, dtype=torch.uint8, device=DEV)
            msk = torch.zeros_like(idx) if dm else None
            ops.maxpool2_fwd_bnfinalize(part, gamma, beta, rm, rv, sm, si, sc, sh, y, q, idx, nc,
                                        B, co, hw, hw, mask=msk, drop_mode=1 if dm else 0,
                                        p_drop=0.3, seed=17, counts=cnt)
            out += [q, idx] + ([msk] if dm else [])
        else:
            ops.bn_finalize_tiles(part, gamma, beta, rm, rv, sm, si, sc, sh, nc, B, co, hw * hw,
                                  counts=cnt)
        return out

    on, off = _both(run)
    _eq(on[0], off[0], cnt)
    for a, c in zip(on[1:7], off[1:7]):
        _eq(a, c)
    for a, c in zip(on[7:], off[7:]):
        _eq(a, c, cnt)


def test_unconsumed_reduction_materialises():
    """An armed split FWD whose output is read by something other than its BN call: the
    skipped epilogue runs first (the reader sees the reduced output)."""
    nc, ci, co, hw = 1, 64, 64, 16
    torch.manual_seed(3)
    x = torch.randn(nc, B, ci, hw, hw, device=DEV)
    w = torch.randn(nc, co, ci, 3, 3, device=DEV) / 24.0
    ys, parts = [], []
    for armed in (True, False):
        y = torch.zeros(nc, B, co, hw, hw, device=DEV)
        part = torch.zeros(nc, co, ops.bnstats_tiles(B, hw, hw), 2, dtype=torch.float64,
                           device=DEV)
        d0, _ = ops.bn_defer_status()
        _arm(armed)
        ops.conv2d_fwd(x, w, None, y, nc, B, ci, hw, hw, co, 3, 1, 1, bn_stats=part)
        d1, _ = ops.bn_defer_status()
        assert (d1 > d0) == armed
        y2 = torch.zeros_like(y)  # a conv reading y: the pending reduction launches first
        ops.conv2d_fwd(y, w, None, y2, nc, B, co, hw, hw, co, 3, 1, 1)
        torch.cuda.synchronize()
        ys.append((y, y2))
        parts.append(part)
    assert torch.equal(ys[0][0], ys[1][0]) and torch.equal(ys[0][1], ys[1][1])
    assert torch.equal(parts[0], parts[1])


def _rounds(model_name, sizes, split_bn, graphs, **kw):
    from fedhip.engine import PackedTrainer
    from src.shared import models_pytorch as hm
    prev, prev_max = ops.SPLIT_BN[0], ops.SPLIT_BN_MAX[0]
    ops.SPLIT_BN[0] = split_bn
    ops.SPLIT_BN_MAX[0] = 8192  # the 16x16 and 32x32 maps too
    try:
        torch.manual_seed(0)
        model = hm.ModelFactory.create_model(model_name, **kw).to(DEV)
        eng = PackedTrainer(model, capacity=len(sizes), batch=B, device=DEV)
        eng.use_graphs = graphs
        for k in range(len(sizes)):
            eng.load_module_state(k, model)
        g = torch.Generator().manual_seed(5)
        data = torch.randn(sum(sizes), 3, 32, 32, generator=g).to(DEV)
        labels = torch.randint(0, 10, (sum(sizes),), generator=g).to(DEV)
        offs = [sum(sizes[:k]) for k in range(len(sizes))]
        gen = torch.Generator().manual_seed(11)
        for r in range(2):
            plan = eng.make_plan(sizes, 1, generator=gen)
            eng.run_round(data, labels, offs, plan, "sgd", 1e-2, seed=r)
        torch.cuda.synchronize()
        return eng.params[:len(sizes)].clone(), eng.bufs[:len(sizes)].clone()
    finally:
        ops.SPLIT_BN[0], ops.SPLIT_BN_MAX[0] = prev, prev_max


@pytest.mark.parametrize("model_name,kw", [("cifar10_cnn", {"dropout_rate": 0.3})])
def test_rounds_bit_identical_with_split_bn(model_name, kw):
    """One-client and ragged steps (split plans): the trained rows and BN buffers with the
    fused launches equal the two-launch path's bit for bit, eager and replayed."""
    sizes = [100, 37, 9]
    d0, t0 = ops.bn_defer_status()
    p_on, b_on = _rounds(model_name, sizes, True, False, **kw)
    d1, t1 = ops.bn_defer_status()
    assert d1 > d0 and t1 - t0 == d1 - d0
    p_g, b_g = _rounds(model_name, sizes, True, True, **kw)
    p_off, b_off = _rounds(model_name, sizes, False, True, **kw)
    assert torch.equal(p_on, p_off) and torch.equal(b_on, b_off)
    assert torch.equal(p_g, p_off) and torch.equal(b_g, b_off)
