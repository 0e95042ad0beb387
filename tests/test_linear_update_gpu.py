"""The classifier layers' optimizer update applied by their weight-gradient launch
(fh_linear_bwd_fused_upd / _pool_upd, ops.LinearUpdate) against the unfused sequence on the
same inputs — fh_linear_bwd_fused followed by fh_sgd_step_slabs / fh_adam_step_slabs.  Nothing
is re-associated, so every comparison is torch.equal: parameters, optimizer state and dX."""
import pytest
import torch

from fedhip import ops
from fedhip.engine import PackedTrainer
from src.shared import models_pytorch as hm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B = 32
# csrc/conv.hip linear_bwd_fused_impl: two launches (the wide path) when in_f % 128 == 0 and
# (in_f / 128) * clients >= fill(256), fill(w) = max(1, int(w * fill fraction))
WIDE_WG = 256
FILL = 0.0625  # fill(256) = 16: the wide path starts at 16 (in_f 128) / 8 (in_f 256) clients
COUNTS = [31, 0, 1, 32]  # per client, cycled: all four in the wide launch

OPTS = {
    "sgd_plain": dict(opt="sgd", momentum=0.0, wd=0.0, first=False),
    "sgd_mom_wd_first": dict(opt="sgd", momentum=0.9, wd=1e-3, first=True),
    "sgd_mom_wd_later": dict(opt="sgd", momentum=0.9, wd=1e-3, first=False),
    "adam": dict(opt="adam", momentum=0.0, wd=0.0, first=False),
    "adamw": dict(opt="adamw", momentum=0.0, wd=0.01, first=False),
}


def _wide_threshold(in_f):
    fill = max(1, int(WIDE_WG * FILL))
    return -(-fill // (in_f // 128))


@pytest.fixture
def fill_fraction():
    ops.set_fill_fraction(FILL)
    yield
    ops.set_fill_fraction(1.0)


def _rows(n, n_w, n_b, gen):
    """Packed rows [w | b | a plain tail] padded to 64 floats, random everywhere."""
    L = (n_w + n_b + 64 + 63) // 64 * 64
    r = lambda: torch.randn(n, L, generator=gen).to(DEV)
    return dict(P=r(), G=r(), S1=r(), S2=r().abs())


def _optimizer(o, t, n, ranges, scal):
    if o["opt"] == "sgd":
        ops.sgd_step_slabs(t["P"], t["G"], t["S1"], 0.05, o["momentum"], n, ranges,
                           weight_decay=o["wd"], first_step=o["first"])
    else:
        ops.adam_step_slabs(t["P"], t["G"], t["S1"], t["S2"], 3, 0.05, n, ranges,
                            weight_decay=o["wd"], decoupled=o["opt"] == "adamw", scal_dev=scal)


def _update(o, t, scal, mode):
    return ops.LinearUpdate(t["P"], t["S1"], t["S2"], o["opt"], 0.05, step=3,
                            first_step=o["first"], momentum=o["momentum"],
                            weight_decay=o["wd"], scal_dev=scal, mode=mode)


def _case(o, n, in_f, out_f, bias, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    n_w = in_f * out_f
    base = _rows(n, n_w, out_f, gen)
    x = torch.randn(n, B, in_f, generator=gen).to(DEV)
    dy = torch.randn(n, B, out_f, generator=gen).to(DEV)
    mask = (torch.rand(n, B, in_f, generator=gen) > 0.3).to(torch.uint8).to(DEV)
    counts = torch.tensor([COUNTS[k % 4] for k in range(n)], dtype=torch.int32, device=DEV)
    scal = None
    if o["opt"] != "sgd":  # the per-step scalars from device memory, as a step program reads them
        step_size, bc2 = ops.adam_bias_corrections(3, 0.05)
        scal = torch.tensor([bc2, -step_size], dtype=torch.float32, device=DEV)
    out = []
    for fused in (False, True):
        t = {k: v.clone() for k, v in base.items()}
        w, dw = t["P"][:, :n_w], t["G"][:, :n_w]
        db = t["G"][:, n_w:n_w + out_f] if bias else None
        dx = torch.zeros(n, B, in_f, device=DEV)
        kw = dict(mask=mask, p_drop=0.3, relu_ref=x, counts=counts)
        if fused:
            slabs = ops.GradSlabs(DEV)
            before = ops.LINEAR_UPDATES[0]
            with slabs.collect(t["G"]) as d:
                assert ops.linear_bwd_fused(x, dy, w, dw, db, dx, n, B, in_f, out_f,
                                            update=_update(o, t, scal, mode), **kw)
            ranges = d.ranges
            applied = ops.LINEAR_UPDATES[0] - before
            assert len(ranges) == applied * (2 if bias else 1)
        else:
            assert ops.linear_bwd_fused(x, dy, w, dw, db, dx, n, B, in_f, out_f, **kw)
            ranges, applied = [], 0
        _optimizer(o, t, n, ranges, scal)
        out.append((t, dx, applied))
    torch.cuda.synchronize()
    (ref, dx_ref, _), (got, dx_got, applied) = out
    tag = (o, n, in_f, out_f, bias, mode)
    assert torch.equal(dx_got, dx_ref), tag
    for k in ("P", "S1", "S2"):
        assert torch.equal(got[k], ref[k]), (k,) + tag
    return applied


@pytest.mark.parametrize("oname", list(OPTS))
@pytest.mark.parametrize("in_f,out_f", [(128, 32), (128, 96), (256, 32), (256, 96)])
def test_fused_update_matches_unfused_sequence(fill_fraction, oname, in_f, out_f):
    o = OPTS[oname]
    thr = _wide_threshold(in_f)
    assert 2 <= thr < 40
    seed = 0
    for n in (1, 3, thr + 1):
        for bias in (True, False):
            for mode in (1, 2):
                seed += 1
                applied = _case(o, n, in_f, out_f, bias, mode, seed)
                # mode 1 fuses on the wide path only, mode 2 at every width
                assert applied == int(mode == 2 or n >= thr), (n, mode, applied)


def test_fused_update_pool_entry_point():
    """The _pool entry point at SimpleCNN's fc1 shape (64 x 7 x 7 -> 128, 16 x 16 planes), two
    clients: in_f % 128 != 0, so only mode 2 fuses."""
    n, C, OH, out_f = 2, 64, 7, 128
    in_f, n_w = C * OH * OH, C * OH * OH * out_f
    o = OPTS["sgd_mom_wd_later"]
    gen = torch.Generator().manual_seed(3)
    base = _rows(n, n_w, out_f, gen)
    x = torch.randn(n, B, C, OH, OH, generator=gen).to(DEV)
    dy = torch.randn(n, B, out_f, generator=gen).to(DEV)
    pidx = torch.randint(0, 4, (n, B, C, OH, OH), generator=gen).to(torch.uint8).to(DEV)
    counts = torch.tensor([32, 9], dtype=torch.int32, device=DEV)
    out = []
    for fused in (False, True):
        t = {k: v.clone() for k, v in base.items()}
        w, dw, db = t["P"][:, :n_w], t["G"][:, :n_w], t["G"][:, n_w:n_w + out_f]
        dx = torch.zeros(n, B, C, 16, 16, device=DEV)
        ranges = []
        if fused:
            with ops.GradSlabs(DEV).collect(t["G"]) as d:
                assert ops.linear_bwd_fused_pool(x, dy, w, dw, db, dx, pidx, n, B, C, OH, OH,
                                                 out_f, counts=counts,
                                                 update=_update(o, t, None, 2))
            ranges = d.ranges
            assert len(ranges) == 2
        else:
            assert ops.linear_bwd_fused_pool(x, dy, w, dw, db, dx, pidx, n, B, C, OH, OH, out_f,
                                             counts=counts)
        _optimizer(o, t, n, ranges, None)
        out.append((t, dx))
    torch.cuda.synchronize()
    (ref, dx_ref), (got, dx_got) = out
    assert torch.equal(dx_got, dx_ref)
    for k in ("P", "S1", "S2"):
        assert torch.equal(got[k], ref[k]), k


# ---- whole steps: two local epochs of three ragged clients ---------------------------------
SIZES = [100, 70, 37]
_ROUNDS = {}


def _round(name, opt, launch, mode, fill):
    """Trained rows after a two-epoch round; computed once per configuration and shared."""
    key = (name, opt, launch, mode, fill)
    if key in _ROUNDS:
        return _ROUNDS[key]
    prev = ops.FUSE_LINEAR_UPDATE[0]
    ops.FUSE_LINEAR_UPDATE[0] = mode
    ops.set_fill_fraction(fill)
    try:
        torch.manual_seed(0)
        kw = {"dropout_rate": 0.3} if name == "cifar10_cnn" else {}
        model = hm.ModelFactory.create_model(name, **kw).to(DEV)
        eng = PackedTrainer(model, capacity=len(SIZES), batch=32, device=DEV)
        if launch == "eager":
            eng.use_graphs = False
        else:
            eng.launch_mode = "program"
        for k in range(len(SIZES)):
            eng.load_module_state(k, model)
        g = torch.Generator().manual_seed(5)
        shape = (1, 28, 28) if name == "simple_cnn" else (3, 32, 32)
        data = torch.randn(sum(SIZES), *shape, generator=g).to(DEV)
        labels = torch.randint(0, 10, (sum(SIZES),), generator=g).to(DEV)
        offs = [sum(SIZES[:k]) for k in range(len(SIZES))]
        plan = eng.make_plan(SIZES, 2, generator=torch.Generator().manual_seed(11))
        before = ops.LINEAR_UPDATES[0]
        eng.run_round(data, labels, offs, plan, opt, 1e-2, seed=1)
        torch.cuda.synchronize()
        res = (eng.params.clone(), eng.bufs.clone(), ops.LINEAR_UPDATES[0] - before)
        eng.release_graphs()
    finally:
        ops.FUSE_LINEAR_UPDATE[0] = prev
        ops.set_fill_fraction(1.0)
    _ROUNDS[key] = res
    return res


# (mode, fill fraction): every width at fill 1; the wide path only, at a fill fraction that
# makes three clients wide for CIFAR10CNN's fc1 (16 k-blocks * 2 clients >= fill(256) = 32)
@pytest.mark.parametrize("mode,fill", [(2, 1.0), (1, 0.125)])
@pytest.mark.parametrize("name", ["cifar10_cnn", "simple_cnn"])
def test_rounds_bit_identical_fused_and_unfused(name, mode, fill):
    p_off, b_off, n_off = _round(name, "sgd", "program", 0, fill)
    p_on, b_on, n_on = _round(name, "sgd", "program", mode, fill)
    p_eager, b_eager, n_eager = _round(name, "sgd", "eager", mode, fill)
    assert n_off == 0
    if mode == 2 or name == "cifar10_cnn":
        assert n_on > 0 and n_eager > 0  # the fused launches really ran
    assert torch.equal(p_on, p_off) and torch.equal(b_on, b_off)
    assert torch.equal(p_eager, p_off) and torch.equal(b_eager, b_off)


def test_adam_round_bit_identical_fused_and_unfused():
    """Adam through step programs: the fused launches read the relocated per-step scalars."""
    p_off, b_off, _ = _round("cifar10_cnn", "adam", "program", 0, 1.0)
    p_on, b_on, n_on = _round("cifar10_cnn", "adam", "program", 2, 1.0)
    assert n_on > 0
    assert torch.equal(p_on, p_off) and torch.equal(b_on, b_off)
