"""The server-optimizer kernel (csrc/fedopt.hip) and what is built on it, on the GPU, against
the numpy reference of tests/fedopt_ref.py (pinned by test_fedopt_ref_cpu.py).

fh_server_opt_step is held to the reference bit for bit (uint32 views of g', m' and v'), for
the four rules, client counts around the 4-rows-in-flight unroll, sizes below / across the
4-column vector width, the 256-thread block and one pass of the capped grid, normal,
state-like and special-value data, through the vector path and every way onto the scalar path
(odd stride, rows + 4 B, each of global / m / v + 4 B).  Outputs live inside sentinel-filled
buffers and the gaps between rows hold NaN.
"""
import os
from datetime import datetime

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fedopt_ref as fr
import robust_ref as rr
from fedhip import ops
from fedhip._lib import FedHipError
from src.aggregation import fedopt, robust
from src.aggregation.fedavg import FedAvgError
from src.shared.models import GlobalModel, ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5
F = np.float32

CS = [1, 2, 3, 4, 5, 9, 33]
PS = [1, 3, 13, 1001, 4099]
RULES = [fr.MOMENTUM, fr.ADAGRAD, fr.ADAM, fr.YOGI]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000,
                     0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA5A5A5, 0x7FFFFFFF],
                    dtype=np.uint32).view(np.float32)
SCALARS = dict(server_lr=0.1, beta1=0.9, beta2=0.99, tau=1e-3)
GRID_PASS = 8192 * 256 * 4  # coordinates one pass of the vector kernel's capped grid covers


def _weights(C):
    n = [10 + k for k in range(C)]
    return np.array([x / sum(n) for x in n], dtype=F)  # n_k / sum(n) in double, then fp32


def _data(kind, C, P, seed):
    """(rows [C, P], g, m, v, scalars)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P).astype(F)
    rows = (g + 0.1 * rng.standard_normal((C, P))).astype(F)
    m = (0.05 * rng.standard_normal(P)).astype(F)
    v = (1e-6 + 0.01 * rng.random(P)).astype(F)
    sc = dict(SCALARS)
    if kind == "state":  # v over sixteen decades, m of both signs and sizes
        v = (10.0 ** rng.uniform(-12, 4, P)).astype(F)
        m = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 1, P)).astype(F)
    elif kind == "special":
        sc["tau"] = 0.0  # v' = 0 divides by zero
        for j in range(P):
            s = SPECIALS[(j // 8) % len(SPECIALS)]
            k = j % 8
            if k == 0:
                rows[rng.integers(C), j] = s
            elif k == 1:
                g[j] = s
            elif k == 2:
                m[j] = s
            elif k == 3:
                v[j] = s
            elif k == 4:   # denormal v
                v[j] = F(1e-40) * F(1 + j % 3)
            elif k == 5:   # d*d underflows to zero, or to a denormal
                g[j] = F(0.0) if j % 16 < 8 else F(-0.0)
                rows[:, j] = F(1e-25) if j % 32 < 16 else F(-3e-20)
            elif k == 6:   # v = 0: 0/0 when d = 0, x/0 otherwise
                v[j] = 0.0
                if j % 16 < 8:
                    rows[:, j] = g[j]
                    m[j] = 0.0
            else:          # signed zeros everywhere
                rows[:, j] = F(-0.0)
                g[j] = F(-0.0) if j % 16 < 8 else F(0.0)
                m[j] = F(-0.0)
    return rows, g, m, v, sc


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show)."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


def _window(x, offset):
    """x [P] inside a sentinel-filled buffer, `offset` floats from its 16-B aligned base."""
    P = x.shape[0]
    buf = torch.full((P + 16,), SENTINEL, device=DEV)
    buf[offset:offset + P].copy_(torch.from_numpy(x))
    return buf, buf[offset:offset + P], offset


def _sentinels_intact(win, P):
    buf, _, offset = win
    b = buf.cpu().numpy()
    return (b[:offset] == SENTINEL).all() and (b[offset + P:] == SENTINEL).all()


def _run(rule, view, weights, g, m, v, sc, offs=(4, 4, 4), row_index=None, v_none=False):
    """One launch on copies of g, m, v placed at `offs` floats; returns (g', m', v') numpy."""
    P = g.shape[0]
    wg, wm, wv = _window(g, offs[0]), _window(m, offs[1]), _window(v, offs[2])
    w32 = None if weights is None else torch.from_numpy(np.asarray(weights, dtype=F)).to(DEV)
    out = ops.server_opt_step(view, wg[1], wm[1], None if v_none else wv[1], rule,
                              weights_f32=w32, row_index=row_index, P=P, **sc)
    torch.cuda.synchronize()
    assert out is wg[1]
    assert all(_sentinels_intact(w, P) for w in (wg, wm, wv))
    return wg[1].cpu().numpy(), wm[1].cpu().numpy(), wv[1].cpu().numpy()


def _same(got, want, rule, v_before):
    """g', m', v' bit for bit; FedAvgM leaves v as it was."""
    if rule == fr.MOMENTUM:
        return rr.same_bits(got[0], want[0]) and rr.same_bits(got[1], want[1]) \
            and rr.same_bits(got[2], v_before)
    return all(rr.same_bits(a, b) for a, b in zip(got, want))


def _layouts(P):
    vec, odd = (P + 3) // 4 * 4 + 4, P | 1
    return [("vector", vec, 0, (4, 4, 4)), ("odd stride", odd, 0, (4, 4, 4)),
            ("rows + 4 B", vec, 1, (4, 4, 4)), ("global + 4 B", vec, 0, (1, 4, 4)),
            ("m + 4 B", vec, 0, (4, 1, 4)), ("v + 4 B", vec, 0, (4, 4, 1))]


@pytest.mark.parametrize("rule", RULES)
def test_server_opt_bits(rule):
    for C in CS:
        w = _weights(C)
        for ki, kind in enumerate(("normal", "state", "special")):
            for P in PS:
                rows, g, m, v, sc = _data(kind, C, P, 1000 * C + 10 * ki + P)
                want = fr.server_opt_step(rule, rows, w, g, m, v, **sc)
                views = {}
                for name, stride, roff, offs in _layouts(P):
                    if (stride, roff) not in views:
                        views[stride, roff] = _place(rows, stride, roff)
                    got = _run(rule, views[stride, roff], w, g, m, v, sc, offs)
                    assert _same(got, want, rule, v), (kind, C, P, name)


@pytest.mark.parametrize("rule", RULES)
def test_single_row_mode(rule):
    """weights=None: the one row is the aggregate.  On data without -0.0 or NaN payloads in
    the row (0 + 1.0*x is x there), rows mode with C = 1, w = [1.0] gives the same bits."""
    one = np.ones(1, dtype=F)
    for ki, kind in enumerate(("normal", "state", "special")):
        for P in PS:
            rows, g, m, v, sc = _data(kind, 1, P, 50 + 10 * ki + P)
            want = fr.server_opt_step(rule, rows, None, g, m, v, **sc)
            for name, stride, roff, offs in _layouts(P)[:3]:
                view = _place(rows, stride, roff)
                got = _run(rule, view, None, g, m, v, sc, offs)
                assert _same(got, want, rule, v), (kind, P, name)
                if kind != "special":
                    assert _same(_run(rule, view, one, g, m, v, sc, offs), want, rule, v)


@pytest.mark.parametrize("rule", RULES)
def test_row_index_picks_rows_in_its_order(rule):
    """A permuted subset of a taller matrix: the reference over the picked rows in THAT
    order (the weighted sum is sequential; another order may round differently)."""
    C, tall, P = 5, 11, 1001
    rng = np.random.default_rng(rule)
    rows, g, m, v, sc = _data("special", tall, P, 300 + rule)
    pick = rng.permutation(tall)[:C]
    w = _weights(C)
    want = fr.server_opt_step(rule, rows[pick], w, g, m, v, **sc)
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    for stride, roff in ((1008, 0), (1003, 0), (1008, 1)):
        got = _run(rule, _place(rows, stride, roff), w, g, m, v, sc, row_index=idx)
        assert _same(got, want, rule, v), (stride, roff)
    # single-row mode through an index: that row is the aggregate
    want1 = fr.server_opt_step(rule, rows[pick[:1]], None, g, m, v, **sc)
    got1 = _run(rule, _place(rows, 1008, 0), None, g, m, v, sc, row_index=idx[:1])
    assert _same(got1, want1, rule, v)


@pytest.mark.parametrize("rule", RULES)
def test_three_consecutive_steps_carry_the_state(rule):
    C, P = 4, 1001
    w = _weights(C)
    rng = np.random.default_rng(7 + rule)
    tau32 = F(SCALARS["tau"])
    g = rng.standard_normal(P).astype(F)
    m, v = np.zeros(P, dtype=F), np.full(P, tau32 * tau32, dtype=F)
    gd, md, vd = (torch.from_numpy(x.copy()).to(DEV) for x in (g, m, v))
    w32 = torch.from_numpy(w).to(DEV)
    for step in range(3):
        rows = (g + 0.05 * rng.standard_normal((C, P))).astype(F)
        g, m, vn = fr.server_opt_step(rule, rows, w, g, m, v, **SCALARS)
        v = v if vn is None else vn
        ops.server_opt_step(_place(rows, 1004, 0), gd, md, vd, rule, weights_f32=w32, **SCALARS)
        for got, want in ((gd, g), (md, m), (vd, v)):
            assert rr.same_bits(got.cpu().numpy(), want), step
    assert not rr.same_bits(m, np.zeros(P, dtype=F))


def test_grid_stride_past_one_pass():
    """P = one pass of the capped vector grid + 5: the last float4 is a second trip of the
    grid-stride loop, the last coordinate the scalar tail."""
    C, P = 2, GRID_PASS + 5
    rng = np.random.default_rng(11)
    g = rng.standard_normal(P, dtype=F)
    rows = np.stack([g + F(0.1) * rng.standard_normal(P, dtype=F) for _ in range(C)])
    m = F(0.05) * rng.standard_normal(P, dtype=F)
    v = F(1e-6) + F(0.01) * rng.random(P, dtype=F)
    w = _weights(C)
    want = fr.server_opt_step(fr.YOGI, rows, w, g, m, v, **SCALARS)
    got = _run(fr.YOGI, _place(rows, P + 3, 0), w, g, m, v, SCALARS)
    assert _same(got, want, fr.YOGI, v)


def test_momentum_needs_no_second_moment():
    C, P = 3, 1001
    rows, g, m, v, sc = _data("normal", C, P, 5)
    w = _weights(C)
    want = fr.server_opt_step(fr.MOMENTUM, rows, w, g, m, None, **sc)
    view = _place(rows, 1004, 0)
    poison = np.full(P, np.nan, dtype=F)
    for v_none in (True, False):
        got = _run(fr.MOMENTUM, view, w, g, m, poison, sc, v_none=v_none)
        assert rr.same_bits(got[0], want[0]) and rr.same_bits(got[1], want[1])
        assert rr.same_bits(got[2], poison)


def test_server_opt_argument_errors():
    rows = torch.zeros(3, 8, device=DEV)
    w3 = torch.full((3,), 1 / 3, device=DEV)
    g = torch.full((8,), SENTINEL, device=DEV)
    m, v = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)

    def step(rows=rows, g=g, m=m, v=v, rule=2, w=w3, **kw):
        sc = dict(SCALARS)
        sc.update(kw)
        P = sc.pop("P", None)
        ops.server_opt_step(rows, g, m, v, rule, weights_f32=w, P=P, **sc)
    for kw, msg in (({"rule": 4}, "outside"), ({"rule": -1}, "outside"),
                    ({"w": None}, "no weights"), ({"rows": rows[:0], "w": w3[:0]}, "num_clients"),
                    ({"tau": -1.0}, "negative"), ({"server_lr": float("inf")}, "non-finite"),
                    ({"beta1": float("nan")}, "non-finite"), ({"beta2": 1e39}, "non-finite"),
                    ({"v": None}, "null pointer"), ({"v": None, "rule": 3}, "null pointer"),
                    ({"rows": torch.zeros(3, 8)}, "HIP device"),
                    ({"g": torch.zeros(8)}, "HIP device"),
                    ({"m": m[:7]}, "at least P=8"), ({"P": 9}, "at least P=9"),
                    ({"rows": rows.double()}, "float32"), ({"v": v.double()}, "float32"),
                    ({"g": torch.zeros(8, 2, device=DEV)[:, 0]}, "contiguous")):
        with pytest.raises(FedHipError, match=msg):
            step(**kw)
    step(P=0)
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == SENTINEL).all()  # nothing was launched
    assert not m.any() and (v == 1).all()


# ------------------------------------------------------------------ ServerOptimizer
SHAPES = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}


def _np(t):
    return t.detach().cpu().numpy()


def _scalars(so):
    return dict(server_lr=so.server_lr, beta1=so.beta1, beta2=so.beta2, tau=so.tau)


def _init_state(so, P):
    tau32 = F(so.tau)
    return np.zeros(P, dtype=F), np.full(P, tau32 * tau32, dtype=F)


def test_step_packed_against_the_reference_and_state_round_trip():
    tall, P, stride = 7, 1001, 1008
    pick, n = [5, 0, 3, 6], [30, 10, 25, 40]
    rng = np.random.default_rng(21)
    w = np.array([x / sum(n) for x in n], dtype=F)
    for kind in ("fedavgm", "fedadagrad", "fedadam", "fedyogi"):
        so = fedopt.create_server_optimizer(kind, server_lr=0.05, tau=0.01, device=DEV)
        g = rng.standard_normal(P).astype(F)
        m, v = _init_state(so, P)
        gd = torch.from_numpy(g.copy()).to(DEV)
        clone = None
        for step in range(3):
            rows = (g + 0.05 * rng.standard_normal((tall, P))).astype(F)
            g, m, vn = fr.server_opt_step(so.rule, rows[pick], w, g, m, v, **_scalars(so))
            v = v if vn is None else vn
            packed = _place(rows, stride, 0)
            opt = so if step < 2 else clone  # the third step runs on the restored copy
            assert opt.step_packed(packed, n, gd, row_index=pick) is gd
            assert rr.same_bits(_np(gd), g) and rr.same_bits(_np(opt.m), m), (kind, step)
            if so.rule != fr.MOMENTUM:
                assert rr.same_bits(_np(opt.v), v), (kind, step)
            else:
                assert opt.v is None
            if step == 1:  # state_dict -> a new object (made for another rule) -> same step
                clone = fedopt.FedAvgM(1.0, device=DEV)
                clone.load_state_dict(so.state_dict())
                assert clone.rule == so.rule and clone.m is not so.m
        with pytest.raises(FedAvgError, match="parameters"):
            so.step_packed(packed[:, :P - 1], n, gd[:P - 1], row_index=pick)
    # rows without an index: every row, in order
    so = fedopt.FedAdam(0.05, device=DEV)
    rows = rng.standard_normal((4, P)).astype(F)
    g = rng.standard_normal(P).astype(F)
    gd = torch.from_numpy(g.copy()).to(DEV)
    so.step_packed(_place(rows, stride, 0), n, gd)
    want = fr.server_opt_step(fr.ADAM, rows, w, g, *_init_state(so, P), **_scalars(so))
    assert rr.same_bits(_np(gd), want[0])


def test_step_packed_with_a_median_base_and_step_vector():
    C, P = 5, 1001
    rng = np.random.default_rng(22)
    g = rng.standard_normal(P).astype(F)
    rows = (g + 0.05 * rng.standard_normal((C, P))).astype(F)
    so = fedopt.FedYogi(0.05, base=robust.MedianAggregator(), device=DEV)
    assert not so.plain_base
    gd = torch.from_numpy(g.copy()).to(DEV)
    so.step_packed(_place(rows, 1008, 0), [10] * C, gd)
    med = rr.median(rows)
    want = fr.server_opt_step(fr.YOGI, med[None], None, g, *_init_state(so, P), **_scalars(so))
    assert rr.same_bits(_np(gd), want[0]) and rr.same_bits(_np(so.m), want[1])
    assert rr.same_bits(_np(so.v), want[2])
    # step_vector on an aggregate that already exists: the same single-row step
    sv = fedopt.FedYogi(0.05, device=DEV)
    gd2 = torch.from_numpy(g.copy()).to(DEV)
    assert sv.step_vector(torch.from_numpy(med).to(DEV), gd2) is gd2
    assert rr.same_bits(_np(gd2), want[0]) and rr.same_bits(_np(sv.v), want[2])


def _flat(weights):
    return np.concatenate([_np(weights[n]).reshape(-1) for n in SHAPES])


def test_aggregate_updates_round_trip():
    gen = torch.Generator().manual_seed(4)
    prev_w = {name: 0.3 * torch.randn(*shape, generator=gen) for name, shape in SHAPES.items()}
    prev = GlobalModel(round_number=3, model_weights=prev_w, accuracy_metrics={},
                       participating_clients=[], convergence_score=0.0)
    ups = []
    for k in range(3):
        wts = {name: t + 0.05 * torch.randn(*t.shape, generator=gen)
               for name, t in prev_w.items()}
        ups.append(ModelUpdate(client_id=f"c{k}", round_number=4, model_weights=wts,
                               num_samples=10 + k, training_loss=0.5, privacy_budget_used=0.5,
                               compression_ratio=0.8, timestamp=datetime.now()))
    so = fedopt.FedAdam(0.05, device=DEV)
    gm = so.aggregate_updates(ups, 4, prev)
    assert gm.round_number == 4 and gm.participating_clients == ["c0", "c1", "c2"]
    assert [gm.model_weights[n].shape for n in SHAPES] == [torch.Size(s) for s in SHAPES.values()]
    rows = np.stack([_flat(u.model_weights) for u in ups])
    g0 = _flat(prev_w)
    want = fr.server_opt_step(fr.ADAM, rows, _weights(3), g0, *_init_state(so, g0.size),
                              **_scalars(so))
    assert rr.same_bits(_flat(gm.model_weights), want[0])
    assert rr.same_bits(_flat(prev_w), g0)  # the previous model is not stepped in place
    assert so.base.aggregation_history[-1]["client_samples"]["c2"] == 12
    with pytest.raises(FedAvgError):
        so.aggregate_updates([], 5, prev)
    bad_prev = GlobalModel(5, {"fc.bias": prev_w["fc.bias"]}, {}, [], 0.0)
    with pytest.raises(FedAvgError, match="previous model"):
        so.aggregate_updates(ups, 5, bad_prev)


# ------------------------------------------------------------------ RankRound
SIZES = [70, 55, 48, 40]


def _client_data(k, n):
    g = torch.Generator().manual_seed(200 + k)
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _rounds(mine, nrounds=1, server_opt="omit"):
    """`nrounds` rounds of SimpleCNN over SIZES' clients `mine` on one RankRound.  Returns the
    RankRound, the global vector before round one, and per round (the trained rows by client,
    copied by the on_trained hook; the global vector; global_bufs; partial)."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    kw = {} if isinstance(server_opt, str) else {"server_opt": server_opt}
    r = RankRound(model, SIZES, mine, epochs=1, device=DEV, lanes=1, shuffle_seed=77, **kw)
    xs, ys = zip(*[_client_data(k, SIZES[k]) for k in r.slots])
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    start = _np(r.global_flat).copy()
    out = []
    for i in range(nrounds):
        r.run(data, labels, offs, "sgd", 0.01, seed=3 + i)
        torch.cuda.synchronize()
        out.append((dict(seen), _np(r.global_flat).copy(), _np(r.global_bufs).copy(),
                    _np(r.partial).copy()))
    return r, start, out


def test_rankround_one_rank_fedadam_two_rounds():
    all4 = list(range(4))
    so = fedopt.FedAdam(0.01, device=DEV)
    r, g, rounds = _rounds(all4, 2, so)
    w = _np(r.w32)
    assert r.clients == all4 and w.dtype == F
    m, v = _init_state(so, r.P)
    for i, (rows, glob, _, _) in enumerate(rounds):
        stack = np.stack([rows[k] for k in r.clients])
        g, m, v = fr.server_opt_step(fr.ADAM, stack, w, g, m, v, **_scalars(so))
        assert rr.same_bits(glob, g), f"round {i + 1}"
    assert rr.same_bits(_np(so.m), m) and rr.same_bits(_np(so.v), v)
    # server_opt=None is today's path: same seeds, same bits as without the argument; and
    # the BN running statistics do not see the server optimizer
    _, _, plain = _rounds(all4)
    _, _, none = _rounds(all4, server_opt=None)
    assert rr.same_bits(plain[0][1], none[0][1]) and not rr.same_bits(plain[0][1], rounds[0][1])
    assert rr.same_bits(plain[0][2], rounds[0][2]) and rr.same_bits(plain[0][2], none[0][2])
    # the plain round assigns the aggregate the server optimizer stepped toward
    stack = np.stack([rounds[0][0][k] for k in all4])
    assert rr.same_bits(plain[0][1], fr.weighted_sum(stack, w))


def _rank_main(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        so = fedopt.FedYogi(0.01, device=DEV)
        r, start, rounds = _rounds(mine, 1, so)
        q.put((rank, (start, rounds[0], _np(so.m), _np(so.v), _np(r.w32), list(r.clients))))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def test_rankround_fedyogi_two_ranks_all_reduce():
    """Two gloo ranks on cuda:0 in all-reduce mode: both ranks end with bit-identical global
    vectors and moments, equal to the reference single-row step from the all-reduced partial
    sum, which is the weighted sum of every client's trained row up to the association of
    the all-reduce (a few ulp of its terms)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29760 + os.getpid() % 200
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for r in range(world):
        assert not isinstance(res[r], str), f"rank {r} failed: {res[r]}"
    assert all(p.exitcode == 0 for p in procs)
    (s0, (rows0, g0, _, part0), m0, v0, w0, c0), (s1, (rows1, g1, _, part1), m1, v1, w1, c1) = \
        res[0], res[1]
    assert sorted(c0 + c1) == list(range(len(SIZES)))
    assert rr.same_bits(s0, s1) and rr.same_bits(part0, part1)
    assert rr.same_bits(g0, g1), "ranks disagree on the global model"
    assert rr.same_bits(m0, m1) and rr.same_bits(v0, v1), "ranks disagree on the state"
    so = fedopt.FedYogi(0.01, device=DEV)
    want = fr.server_opt_step(fr.YOGI, part0[None], None, s0, *_init_state(so, s0.size),
                              **_scalars(so))
    assert rr.same_bits(g0, want[0]) and rr.same_bits(m0, want[1]) and rr.same_bits(v0, want[2])
    assert not rr.same_bits(g0, part0)
    # the partial sums: each rank's is sequential over its clients, the all-reduce adds the two
    sums = [fr.weighted_sum(np.stack([rows[k] for k in c]), w)
            for rows, w, c in ((rows0, w0, c0), (rows1, w1, c1))]
    assert rr.same_bits(part0, sums[0] + sums[1])
