"""The robust aggregation kernels (csrc/robust.hip) and the rules built on them, on the GPU,
against the numpy references of tests/robust_ref.py (pinned by test_robust_ref_cpu.py).

fh_trimmed_mean_rows is held to the reference bit for bit (uint32 views), over every padded
network size and its neighbours, every legal kind of trim, sizes below / across the 4-column
vector width and the 256-thread block, normal, heavily tied and special-value data, through
both the vector path and the scalar path (odd stride, misaligned rows, misaligned out).
fh_pairwise_sqdist must be exact on small-integer rows whatever the chunking, and within the
fp64 summation-order bound  P * 2^-53 * sum  on normal data.
"""
import os
from datetime import datetime

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import robust_ref as rr
from fedhip import ops
from fedhip._lib import FedHipError
from src.aggregation import robust
from src.aggregation.fedavg import FedAvgAggregator
from src.shared.models import ModelUpdate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -12345.5

CS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
PS = [1, 3, 13, 1001, 4099]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000,
                     0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA5A5A5, 0x7FFFFFFF],
                    dtype=np.uint32).view(np.float32)


def _trims(C):
    return sorted({t for t in (0, 1, (C - 1) // 2) if 2 * t < C})  # (C-1)//2: median = largest


def _data(kind, C, P, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((C, P)).astype(np.float32)
    if kind == "tied":
        return rng.integers(-3, 4, size=(C, P)).astype(np.float32)
    # special: coordinate j holds j % (C + 1) special values (0 .. C of them, so some
    # coordinates stay within every trim and some exceed it), in random rows
    rows = rng.standard_normal((C, P)).astype(np.float32)
    for j in range(P):
        n = j % (C + 1)
        rows[rng.permutation(C)[:n], j] = SPECIALS[(j + np.arange(n)) % len(SPECIALS)]
    return rows


def _window(P, offset):
    """out: P floats inside a sentinel-filled buffer, `offset` floats from its 16-B base."""
    buf = torch.full((P + 16,), SENTINEL, device=DEV)
    return buf, buf[offset:offset + P]


def _sentinels_intact(buf, offset, P):
    b = buf.cpu().numpy()
    return (b[:offset] == SENTINEL).all() and (b[offset + P:] == SENTINEL).all()


def _place(rows, stride, base_offset):
    """rows [C, P] as a device view with the given row stride, `base_offset` floats from a
    16-B aligned base; the gaps hold NaN (a read past a row would show)."""
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), float("nan"), device=DEV)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


def _tm(view, trim, out_offset=4, row_index=None):
    P = view.shape[1]
    buf, out = _window(P, out_offset)
    ops.trimmed_mean_rows(view, out, trim, row_index=row_index)
    torch.cuda.synchronize()
    assert _sentinels_intact(buf, out_offset, P)
    return out.cpu().numpy()


@pytest.mark.parametrize("C", CS)
def test_trimmed_mean_bits(C):
    for ki, kind in enumerate(("normal", "tied", "special")):
        for P in PS:
            rows = _data(kind, C, P, 1000 * C + 10 * ki + P)
            vec = _place(rows, (P + 3) // 4 * 4 + 4, 0)   # 16-B columns + scalar tail
            sca = _place(rows, P | 1, 0)                  # odd stride: scalar path
            for trim in _trims(C):
                want = rr.trimmed_mean(rows, trim)
                for view in (vec, sca):
                    got = _tm(view, trim)
                    assert rr.same_bits(got, want), (kind, P, trim, view.stride(0))


@pytest.mark.parametrize("C", [3, 8, 17, 33, 64])
def test_trimmed_mean_row_index_misalignment_and_permutation(C):
    P, tall = 1001, C + 5
    rng = np.random.default_rng(C)
    rows = _data("special", tall, P, 77 + C)
    pick = rng.permutation(tall)[:C]           # a subset of a taller matrix, permuted
    pick2 = pick[rng.permutation(C)]           # the same rows in another order
    trim = max(1, C // 4) if C > 2 else 0
    want = rr.trimmed_mean(rows[pick], trim)
    idx, idx2 = (torch.tensor(p, dtype=torch.int32, device=DEV) for p in (pick, pick2))
    aligned = _place(rows, 1008, 0)
    a = _tm(aligned, trim, row_index=idx)
    assert rr.same_bits(a, want)
    assert rr.same_bits(_tm(aligned, trim, row_index=idx2), a)          # order-independent
    assert rr.same_bits(_tm(_place(rows, 1008, 1), trim, row_index=idx), want)   # rows + 4 B
    assert rr.same_bits(_tm(aligned, trim, out_offset=1, row_index=idx), want)   # out + 4 B
    assert rr.same_bits(_tm(_place(rows, 1003, 0), trim, row_index=idx2), want)  # odd stride
    # the median, and the identity index against no index
    ident = torch.arange(C, dtype=torch.int32, device=DEV)
    med = _tm(aligned[:C], (C - 1) // 2)
    assert rr.same_bits(med, rr.median(rows[:C]))
    assert rr.same_bits(_tm(aligned, (C - 1) // 2, row_index=ident), med)


def test_trimmed_mean_argument_errors():
    rows = torch.zeros(65, 8, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    for C, trim, msg in ((4, 2, "trim"), (5, 3, "trim"), (0, 0, "outside"), (65, 0, "outside")):
        with pytest.raises(FedHipError, match=msg):
            ops.trimmed_mean_rows(rows[:C], out, trim)
    with pytest.raises(FedHipError, match="HIP device"):
        ops.trimmed_mean_rows(torch.zeros(3, 8), out, 1)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()  # nothing was launched
    ops.trimmed_mean_rows(rows[:3], out, 1, P=0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


# ------------------------------------------------------------------ pairwise distances
def _pw(view, row_index=None):
    d = ops.pairwise_sqdist(view, row_index=row_index)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("C", [2, 3, 7, 32, 33, 64])
def test_pairwise_sqdist_exact_on_small_integers(C):
    """|x| <= 8: every term (<= 256) and every partial sum is an integer far below 2^53, so
    the result is exact whatever the chunking and must equal the reference exactly."""
    rng = np.random.default_rng(C)
    for P in (1, 5, 1001, 4099):
        rows = rng.integers(-8, 9, size=(C, P)).astype(np.float32)
        want = rr.pairwise_sqdist(rows)
        for stride in ((P | 1) + 2, (P + 3) // 4 * 4):  # odd, and a multiple of 4
            d = _pw(_place(rows, stride, 0))
            assert d.dtype == np.float64 and d.shape == (C, C)
            assert np.array_equal(d, want), (P, stride)
            assert np.array_equal(d, d.T) and not d.diagonal().any()


def test_pairwise_sqdist_many_tiles_row_index_and_replay():
    """P = 131077: chunks of 192 columns, 3 LDS tiles each, 683 chunks, a 5-column tail."""
    C, tall, P = 7, 10, 131077
    rng = np.random.default_rng(5)
    rows = rng.integers(-8, 9, size=(tall, P)).astype(np.float32)
    pick = rng.permutation(tall)[:C]
    view = _place(rows, P + 2, 1)
    idx = torch.tensor(pick, dtype=torch.int32, device=DEV)
    d = _pw(view, idx)
    assert np.array_equal(d, rr.pairwise_sqdist(rows[pick]))
    assert np.array_equal(_pw(view), rr.pairwise_sqdist(rows))
    # normal data: the reference differs only in the order of the fp64 sum of P non-negative
    # terms, so |d - ref| <= P * 2^-53 * ref
    x = rng.standard_normal((C, P)).astype(np.float32)
    xv = _place(x, P + 3, 0)
    got, want = _pw(xv), rr.pairwise_sqdist(x)
    print("pairwise normal-data max rel err", np.max(np.abs(got - want) / np.maximum(want, 1)))
    assert np.all(np.abs(got - want) <= P * 2.0 ** -53 * want)
    assert np.array_equal(got.view(np.uint64), _pw(xv).view(np.uint64))  # same bits again


def test_pairwise_sqdist_argument_errors():
    rows = torch.zeros(65, 8, device=DEV)
    for C in (1, 65):
        with pytest.raises(FedHipError, match="outside"):
            ops.pairwise_sqdist(rows[:C])


# ------------------------------------------------------------------ aggregators
SHAPES = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}


def _updates(n, seed, attackers=(), scale=-5.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    ups = []
    for k in range(n):
        w = {name: 0.3 * torch.randn(*shape, generator=g) for name, shape in SHAPES.items()}
        if k in attackers:
            w = {name: scale * t + shift for name, t in w.items()}
        ups.append(ModelUpdate(client_id=f"c{k}", round_number=1, model_weights=w,
                               num_samples=10 + k, training_loss=0.5, privacy_budget_used=0.5,
                               compression_ratio=0.8, timestamp=datetime.now()))
    return ups


def _flat(weights):
    return np.concatenate([weights[n].detach().cpu().numpy().reshape(-1) for n in SHAPES])


def test_trimmed_mean_and_median_aggregators_resist_scaled_clients():
    attackers = (2, 5)
    for ups in (_updates(7, 1), _updates(7, 1, attackers)):
        rows = np.stack([_flat(u.model_weights) for u in ups])
        for agg, trim in ((robust.TrimmedMeanAggregator(trim_ratio=0.3), 2),
                          (robust.MedianAggregator(), 3)):
            gm = agg.aggregate_updates(ups)
            assert [gm.model_weights[n].shape for n in SHAPES] == [torch.Size(s)
                                                                   for s in SHAPES.values()]
            assert rr.same_bits(_flat(gm.model_weights), rr.trimmed_mean(rows, trim))
            h = agg.aggregation_history[-1]
            assert h["num_clients"] == 7 and h["client_samples"]["c3"] == 13
    honest = np.delete(rows, attackers, axis=0)
    lo, hi = honest.min(axis=0), honest.max(axis=0)
    tm = _flat(robust.TrimmedMeanAggregator(trim_ratio=0.3).aggregate_updates(ups).model_weights)
    assert np.all((tm >= lo) & (tm <= hi))
    fa = _flat(FedAvgAggregator().aggregate_updates(ups).model_weights)
    assert np.any((fa < lo) | (fa > hi))  # what the plain mean cannot do


def test_krum_aggregator_drops_outliers_and_breaks_ties_low():
    outliers = (3, 7)
    ups = _updates(9, 2, outliers, scale=1.0, shift=5.0)  # passes the magnitude validator
    rows = np.stack([_flat(u.model_weights) for u in ups])
    for kind, m in (("multi_krum", 7), ("krum", 1)):
        agg = robust.create_robust_aggregator(kind, num_byzantine=2)
        gm = agg.aggregate_updates(ups)
        sel, _ = rr.krum_select(rr.pairwise_sqdist(rows), 2, m)
        assert agg.last_selected == sel and not set(sel) & set(outliers) and len(sel) == m
        assert rr.same_bits(_flat(gm.model_weights), rr.uniform_mean(rows[sel], m))
    # duplicate rows: every score ties, the lowest indices are kept
    same = [ups[0].model_weights] * 7
    dup = [ModelUpdate(client_id=f"d{k}", round_number=1, model_weights=w, num_samples=5,
                       training_loss=0.1, privacy_budget_used=0.5, compression_ratio=0.8,
                       timestamp=datetime.now()) for k, w in enumerate(same)]
    agg = robust.KrumAggregator(num_byzantine=1, num_selected=3)
    gm = agg.aggregate_updates(dup)
    assert agg.last_selected == [0, 1, 2]
    assert rr.same_bits(_flat(gm.model_weights), rr.uniform_mean(rows[[0, 0, 0]], 3))
    # aggregate_packed through a row_index: rows of a taller matrix, result in `out`
    packed = _place(np.concatenate([rows, rows[::-1]]), 128, 0)
    pick = [17, 1, 2, 14, 4, 5, 6, 10, 8]  # = rows 0, 1, 2, 3, .. (17 - i is row i again)
    out = torch.empty(rows.shape[1], device=DEV)
    agg = robust.KrumAggregator(num_byzantine=2)
    assert agg.aggregate_packed(packed, [1] * 9, row_index=pick, out=out) is out
    assert agg.last_selected == [0, 1, 2, 4, 5, 6, 8]
    assert rr.same_bits(out.cpu().numpy(), rr.uniform_mean(rows[agg.last_selected], 7))


# ------------------------------------------------------------------ RankRound
SIZES = [70, 55, 48, 40]


def _client_data(k, n):
    g = torch.Generator().manual_seed(200 + k)
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _round(mine, aggregator="omit", exact=False, inject=None):
    """One round of SimpleCNN over SIZES' clients `mine`; returns the trained rows by client
    (copied by the on_trained hook) and the new global vector.  `inject` (rows by client)
    replaces the trained rows before aggregation."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    kw = {} if isinstance(aggregator, str) else {"aggregator": aggregator}
    r = RankRound(model, SIZES, mine, epochs=1, device=DEV, lanes=1, shuffle_seed=77,
                  exact=exact, **kw)
    xs, ys = zip(*[_client_data(k, SIZES[k]) for k in r.slots])
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            if inject is not None:
                params[r.slot_of[k], :r.P].copy_(torch.from_numpy(inject[k]))
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    r.run(data, labels, offs, "sgd", 0.01, seed=3)
    torch.cuda.synchronize()
    return seen, r.global_flat.cpu().numpy().copy()


def test_rankround_with_a_robust_aggregator_one_rank():
    all4 = list(range(4))
    rows, glob = _round(all4, robust.MedianAggregator())
    stack = np.stack([rows[k] for k in all4])
    assert rr.same_bits(glob, rr.median(stack))
    rows_t, glob_t = _round(all4, robust.TrimmedMeanAggregator(trim_ratio=0.25))
    assert rr.same_bits(glob_t, rr.trimmed_mean(np.stack([rows_t[k] for k in all4]), 1))
    # aggregator=None is today's path: same seeds, same bits as without the argument
    _, plain = _round(all4)
    _, none = _round(all4, None)
    assert rr.same_bits(plain, none) and not rr.same_bits(plain, glob)


def _rank_main(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        mine = [k for k in range(len(SIZES)) if k % world == rank]
        q.put((rank, _round(mine, robust.MedianAggregator(), exact=True)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:  # surface the failure to the parent instead of hanging it
        q.put((rank, repr(e)))
        raise


def test_rankround_median_two_ranks_exact():
    """Two gloo ranks on cuda:0 with exact=True and the median rule: both ranks end with the
    same global vector, the median of every client's trained row, and a one-rank round over
    the same clients gives the same bits.  A client's trained row depends on its packed
    layout in the last bits (split-K order, tests/test_multirank_gpu.py), so the one-rank
    round aggregates the rows the two ranks trained, put in place by the on_trained hook."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29560 + os.getpid() % 200
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
    (rows0, glob0), (rows1, glob1) = res[0], res[1]
    assert sorted(list(rows0) + list(rows1)) == list(range(len(SIZES)))
    assert rr.same_bits(glob0, glob1), "ranks disagree on the global model"
    rows = {**rows0, **rows1}
    assert rr.same_bits(glob0, rr.median(np.stack([rows[k] for k in range(len(SIZES))])))
    _, one = _round(list(range(len(SIZES))), robust.MedianAggregator(), inject=rows)
    assert rr.same_bits(glob0, one)
