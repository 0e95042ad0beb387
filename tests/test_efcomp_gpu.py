"""csrc/efcomp.hip on the device, bit for bit against tests/efcomp_ref.py: fh_ef_fold,
fh_ef_topk_finish, fh_ef_quant_finish, fh_squant_rows, their chaining in compress_rows and in
RankRound(compression=CompressionConfig(error_feedback=..., stochastic=...)).

Shapes: 3 client rows, segments of 1, 7, 8191, 8193 and 300 elements behind a lead of 5 (edges
on both sides of an fh_compress_chunk_elems() boundary, a one-element segment, segment starts
on no 16-byte boundary).  "aligned": every tensor 16-byte aligned with a row stride that is a
multiple of 4 floats (the float4 path with scalar heads and tails).  "scalar": row stride W + 1
and every pointer one element off — rows whose tensors disagree on the offset run one element
per thread, the row where they agree runs float4 groups that straddle two Philox blocks.
The base is one broadcast row (stride 0) or one row per client.  Every buffer has a padding row
and is pre-filled with a NaN pattern (0xA5 for bytes); everything outside
[seg_offsets[0], seg_offsets[nseg]) of the client rows must keep it.

No tolerances: floats are compared by their int32 view."""
import functools

import numpy as np
import pytest
import torch

import efcomp_ref as er
from fedhip._lib import FedHipError
from fedhip.compress import (CompressionConfig, SegmentPlan, compress_rows, ef_fold,
                             ef_topk_finish, squant_rows, topk_rows)
from oracle import fedavg_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F = np.float32

C = 3
LEAD, TAIL = 5, 9
LENS = [1, 7, 8191, 8193, 300]
SEG = np.concatenate([[LEAD], LEAD + np.cumsum(LENS)]).tolist()
A, E = SEG[0], SEG[-1]
W = E + TAIL
NSEG = len(LENS)
POISON_I32 = 0x7FC0BEEF          # a quiet NaN with a payload
POISON_U8 = 0xA5
VARIANTS = ["aligned", "scalar"]
MODES = ["broadcast", "per_row"]
IDS = [7, 12, 7]
KEY = 0x0123456789ABCDEF


def i32(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    return np.array_equal(i32(a), i32(b))


class Buf:
    """[C + 1, stride] device rows over one poisoned flat allocation; .view is [:C, :W]."""

    def __init__(self, variant, dtype=torch.float32, rows=C + 1):
        self.u8 = dtype != torch.float32
        self.stride = (W + 3) // 4 * 4 + 4 if variant == "aligned" else W + 1
        self.off = 0 if variant == "aligned" else 1
        n = rows * self.stride
        if self.u8:
            self.flat = torch.full((n + 16,), POISON_U8, dtype=dtype, device=DEV)
        else:
            self.flat = torch.full((n + 4,), POISON_I32, dtype=torch.int32,
                                   device=DEV).view(torch.float32)
        self.full = self.flat[self.off:self.off + n].view(rows, self.stride)
        self.view = self.full[:C, :W]
        assert self.flat.data_ptr() % 16 == 0 and self.view.stride(0) == self.stride

    def put(self, arr):
        self.view[:, A:E] = torch.from_numpy(np.ascontiguousarray(arr[:, A:E])).to(DEV)
        return self

    def get(self):
        return self.view.cpu().numpy()[:, A:E]

    def assert_poison_outside(self):
        mask = torch.ones(self.flat.shape, dtype=torch.bool, device=DEV)
        n = self.full.numel()
        mask[self.off:self.off + n].view(self.full.shape)[:C, A:E] = False
        flat = self.flat if self.u8 else self.flat.view(torch.int32)
        assert bool((flat[mask] == (POISON_U8 if self.u8 else POISON_I32)).all())


class Base:
    def __init__(self, variant, arr):
        """arr: [1, W] (broadcast, stride 0) or [C, W]."""
        arr = np.array(arr, F)
        if arr.shape[0] == 1:
            off = 0 if variant == "aligned" else 1
            self.flat = torch.zeros(W + 4, device=DEV)
            self.flat[off:off + W] = torch.from_numpy(arr[0]).to(DEV)
            self.view = self.flat[off:off + W].view(1, W).expand(C, -1)
            assert self.view.stride(0) == 0
        else:
            b = Buf(variant)
            b.full[:C, :W] = torch.from_numpy(arr).to(DEV)
            self.flat, self.view = b.flat, b.view
        self.before = self.flat.clone()

    def assert_unchanged(self):
        assert torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32))


def grid(rng, shape, step=2.0 ** -10, amp=0.25):
    m = int(round(amp / step))
    return (rng.integers(-m, m + 1, size=shape) * step).astype(F)


@functools.lru_cache(maxsize=None)
def make_base(mode):
    rng = np.random.default_rng(7 + (mode == "per_row"))
    b = grid(rng, (1 if mode == "broadcast" else C, W))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def plan():
    p = SegmentPlan(SEG, DEV)
    assert p.chunk == 8192 and p.nchunks == NSEG + 1     # only the 8193 segment has two chunks
    return p


# ------------------------------------------------------------------ fold + top-k + finish
@functools.lru_cache(maxsize=None)
def topk_problem(ratio, mode, integer):
    """Three rounds of updates and the reference's x_out / resid / keep after each."""
    rng = np.random.default_rng(int(ratio * 10) + 100 * (mode == "per_row") + 1000 * integer)
    base = make_base(mode)
    if integer:
        base = (base * F(2.0 ** 14)).astype(F)           # integers, |b| <= 2^12
    resid = np.zeros((C, W), F)
    rounds = []
    for t in range(3):
        if integer:
            delta = rng.integers(-1023, 1024, size=(C, W)).astype(F)
        else:
            delta = (rng.standard_normal((C, W)) * 0.05).astype(F)
        x = (base + delta).astype(F)
        x_out, resid, keep, v = er.ef_topk_round(x, base, resid, SEG, ratio)
        rounds.append({"x": x, "delta": delta, "x_out": x_out, "resid": resid, "keep": keep})
    return base, rounds


def run_topk_rounds(variant, ratio, mode, integer=False):
    base_np, rounds = topk_problem(ratio, mode, integer)
    base = Base(variant, np.asarray(base_np))
    resid = Buf(variant).put(np.zeros((C, W), F))
    got = []
    for r in rounds:
        x = Buf(variant).put(r["x"])
        keep = Buf(variant, torch.uint8)
        ef_fold(plan(), x.view, resid.view, C, base=base.view)
        topk_rows(plan(), resid.view, C, ratio, keep=keep.view)
        ef_topk_finish(plan(), keep.view, resid.view, x.view, C, base=base.view)
        torch.cuda.synchronize()
        for b in (x, keep, resid):
            b.assert_poison_outside()
        base.assert_unchanged()
        got.append((x.get(), resid.get(), keep.get()))
    return base_np, rounds, got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ratio", [0.9, 0.0, 1.0])
@pytest.mark.parametrize("variant", VARIANTS)
def test_ef_topk_three_rounds(variant, ratio, mode):
    _, rounds, got = run_topk_rounds(variant, ratio, mode)
    for t, (r, (x_out, resid, keep)) in enumerate(zip(rounds, got)):
        assert np.array_equal(keep, r["keep"][:, A:E]), t
        assert same(x_out, r["x_out"][:, A:E]), t
        assert same(resid, r["resid"][:, A:E]), t
    k = [er.compress_ref.topk_k(n, ratio) for n in LENS]
    assert int(got[0][2][0].sum()) == sum(k)
    if ratio == 0.0:   # everything kept: nothing is left behind
        assert not i32(got[-1][1]).any()
    else:
        assert np.abs(got[-1][1]).max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_ef_topk_telescopes_on_the_device(variant):
    """Integer deltas below 2^10 over an integer base: sum_t sent_t + resid_R == sum_t delta_t
    exactly, from the device's own outputs."""
    base_np, rounds, got = run_topk_rounds(variant, 0.9, "broadcast", integer=True)
    b = np.asarray(base_np, np.float64)[:, A:E]
    sent = sum(x_out.astype(np.float64) - b for x_out, _, _ in got)
    total = sum(r["delta"][:, A:E].astype(np.float64) for r in rounds)
    assert np.array_equal(sent + got[-1][1], total)
    assert (sent != total).any()


# ------------------------------------------------------------------ stochastic quantiser
@functools.lru_cache(maxsize=None)
def squant_problem(bits, sym, mode, ef):
    rng = np.random.default_rng(bits * 8 + sym * 4 + (mode == "per_row") * 2 + ef)
    base = make_base(mode)
    delta = (rng.standard_normal((C, W)) * 0.05).astype(F)
    a4, e4 = SEG[4], SEG[5]
    delta[0, a4:e4] = 0.0                     # an all-zero segment
    delta[1, a4:e4] = 0.75                    # constant: passes through in asymmetric mode
    x = (base + delta).astype(F)
    assert same((x - base)[:2, a4:e4], delta[:2, a4:e4])   # the grid base keeps them exact
    resid = None
    if ef:
        resid = (rng.standard_normal((C, W)) * 0.02).astype(F)
        resid[:2, a4:e4] = 0.0
    ref = er.squant_round(x, base, resid, SEG, bits, sym, KEY, IDS)
    s4 = ref["scale"][:, 4]
    assert s4[0] == 0 and (s4[1] == 0) == (not sym) and s4[2] > 0
    return base, x, resid, ref


SQ_LAYOUTS = [("aligned", "broadcast", False), ("aligned", "per_row", True),
              ("scalar", "broadcast", True), ("scalar", "per_row", False)]


def run_squant(variant, bits, sym, base_np, x_np, resid_np, words=None, ids=IDS, key=KEY):
    base = None if base_np is None else Base(variant, np.asarray(base_np))
    x = Buf(variant).put(x_np)
    out = Buf(variant)
    codes = Buf(variant, torch.uint8) if bits <= 8 else None
    scale = torch.full((C, NSEG), float("nan"), device=DEV)
    lo = torch.full((C, NSEG), float("nan"), device=DEV)
    row_ids = torch.tensor(ids, dtype=torch.int64, device=DEV)
    bview = None if base is None else base.view
    if resid_np is None:
        rout = Buf(variant)
        squant_rows(plan(), x.view, C, bits, sym, key, row_ids, base=bview, out=out.view,
                    codes=None if codes is None else codes.view, resid_out=rout.view,
                    scale_out=scale, lo_out=lo, words=words)
        x_before = Buf(variant).put(x_np)
        assert torch.equal(x.flat.view(torch.int32), x_before.flat.view(torch.int32))
    else:     # the folded residual is the input; it is updated in place
        rout = Buf(variant).put(resid_np)
        ef_fold(plan(), x.view, rout.view, C, base=bview)
        squant_rows(plan(), None, C, bits, sym, key, row_ids, base=bview, resid=rout.view,
                    out=out.view, codes=None if codes is None else codes.view,
                    resid_out=rout.view, scale_out=scale, lo_out=lo, words=words)
    torch.cuda.synchronize()
    for b in (out, rout) + (() if codes is None else (codes,)):
        b.assert_poison_outside()
    if base is not None:
        base.assert_unchanged()
    return {"out": out.get(), "codes": None if codes is None else codes.get(),
            "resid": rout.get(), "scale": scale.cpu().numpy(), "lo": lo.cpu().numpy()}


def check_squant(got, ref):
    assert same(got["scale"], ref["scale"]) and same(got["lo"], ref["lo"])
    assert same(got["out"], ref["out"][:, A:E])
    if got["codes"] is not None:
        assert np.array_equal(got["codes"], ref["codes"][:, A:E])
    assert same(got["resid"], ref["err"][:, A:E])


@pytest.mark.parametrize("variant,mode,ef", SQ_LAYOUTS,
                         ids=[f"{v}-{m}-{'ef' if e else 'plain'}" for v, m, e in SQ_LAYOUTS])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("bits", [2, 4, 8, 16])
def test_squant_matches_reference(bits, sym, variant, mode, ef):
    base, x, resid, ref = squant_problem(bits, sym, mode, ef)
    got = run_squant(variant, bits, sym, base, x, resid)
    check_squant(got, ref)
    a4, e4 = SEG[4] - A, SEG[5] - A
    if got["codes"] is not None:
        assert not got["codes"][0, a4:e4].any()
        assert got["codes"][1, a4:e4].any() == sym


def test_squant_streams_follow_the_client_id():
    """The same update under ids (7, 12, 7): rows 0 and 2 draw the same words, row 1 others."""
    rng = np.random.default_rng(5)
    x = np.tile((rng.standard_normal((1, W)) * 0.05).astype(F), (C, 1))
    ref = er.squant_round(x, None, None, SEG, 4, True, KEY, IDS)
    for variant in VARIANTS:
        got = run_squant(variant, 4, True, None, x, None)
        check_squant(got, ref)
        assert np.array_equal(got["codes"][0], got["codes"][2])
        assert not np.array_equal(got["codes"][0], got["codes"][1])
    other = run_squant("aligned", 4, True, None, x, None, key=KEY + 1)
    assert not np.array_equal(other["codes"][0], got["codes"][0])


@pytest.mark.parametrize("variant", VARIANTS)
def test_squant_injected_words_equal_the_philox_path(variant):
    base, x, resid, ref = squant_problem(4, True, "broadcast", True)
    words_np = np.zeros((C, W), np.uint32)
    for z in range(C):
        words_np[z, A:E] = er.squant_words(KEY, IDS[z], np.arange(A, E))
    words = Buf(variant).view.view(torch.int32)        # uint32 rows, laid out like x
    words[:, A:E] = torch.from_numpy(np.ascontiguousarray(words_np[:, A:E]).view(np.int32)).to(DEV)
    philox = run_squant(variant, 4, True, base, x, resid)
    injected = run_squant(variant, 4, True, base, x, resid, words=words, key=0, ids=[0, 0, 0])
    check_squant(injected, ref)
    for k in ("out", "codes", "resid", "scale", "lo"):
        assert np.array_equal(philox[k].view(np.uint8), injected[k].view(np.uint8)), k
    flipped = run_squant(variant, 4, True, base, x, resid, words=(words ^ -1), key=0,
                         ids=[0, 0, 0])
    assert not np.array_equal(flipped["codes"], injected["codes"])


def test_squant_unbiased_on_the_device():
    """The CPU test's check (tests/test_efcomp_ref_cpu.py) with the same vector and keys."""
    v = er.unbiased_vector()
    n, bits = v.size, er.UNBIASED_BITS
    p = SegmentPlan([0, n], DEV)
    x = torch.from_numpy(v).to(DEV).view(1, n)
    out = torch.empty(1, n, device=DEV)
    ids = torch.tensor([er.UNBIASED_ID], dtype=torch.int64, device=DEV)
    scale = torch.zeros(1, 1, device=DEV)
    acc = torch.zeros(n, dtype=torch.float64, device=DEV)
    for key in er.UNBIASED_KEYS:
        squant_rows(p, x, 1, bits, True, key, ids, out=out, scale_out=scale)
        acc += out[0].double()
    mean = (acc / len(er.UNBIASED_KEYS)).cpu().numpy()
    s = scale.cpu().numpy()[0, 0]
    bound = er.unbiased_bound(v, s)
    err = np.abs(mean - v)
    print("max |mean - v| / scale =", err.max() / float(s), "bound / scale =", bound / float(s))
    assert err.max() <= bound
    last = er.squant_segment(v, er.squant_words(er.UNBIASED_KEYS[-1], er.UNBIASED_ID,
                                                np.arange(n)), bits, True)
    assert same(out.cpu().numpy()[0], last["deq"])
    assert np.abs(er.quant_dense(v, bits, True).astype(np.float64) - v).max() > bound


# ------------------------------------------------------------------ deterministic quantiser + EF
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("bits", [4, 8])
def test_ef_deterministic_quantiser_two_rounds(bits, sym, variant):
    rng = np.random.default_rng(bits + sym)
    base_np = make_base("broadcast")
    base = Base(variant, np.asarray(base_np))
    cfg = CompressionConfig("quantization", bits=bits, symmetric=sym, error_feedback=True)
    resid = Buf(variant).put(np.zeros((C, W), F))
    resid_np = np.zeros((C, W), F)
    for t in range(2):
        delta = (rng.standard_normal((C, W)) * 0.05).astype(F)
        delta[0, SEG[4]:SEG[5]] = 0.0
        x_np = (base_np + delta).astype(F)
        x = Buf(variant).put(x_np)
        compress_rows(plan(), cfg, x.view, C, base=base.view, resid=resid.view)
        torch.cuda.synchronize()
        x_out, resid_np = er.ef_quant_round(x_np, base_np, resid_np, SEG, bits, sym)
        x.assert_poison_outside()
        resid.assert_poison_outside()
        base.assert_unchanged()
        assert same(x.get(), x_out[:, A:E]), t
        assert same(resid.get(), resid_np[:, A:E]), t
    assert np.abs(resid_np[:, A:E]).max() > 0


def test_compress_rows_chains_equal_the_staged_calls():
    """compress_rows with error_feedback (top-k) gives the staged kernels' result."""
    base_np, rounds = topk_problem(0.9, "broadcast", False)
    base = Base("aligned", np.asarray(base_np))
    cfg = CompressionConfig("topk", sparsity_ratio=0.9, error_feedback=True)
    resid = Buf("aligned").put(np.zeros((C, W), F))
    for r in rounds[:2]:
        x = Buf("aligned").put(r["x"])
        compress_rows(plan(), cfg, x.view, C, base=base.view, resid=resid.view)
        torch.cuda.synchronize()
        x.assert_poison_outside()
        assert same(x.get(), r["x_out"][:, A:E]) and same(resid.get(), r["resid"][:, A:E])


# ------------------------------------------------------------------ RankRound
SIZES = [40, 33, 32, 1]


def _round_setup(cfg, **kw):
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn", dropout_rate=0.0).to(DEV)
    rr = RankRound(model, SIZES, list(range(4)), epochs=1, batch=32, device=DEV, lanes=1,
                   compression=cfg, dp_seed=11, shuffle_seed=5, **kw)
    g = torch.Generator().manual_seed(3)
    total = sum(SIZES)
    data = torch.randn(total, 1, 28, 28, generator=g).to(DEV)
    lab = torch.randint(0, 10, (total,), generator=g).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in rr.slots][:-1]).tolist()
    cap = {}

    def on_trained(params, S):
        cap["rows"] = params[:S, :rr.P].clone()
    rr.on_trained = on_trained
    return rr, data, lab, offs, cap


def _fedavg(rr, rows):
    w = fedavg_ref.calculate_sample_weights(SIZES)
    return fedavg_ref.weighted_average([rows[rr.slot_of[k]] for k in range(4)], w)


@pytest.mark.parametrize("cfg", [
    CompressionConfig("topk", sparsity_ratio=0.9, error_feedback=True),
    CompressionConfig("quantization", bits=4, symmetric=True, error_feedback=True,
                      stochastic=True)], ids=["topk_ef", "squant4_ef"])
def test_rank_round_error_feedback_end_to_end(cfg):
    rr, data, lab, offs, cap = _round_setup(cfg)
    seg = rr.trainer.layout.seg_offsets()
    S = len(rr.slots)
    assert tuple(rr.residual.shape) == (S, rr.P) and not rr.residual.any()
    resid = np.zeros((S, rr.P), F)
    for t in range(2):
        g0 = rr.global_flat.cpu().numpy()
        key = rr._round_key(t + 1)
        rr.run(data, lab, offs, "sgd", 0.01, seed=t + 1)
        rows = cap["rows"].cpu().numpy()
        if cfg.stochastic:
            ref = er.squant_round(rows, g0[None], resid, seg, cfg.bits, cfg.symmetric, key,
                                  rr.slots)
            x_out, resid = ref["out"], ref["resid"]
        else:
            x_out, resid, _, _ = er.ef_topk_round(rows, g0[None], resid, seg, cfg.sparsity_ratio)
        assert same(rr.residual.cpu().numpy(), resid), t
        assert same(rr.global_flat.cpu().numpy(), _fedavg(rr, x_out)), t
        assert np.abs(resid).max() > 0
    rr.reset_compression_state()
    assert not rr.residual.view(torch.int32).any()


def test_rank_round_squant_words_replay():
    """squant_words replaces the Philox words: the reference's own words give the same model."""
    cfg = CompressionConfig("quantization", bits=4, error_feedback=True, stochastic=True)
    rr, data, lab, offs, cap = _round_setup(cfg)
    g0 = rr.global_flat.clone()
    key = rr._round_key(1)
    words = np.stack([er.squant_words(key, k, np.arange(rr.P)) for k in rr.slots])
    rr.run(data, lab, offs, "sgd", 0.01, seed=1)
    g1, r1, rows = rr.global_flat.clone(), rr.residual.clone(), cap["rows"]
    assert r1.any()
    # the same round again from the same start and the same trained rows, under another key:
    # only the injected words can reproduce it
    rr.set_global(g0)
    rr.reset_compression_state()
    rr.dp_seed = 999
    rr.squant_words = torch.from_numpy(words.view(np.int32)).to(DEV)
    rr.on_trained = lambda params, S: params[:S, :rr.P].copy_(rows)
    rr.run(data, lab, offs, "sgd", 0.01, seed=1)
    assert torch.equal(rr.global_flat.view(torch.int32), g1.view(torch.int32))
    assert torch.equal(rr.residual.view(torch.int32), r1.view(torch.int32))
    rr.set_global(g0)
    rr.reset_compression_state()
    rr.squant_words = None
    rr.run(data, lab, offs, "sgd", 0.01, seed=1)
    assert not torch.equal(rr.global_flat.view(torch.int32), g1.view(torch.int32))


def test_rank_round_default_config_is_the_old_path():
    cfg = CompressionConfig()
    assert not cfg.error_feedback and not cfg.stochastic
    rr, data, lab, offs, cap = _round_setup(cfg)
    g0 = rr.global_flat.clone()
    rr.run(data, lab, offs, "sgd", 0.01, seed=1)
    assert rr.residual is None
    rows = cap["rows"].clone()
    S = rows.shape[0]
    compress_rows(rr._cplan, cfg, rows, S, base=g0.view(1, -1).expand(S, -1))   # the old call
    torch.cuda.synchronize()
    assert same(rr.global_flat.cpu().numpy(), _fedavg(rr, rows.cpu().numpy()))


# ------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(FedHipError, match="stochastic"):
        CompressionConfig("topk", stochastic=True)
    with pytest.raises(FedHipError, match="bits"):
        CompressionConfig("quantization", bits=1, stochastic=True)
    rows = torch.zeros(C, W, device=DEV)
    with pytest.raises(FedHipError, match="resid"):
        compress_rows(plan(), CompressionConfig("topk", error_feedback=True), rows, C)
    with pytest.raises(FedHipError, match="key"):
        compress_rows(plan(), CompressionConfig("quantization", stochastic=True), rows, C)
    ids = torch.zeros(C, dtype=torch.int64, device=DEV)
    with pytest.raises(FedHipError, match="bits"):
        squant_rows(plan(), rows, C, 1, True, 0, ids, out=rows)
    with pytest.raises(FedHipError, match="codes"):
        squant_rows(plan(), rows, C, 16, True, 0, ids, out=rows,
                    codes=torch.zeros(C, W, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert not rows.any()
