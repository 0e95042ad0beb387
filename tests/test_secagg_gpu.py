"""The secure-aggregation kernels (csrc/secagg.hip) and SecureAggregator on the GPU, against
the numpy reference of tests/secagg_ref.py (pinned by test_secagg_ref_cpu.py).

Everything after the one rounded fp32 multiply of the encoding is exact or an integer mod
2^32, so fh_secagg_encode_mask_rows and fh_secagg_sum_decode are held to the reference bit for
bit: over sizes below / across the 4-coordinate Philox block and the 256-thread workgroup,
every legal kind of term list, the 16-byte path and the scalar path (odd strides, bases 4
bytes off 16), permuted row indices, and data that holds NaN, +-Inf, +-0, denormals, exact
ties and values at and one step beyond the saturation bound.  The aggregator is compared with
FedAvgAggregator within the derived bound

    |secure - fedavg|[j] <= C * 2^-(frac_bits+1) + (C + 1) * 2^-24 * sum_k |fl32(w_k x_k[j])|

(per-client quantisation; the one decode rounding; the first-order bound on FedAvg's
sequential fp32 sum over the same rounded products).
"""
import numpy as np
import pytest
import torch

import secagg_ref as sr
from fedhip import ops
from fedhip._lib import FedHipError
from src.aggregation import secure
from src.aggregation.fedavg import FedAvgAggregator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENT = -1234567          # int32 sentinel around integer outputs
FSENT = -12345.5         # fp32 sentinel around the decoded row

CS = [1, 2, 3, 5, 17, 64]
PS = [1, 3, 4, 5, 13, 1001, 4099]
FRACS = [0, 16, 30]
NONCE = 2 ** 40 + 12345


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a).to(DEV)
    return t if dtype is None else t.to(dtype)


def _place(rows, stride, base_offset, fill):
    """rows [C, P] (fp32 or the int32 bits of uint32) as a device view with the given row
    stride, `base_offset` elements from a 16-B aligned base; the gaps hold `fill`."""
    rows = np.ascontiguousarray(rows)
    if rows.dtype == np.uint32:
        rows = rows.view(np.int32)
    C, P = rows.shape
    flat = torch.full((C * stride + base_offset + 4,), fill, device=DEV,
                      dtype=torch.from_numpy(rows).dtype)
    view = flat[base_offset:base_offset + C * stride].view(C, stride)[:, :P]
    view.copy_(torch.from_numpy(rows))
    return view


class Window:
    """[C, P] output view with row stride `stride`, `offset` elements from the 16-B base of a
    sentinel-filled buffer; read() returns the view's content and checks the rest."""

    def __init__(self, C, P, stride, offset, dtype, sentinel):
        self.C, self.P, self.stride, self.offset, self.sentinel = C, P, stride, offset, sentinel
        self.buf = torch.full((C * stride + offset + 8,), sentinel, device=DEV, dtype=dtype)
        self.view = self.buf[offset:offset + C * stride].view(C, stride)[:, :P]

    def read(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy().copy()
        region = b[self.offset:self.offset + self.C * self.stride].reshape(self.C, self.stride)
        got = region[:, :self.P].copy()
        region[:, :self.P] = self.sentinel
        assert (b == self.sentinel).all(), "a write outside the output rows"
        return got


def _data(C, P, seed, frac_bits, qmax):
    """Normal draws at 0.4 of the saturation bound (about 1 % beyond it), with the special
    values planted: NaN, +-Inf, +-0, denormals, exact .5 ties, +-qmax and one step beyond."""
    rng = np.random.default_rng(seed)
    step = 2.0 ** -frac_bits
    rows = (rng.standard_normal((C, P)) * (0.4 * qmax * step)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 0.5 * step,
                        1.5 * step, 2.5 * step, -0.5 * step, -1.5 * step, qmax * step,
                        -qmax * step, (qmax + 1) * step, -(qmax + 1) * step, 3e38, -3e38],
                       dtype=np.float32)
    n = min(P, len(special))
    for z in range(C):
        cols = rng.permutation(P)[:n]
        rows[z, cols] = special[(z + np.arange(n)) % len(special)]
    return rows


def _terms(rng, Z, nterms):
    keys = rng.integers(0, 2 ** 64, size=(Z, nterms), dtype=np.uint64)
    signs = rng.choice(np.array([1, -1, 0], dtype=np.int32), size=(Z, nterms), p=[0.4, 0.4, 0.2])
    return keys, signs


# ------------------------------------------------------------------ encode + mask
@pytest.mark.parametrize("ci", range(len(CS)))
def test_encode_mask_rows_bits(ci):
    C = CS[ci]
    for i, P in enumerate(PS):
        nterms = [64, C - 1, 0, 1][(i + ci) % 4]
        frac = FRACS[(i + ci) % 3]
        # 2^24 - 1 is an fp32 number, so "at the bound" and "one step beyond" are exact there
        qmax = (2 ** 31 - 1) // C if i % 2 else 2 ** 24 - 1
        rng = np.random.default_rng(1000 * C + P)
        tall = C + 3
        rows = _data(tall, P, 77 * C + P, frac, qmax)
        weights = None
        if (i + ci) % 2 == 0:
            weights = rng.uniform(0.05, 1.0, size=C).astype(np.float32)
            weights[0] = 1.0  # this row keeps its planted values exactly
        pick = rng.permutation(tall)[:C] if i % 3 else None
        keys, signs = _terms(rng, C, nterms)
        sel = rows[:C] if pick is None else rows[pick]
        want, nclip = sr.encode_mask_rows(sel, weights, frac, qmax, keys if nterms else None,
                                          signs, NONCE)
        assert nclip.sum() > 0 or P < 13
        kt, st = (_dev(keys), _dev(signs)) if nterms else (None, None)
        wt = None if weights is None else _dev(weights)
        idx = None if pick is None else _dev(pick.astype(np.int32))
        nr = C if pick is None else tall
        vs = (P + 3) // 4 * 4 + 4
        # (row stride, row base, out stride, out base): the 16-byte path, then the scalar
        # path for each reason it is taken
        for rs, rb, os_, ob in ((vs, 0, vs, 0), (P | 1, 0, vs, 0), (vs, 0, vs + 1, 0),
                                (vs, 1, vs, 0), (vs, 0, vs, 1)):
            src = _place(rows[:nr], rs, rb, float("nan"))
            win = Window(C, P, os_, ob, torch.int32, SENT)
            start = np.arange(7, 7 + C, dtype=np.int32)
            clipped = _dev(start)
            ops.secagg_encode_mask_rows(src, win.view, frac, qmax, kt, st, NONCE, weights=wt,
                                        row_index=idx, clipped=clipped)
            got = win.read().view(np.uint32)
            assert np.array_equal(got, want), (C, P, nterms, frac, rs, rb, os_, ob)
            assert np.array_equal(clipped.cpu().numpy(), start + nclip), (C, P, rs, rb, os_, ob)
        # no clip counter is a legal call with the same rows
        win = Window(C, P, vs, 0, torch.int32, SENT)
        ops.secagg_encode_mask_rows(_place(rows[:nr], vs, 0, float("nan")), win.view, frac, qmax,
                                    kt, st, NONCE, weights=wt, row_index=idx)
        assert np.array_equal(win.read().view(np.uint32), want)


def test_encode_more_rows_than_one_grid_dimension():
    """65540 rows: past the 65535 workgroups of the grid's row dimension."""
    Z, P, frac, qmax = 65540, 5, 16, 2 ** 24 - 1
    rng = np.random.default_rng(9)
    rows = (rng.standard_normal((Z, P)) * 100).astype(np.float32)
    rows[::1000, 1] = np.nan
    keys, signs = _terms(rng, Z, 1)
    q, nclip = sr.encode(rows, None, frac, qmax)
    m = sr.masks(keys[:, 0], 0, P)  # [Z, P]: one term per row, nonce 0
    want = q + (m.astype(np.int64) * signs).astype(np.uint32)  # wraps mod 2^32
    for stride in (8, 5):  # the 16-byte path with a scalar tail, and the scalar path
        win = Window(Z, P, stride, 0, torch.int32, SENT)
        clipped = torch.zeros(Z, dtype=torch.int32, device=DEV)
        ops.secagg_encode_mask_rows(_place(rows, stride, 0, float("nan")), win.view, frac, qmax,
                                    _dev(keys), _dev(signs), 0, clipped=clipped)
        assert np.array_equal(win.read().view(np.uint32), want)
        assert np.array_equal(clipped.cpu().numpy(), nclip)


def test_encode_argument_errors():
    rows = torch.zeros(4, 8, device=DEV)
    win = Window(4, 8, 8, 0, torch.int32, SENT)
    k = torch.zeros(4, 2, dtype=torch.int64, device=DEV)
    s = torch.ones(4, 2, dtype=torch.int32, device=DEV)
    for kw, msg in (({"frac_bits": 31}, "frac_bits"), ({"qmax": 0}, "qmax")):
        a = {"frac_bits": 16, "qmax": 100, **kw}
        with pytest.raises(FedHipError, match=msg):
            ops.secagg_encode_mask_rows(rows, win.view, a["frac_bits"], a["qmax"], k, s, 1)
    k65 = torch.zeros(4, 65, dtype=torch.int64, device=DEV)
    with pytest.raises(FedHipError, match="nterms"):
        ops.secagg_encode_mask_rows(rows, win.view, 16, 100, k65, torch.ones_like(k65).int(), 1)
    with pytest.raises(FedHipError, match="shape"):
        ops.secagg_encode_mask_rows(rows, win.view, 16, 100, k[:3], s[:3], 1)
    with pytest.raises(FedHipError, match="go together"):
        ops.secagg_encode_mask_rows(rows, win.view, 16, 100, k, None, 1)
    with pytest.raises(FedHipError, match="HIP device"):
        ops.secagg_encode_mask_rows(torch.zeros(4, 8), win.view, 16, 100, k, s, 1)
    ops.secagg_encode_mask_rows(rows, win.view, 16, 100, k, s, 1, P=0)
    assert (win.read() == SENT).all()  # nothing was written


# ------------------------------------------------------------------ sum + unmask + decode
@pytest.mark.parametrize("nterms", [0, 1, 7, 1024 + 32])
def test_sum_decode_bits(nterms):
    rng = np.random.default_rng(nterms + 1)
    for i, (K, P) in enumerate(((1, 1), (5, 5), (9, 1001), (4, 4099), (64, 13))):
        frac = FRACS[(i + nterms) % 3]
        tall = K + 2
        masked = rng.integers(0, 2 ** 32, size=(tall, P), dtype=np.uint64).astype(np.uint32)
        masked[0, : min(P, 4)] = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0][: min(P, 4)]
        pick = rng.permutation(tall)[:K] if i % 2 else None
        keys, signs = _terms(rng, 1, nterms)
        keys, signs = keys[0], signs[0]
        sel = masked[:K] if pick is None else masked[pick]
        want_f, want_u = sr.sum_decode(sel, keys if nterms else None, signs, NONCE, frac)
        kt, st = (_dev(keys), _dev(signs)) if nterms else (None, None)
        idx = None if pick is None else _dev(pick.astype(np.int32))
        nr = K if pick is None else tall
        vs = (P + 3) // 4 * 4 + 4
        # (row stride, row base, base of out, base of sum_out, which outputs)
        for rs, rb, fo, so, which in ((vs, 0, 0, 0, "both"), (vs, 0, 4, 8, "out"),
                                      (vs, 0, 0, 4, "sum"), (P | 1, 0, 0, 0, "both"),
                                      (vs, 1, 0, 0, "sum"), (vs, 0, 1, 0, "both"),
                                      (vs, 0, 0, 3, "both"), (vs, 0, 1, 0, "out")):
            src = _place(sel if pick is None else masked[:nr], rs, rb, SENT)
            fw = Window(1, P, P, fo, torch.float32, FSENT)
            uw = Window(1, P, P, so, torch.int32, SENT)
            ops.secagg_sum_decode(src, frac, kt, st, NONCE, row_index=idx,
                                  out=fw.view[0] if which != "sum" else None,
                                  sum_out=uw.view[0] if which != "out" else None)
            f, u = fw.read()[0], uw.read()[0]
            tag = (nterms, K, P, rs, rb, fo, so, which)
            if which != "sum":
                assert sr.same_bits(f, want_f), tag
            else:
                assert (f == FSENT).all(), tag
            if which != "out":
                assert np.array_equal(u.view(np.uint32), want_u), tag
            else:
                assert (u == SENT).all(), tag


def test_sum_decode_argument_errors():
    masked = torch.zeros(3, 8, dtype=torch.int32, device=DEV)
    out = torch.full((8,), FSENT, device=DEV)
    with pytest.raises(FedHipError, match="out / sum_out"):
        ops.secagg_sum_decode(masked, 16)
    with pytest.raises(FedHipError, match="frac_bits"):
        ops.secagg_sum_decode(masked, 31, out=out)
    with pytest.raises(FedHipError, match="int32"):
        ops.secagg_sum_decode(masked.float(), 16, out=out)
    ops.secagg_sum_decode(masked, 16, out=out, P=0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FSENT).all()


# ------------------------------------------------------------------ the aggregator, end to end
SEED = 0x0123456789ABCDEF
E2E_P = 4099


def _ids(C):
    ids = [2 ** 33 + 1, 4, 2 ** 64 - 2, 0, 9]
    return (ids + list(range(100, 100 + C)))[:C]


def _ring_sum(u32_rows):
    return (np.asarray(u32_rows).astype(np.uint64).sum(axis=0)
            & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _e2e_rows(C, P):
    rng = np.random.default_rng(C)
    rows = (0.1 * rng.standard_normal((C, P))).astype(np.float32)
    rows[0, 5], rows[C - 1, 7], rows[C // 2, 11] = np.nan, 1e30, -np.inf
    samples = [int(n) for n in rng.integers(20, 200, size=C)]
    return rows, samples


def _agg(**kw):
    return secure.SecureAggregator(session_seed=SEED, device=DEV, **kw)


@pytest.mark.parametrize("C", [2, 5, 33])
def test_masks_cancel_hide_and_recover_after_dropouts(C):
    P, frac = E2E_P, 16
    rows, samples = _e2e_rows(C, P)
    ids = _ids(C)
    w = sr.fedavg_weights(samples)
    qmax = (2 ** 31 - 1) // C
    q, qclip = sr.encode(rows, w, frac, qmax)
    keys, signs = sr.client_terms(SEED, ids)
    want_masked, _ = sr.encode_mask_rows(rows, w, frac, qmax, keys, signs, 0)
    agg = _agg(frac_bits=frac)
    packed = _dev(rows)
    masked, clipped = agg.mask(packed, samples, client_ids=ids)
    assert masked.dtype == torch.int32 and tuple(masked.shape) == (C, P) and agg.nonce == 1
    got = masked.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want_masked)
    assert np.array_equal(clipped.cpu().numpy(), qclip) and qclip.sum() == 3
    assert agg.last_clipped is clipped
    # the masks cancel: the ring sum of the masked rows is the ring sum of the plain codes
    _, s = ops.secagg_sum_decode(masked, frac, sum_out=torch.empty(P, dtype=torch.int32,
                                                                   device=DEV))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), _ring_sum(q))
    assert np.array_equal(_ring_sum(got), _ring_sum(q))
    # ... and hide: a word equals its plain code by chance with probability 2^-32
    assert ((got == q).sum(axis=1) <= 4).all()
    # nobody dropped: the decoded row is the reference's, whatever the row order
    want = sr.decode(_ring_sum(q), frac)
    assert sr.same_bits(agg.unmask_sum(masked, ids).cpu().numpy(), want)
    perm = np.random.default_rng(1).permutation(C)
    agg2 = _agg(frac_bits=frac)
    m2, _ = agg2.mask(_dev(rows[perm]), [samples[i] for i in perm],
                      client_ids=[ids[i] for i in perm])
    assert np.array_equal(m2.cpu().numpy().view(np.uint32), want_masked[perm])
    assert sr.same_bits(agg2.unmask_sum(m2, [ids[i] for i in perm]).cpu().numpy(), want)
    # rows picked out of a taller matrix give the same masked rows
    tall = np.concatenate([rows[::-1], rows[:1]])
    agg3 = _agg(frac_bits=frac)
    m3, _ = agg3.mask(_dev(tall), samples, client_ids=ids,
                      row_index=[C - 1 - k for k in range(C)])
    assert np.array_equal(m3.cpu().numpy().view(np.uint32), want_masked)
    # dropouts after masking: the survivors' sum comes back exactly
    for ndrop in sorted({1, C // 2}):
        gone = [ids[i] for i in np.random.default_rng(ndrop).permutation(C)[:ndrop]]
        surv = [c for c in ids if c not in gone]
        keep = [ids.index(c) for c in surv]
        n_s = sum(samples[i] for i in keep)
        plain = sr.decode(_ring_sum(q[keep]), frac)
        want_s = (np.float32(sum(samples) / n_s) * plain).astype(np.float32)
        got_s = agg.unmask_sum(masked, surv, gone).cpu().numpy()
        assert sr.same_bits(got_s, want_s), (C, ndrop)
        # without the server's terms the survivors' rows do not decode
        raw, _ = ops.secagg_sum_decode(masked, frac, row_index=_dev(np.array(keep, np.int32)),
                                       out=torch.empty(P, device=DEV))
        assert (raw.cpu().numpy() != plain).sum() > P - 8


@pytest.mark.parametrize("C", [2, 5, 33])
def test_self_masks_recover_exactly(C):
    P, frac = 1001, 12
    rows, samples = _e2e_rows(C, P)
    ids = _ids(C)
    w = sr.fedavg_weights(samples)
    q, _ = sr.encode(rows, w, frac, (2 ** 31 - 1) // C)
    agg = _agg(frac_bits=frac, self_masks=True)
    agg.nonce = NONCE
    masked, _ = agg.mask(_dev(rows), samples, client_ids=ids)
    keys, signs = sr.client_terms(SEED, ids, self_masks=True)
    want_masked, _ = sr.encode_mask_rows(rows, w, frac, (2 ** 31 - 1) // C, keys, signs, NONCE)
    got = masked.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want_masked)
    assert not np.array_equal(_ring_sum(got), _ring_sum(q))  # the self masks do not cancel
    assert sr.same_bits(agg.unmask_sum(masked, ids).cpu().numpy(),
                        sr.decode(_ring_sum(q), frac))
    for ndrop in sorted({1, C // 2}):
        gone = ids[:ndrop]
        keep = list(range(ndrop, C))
        n_s = sum(samples[i] for i in keep)
        want = (np.float32(sum(samples) / n_s) * sr.decode(_ring_sum(q[keep]), frac))
        got_s = agg.unmask_sum(masked, ids[ndrop:], gone).cpu().numpy()
        assert sr.same_bits(got_s, want.astype(np.float32)), (C, ndrop)


def test_same_nonce_same_bits_next_nonce_other_rows_same_sum():
    C, P = 5, 1001
    rows, samples = _e2e_rows(C, P)
    packed = _dev(rows)
    agg = _agg()
    agg.nonce = 7
    m1, _ = agg.mask(packed, samples)
    d1 = agg.unmask_sum(m1, list(range(C))).cpu().numpy()
    assert agg.nonce == 8
    agg.nonce = 7
    m2, _ = agg.mask(packed, samples)
    assert torch.equal(m1, m2)
    m3, _ = agg.mask(packed, samples)  # nonce 8
    assert agg.nonce == 9
    assert ((m3 == m1).sum(dim=1) <= 4).all()
    assert sr.same_bits(agg.unmask_sum(m3, list(range(C))).cpu().numpy(), d1)
    # aggregate_packed is the two stages in a row, and writes into `out`
    out = torch.empty(P, device=DEV)
    assert agg.aggregate_packed(packed, samples, out=out) is out
    assert sr.same_bits(out.cpu().numpy(), d1) and agg.nonce == 10


def _fedavg_bound(rows, samples, frac):
    """C * 2^-(frac+1) + (C + 1) * 2^-24 * sum_k |fl32(w_k x_k[j])| per coordinate, in fp64."""
    C = len(samples)
    w32 = np.array(sr.fedavg_weights(samples), dtype=np.float32)
    prod = (w32[:, None] * rows).astype(np.float32).astype(np.float64)
    return C * 2.0 ** -(frac + 1) + (C + 1) * 2.0 ** -24 * np.abs(prod).sum(axis=0)


@pytest.mark.parametrize("C,frac", [(2, 16), (5, 8), (17, 24), (64, 16), (64, 20)])
def test_secure_aggregate_within_the_bound_of_fedavg(C, frac):
    P = 4099
    rng = np.random.default_rng(C + frac)
    rows = (0.1 * rng.standard_normal((C, P))).astype(np.float32)
    samples = [int(n) for n in rng.integers(20, 200, size=C)]
    packed = _place(rows, 4160, 0, float("nan"))  # a padded row stride, as the engine packs
    agg = _agg(frac_bits=frac)
    got = agg.aggregate_packed(packed, samples).cpu().numpy().astype(np.float64)
    assert not agg.last_clipped.cpu().numpy().any()
    assert not sr.encode(rows, sr.fedavg_weights(samples), frac, agg.qmax(C))[1].any()
    ref = FedAvgAggregator(device=DEV).aggregate_packed(packed, samples).cpu().numpy()
    err, bound = np.abs(got - ref.astype(np.float64)), _fedavg_bound(rows, samples, frac)
    print(f"C={C} frac={frac}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # with a row order of its own
    order = rng.permutation(C)
    got2 = agg.aggregate_packed(packed, [samples[i] for i in order],
                                row_index=[int(i) for i in order]).cpu().numpy()
    assert sr.same_bits(got2, got.astype(np.float32))


def test_aggregate_updates_goes_through_the_masked_rows():
    from datetime import datetime

    from src.shared.models import ModelUpdate
    shapes = {"conv.weight": (4, 3, 3), "fc.weight": (13, 5), "fc.bias": (7,)}
    g = torch.Generator().manual_seed(5)
    ups = [ModelUpdate(client_id=f"c{k}", round_number=1,
                       model_weights={n: 0.3 * torch.randn(*s, generator=g)
                                      for n, s in shapes.items()},
                       num_samples=10 + k, training_loss=0.5, privacy_budget_used=0.5,
                       compression_ratio=0.8, timestamp=datetime.now()) for k in range(6)]
    rows = np.stack([np.concatenate([u.model_weights[n].numpy().reshape(-1) for n in shapes])
                     for u in ups])
    samples = [u.num_samples for u in ups]
    agg = _agg()
    gm = agg.aggregate_updates(ups)
    flat = np.concatenate([gm.model_weights[n].cpu().numpy().reshape(-1) for n in shapes])
    want, _, _ = sr.secure_fedavg(rows, samples, list(range(6)), SEED, 0, 16)
    assert sr.same_bits(flat, want)
    assert [tuple(gm.model_weights[n].shape) for n in shapes] == list(shapes.values())
    ref = FedAvgAggregator(device=DEV).aggregate_updates(ups)
    ref_flat = np.concatenate([ref.model_weights[n].cpu().numpy().reshape(-1) for n in shapes])
    assert np.all(np.abs(flat.astype(np.float64) - ref_flat) <= _fedavg_bound(rows, samples, 16))
    assert agg.aggregation_history[-1]["num_clients"] == 6


# ------------------------------------------------------------------ RankRound
SIZES = [70, 55, 48, 40]


def _client_data(k, n):
    g = torch.Generator().manual_seed(200 + k)
    return torch.randn(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)


def _round(aggregator):
    """One round of SimpleCNN over SIZES' clients on one rank; returns the trained rows by
    client (copied by the on_trained hook), the new global vector and the BN statistics."""
    from fedhip.round import RankRound
    from src.shared import models_pytorch as hm
    torch.manual_seed(0)
    model = hm.ModelFactory.create_model("simple_cnn").to(DEV)
    r = RankRound(model, SIZES, list(range(len(SIZES))), epochs=1, device=DEV, lanes=1,
                  shuffle_seed=77, aggregator=aggregator)
    xs, ys = zip(*[_client_data(k, SIZES[k]) for k in r.slots])
    data, labels = torch.cat(xs).to(DEV), torch.cat(ys).to(DEV)
    offs = np.cumsum([0] + [SIZES[k] for k in r.slots][:-1]).tolist()
    seen = {}

    def hook(params, S):
        for k in r.clients:
            seen[k] = params[r.slot_of[k], :r.P].cpu().numpy().copy()
    r.on_trained = hook
    r.run(data, labels, offs, "sgd", 0.01, seed=3)
    torch.cuda.synchronize()
    return seen, r.global_flat.cpu().numpy().copy(), r.global_bufs.cpu().numpy().copy(), r


def test_rankround_with_the_secure_aggregator_one_rank():
    agg = _agg()
    rows_s, glob_s, bufs_s, r = _round(agg)
    rows_p, glob_p, bufs_p, _ = _round(None)
    clients = list(r.clients)
    for k in clients:  # the same seeds train the same rows
        assert sr.same_bits(rows_s[k], rows_p[k])
    stack = np.stack([rows_s[k] for k in clients])
    samples = [SIZES[k] for k in clients]  # one epoch: samples processed = train size
    assert not agg.last_clipped.cpu().numpy().any() and agg.nonce == 1
    # the masks cancelled: the global vector is the decoded ring sum of the plain codes
    q, _ = sr.encode(stack, sr.fedavg_weights(samples), 16, agg.qmax(len(clients)))
    assert sr.same_bits(glob_s, sr.decode(_ring_sum(q), 16))
    err = np.abs(glob_s.astype(np.float64) - glob_p.astype(np.float64))
    bound = _fedavg_bound(stack, samples, 16)
    print(f"RankRound: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound) and not sr.same_bits(glob_s, glob_p)
    assert np.array_equal(bufs_s.view(np.uint32), bufs_p.view(np.uint32))
