"""CPU tier for secure aggregation: the properties of the numpy reference of
tests/secagg_ref.py (which the GPU tests hold the kernels to, bit for bit), proof that a
comparison against it notices the plausible defects of a masker, the product's host-side key
derivation against the reference's, and everything the product validates on the host: the
argument checks of the two entry points (no launch) and the aggregator's ranges."""
import numpy as np
import pytest
import torch

import secagg_ref as sr
from fedhip import _lib
from src.aggregation import secure
from src.aggregation.fedavg import FedAvgAggregator, FedAvgError

SEED = 0x5EC0A66C0FFEE123
IDS = [3, 0, 2 ** 33 + 1, 7, 2 ** 64 - 2]  # unsorted, beyond 32 bits, next to the self-key hi
SAMPLES = [10, 30, 20, 25, 15]
NONCE = 2 ** 40 + 5
FRAC = 16
P = 13
STEP = 2.0 ** -FRAC


def _rows():
    rng = np.random.default_rng(11)
    rows = (0.1 * rng.standard_normal((5, P))).astype(np.float32)
    w = np.array(sr.fedavg_weights(SAMPLES), dtype=np.float32)
    rows[0, 1] = np.nan
    rows[1, 2] = 1e30
    rows[2, 3] = -np.inf
    return rows, w


def test_masks_cancel_and_hide_every_word():
    rows, w = _rows()
    out, masked, clipped = sr.secure_fedavg(rows, SAMPLES, IDS, SEED, NONCE, FRAC)
    q, qclip = sr.encode(rows, w, FRAC, (2 ** 31 - 1) // 5)
    plain = (q.astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    got = (masked.astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(got, plain)                      # the masks cancel bit for bit
    assert sr.same_bits(out, sr.decode(plain, FRAC))
    assert not (masked == q).any()                         # no word travels in the clear
    assert clipped.tolist() == [1, 1, 1, 0, 0] == qclip.tolist()
    qm = (2 ** 31 - 1) // 5
    assert q.view(np.int32)[0, 1] == 0 and q.view(np.int32)[1, 2] == qm \
        and q.view(np.int32)[2, 3] == -qm
    # row order does not matter, and another nonce gives other rows with the same sum
    perm = [4, 2, 0, 1, 3]
    out_p, masked_p, _ = sr.secure_fedavg(rows[perm], [SAMPLES[i] for i in perm],
                                          [IDS[i] for i in perm], SEED, NONCE, FRAC)
    assert sr.same_bits(out_p, out) and np.array_equal(masked_p, masked[perm])
    out_n, masked_n, _ = sr.secure_fedavg(rows, SAMPLES, IDS, SEED, NONCE + 1, FRAC)
    assert sr.same_bits(out_n, out) and not (masked_n == masked).any()


def test_rounding_is_to_nearest_even_in_fixed_point():
    x = np.array([[0.5 * STEP, 1.5 * STEP, 2.5 * STEP, -0.5 * STEP, -1.5 * STEP, 0.49 * STEP,
                   -0.0, 1e-45, 3.0, -2.25]], dtype=np.float32)
    q, clipped = sr.encode(x, None, FRAC, 2 ** 31 - 1)
    assert q.view(np.int32)[0].tolist() == [0, 2, 2, 0, -2, 0, 0, 0, 3 << 16, -(9 << 14)]
    assert clipped.tolist() == [0]
    # saturation: qmax itself passes, one step beyond is clipped, on both sides
    qm = 1000
    edge = np.array([[qm * STEP, (qm + 1) * STEP, -qm * STEP, -(qm + 1) * STEP]], np.float32)
    q, clipped = sr.encode(edge, None, FRAC, qm)
    assert q.view(np.int32)[0].tolist() == [qm, qm, -qm, -qm] and clipped.tolist() == [2]
    # the weight is one rounded fp32 multiply
    w = np.array([1 / 3], dtype=np.float32)
    v = np.array([[0.7]], dtype=np.float32)
    want = int(np.rint(np.float64(np.float32(w[0] * v[0, 0])) * 2.0 ** FRAC))
    assert sr.encode(v, w, FRAC, 2 ** 31 - 1)[0].view(np.int32)[0, 0] == want


@pytest.mark.parametrize("self_masks", [False, True])
@pytest.mark.parametrize("gone", [[7], [0, 2 ** 33 + 1], [3, 0, 7, 2 ** 64 - 2]])
def test_recovery_after_dropouts_is_exact(gone, self_masks):
    rows, w = _rows()
    surv = [c for c in IDS if c not in gone]
    out, masked, _ = sr.secure_fedavg(rows, SAMPLES, IDS, SEED, NONCE, FRAC, survivors=surv,
                                      self_masks=self_masks)
    q, _ = sr.encode(rows, w, FRAC, (2 ** 31 - 1) // 5)
    keep = [IDS.index(s) for s in surv]
    plain = (q[keep].astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    n_s = sum(SAMPLES[i] for i in keep)
    want = (np.float32(100 / n_s) * sr.decode(plain, FRAC)).astype(np.float32)
    assert sr.same_bits(out, want)
    # without the server's terms the survivors' sum is noise
    raw, _ = sr.sum_decode(masked[keep], None, None, NONCE, FRAC)
    assert not sr.same_bits(raw, sr.decode(plain, FRAC))
    if self_masks:  # every client's row differs from the pair-masked one
        _, pair_only, _ = sr.secure_fedavg(rows, SAMPLES, IDS, SEED, NONCE, FRAC)
        assert not (pair_only == masked).any()


@pytest.mark.parametrize("defect", [{"flip_signs": True}, {"lane_rot": 1}, {"lo_offset": 1},
                                    {"drop_nonce": True}])
def test_each_masker_defect_changes_the_decoded_sum(defect):
    """A client-side masker with the defect against a correct server (one client dropped, so
    the server removes masks too): the decoded sum must change.  With flip_signs on one side
    only the pair masks between survivors still cancel; the leftovers do not."""
    rows, w = _rows()
    keys, signs = sr.client_terms(SEED, IDS)
    qm = (2 ** 31 - 1) // 5
    good, _ = sr.encode_mask_rows(rows, w, FRAC, qm, keys, signs, NONCE)
    bad, _ = sr.encode_mask_rows(rows, w, FRAC, qm, keys, signs, NONCE, **defect)
    assert not (good == bad).all(axis=1).any()
    surv, gone = IDS[:4], IDS[4:]
    sk, ss = sr.server_terms(SEED, surv, gone)
    want, _ = sr.sum_decode(good[:4], sk, ss, NONCE, FRAC)
    got, _ = sr.sum_decode(bad[:4], sk, ss, NONCE, FRAC)
    assert not sr.same_bits(got, want) and (got != want).sum() >= P - 1
    # the same defect on both sides of one pair still cancels there: only a comparison of the
    # masked rows themselves (as the GPU tests make) sees it
    both, _ = sr.sum_decode(bad, None, None, NONCE, FRAC)
    assert sr.same_bits(both, sr.sum_decode(good, None, None, NONCE, FRAC)[0])


def test_sign_zero_terms_are_skipped_and_empty_term_lists_work():
    rows, w = _rows()
    keys, signs = sr.client_terms(SEED, IDS)
    qm = (2 ** 31 - 1) // 5
    plain, _ = sr.encode_mask_rows(rows, w, FRAC, qm, None, None, NONCE)
    assert np.array_equal(plain, sr.encode(rows, w, FRAC, qm)[0])
    zero, _ = sr.encode_mask_rows(rows, w, FRAC, qm, keys, np.zeros_like(signs), NONCE)
    assert np.array_equal(zero, plain)
    one = signs.copy()
    one[:, 1:] = 0
    got, _ = sr.encode_mask_rows(rows, w, FRAC, qm, keys, one, NONCE)
    want, _ = sr.encode_mask_rows(rows, w, FRAC, qm, keys[:, :1], signs[:, :1], NONCE)
    assert np.array_equal(got, want) and not (got == plain).any()


# ------------------------------------------------------------------ the product's host side
def test_key_derivation_matches_the_reference():
    agg = secure.SecureAggregator(session_seed=SEED, self_masks=True, device="cpu")
    for a, b in ((0, 1), (3, 2 ** 33 + 1), (7, 2 ** 64 - 2), (2 ** 33 + 1, 2 ** 64 - 2)):
        assert agg.pair_key(a, b) == sr.pair_key(SEED, a, b)
    with pytest.raises(ValueError):
        agg.pair_key(5, 5)
    with pytest.raises(ValueError):
        agg.pair_key(6, 5)
    for a in (0, 7, 2 ** 64 - 2):
        assert agg.self_key(a) == sr.self_key(SEED, a)
    assert agg.pair_key(0, 1) != agg.pair_key(1, 2) != agg.self_key(1)
    for self_masks in (False, True):
        agg.self_masks = self_masks
        k, s = agg.client_terms(IDS)
        rk, rs = sr.client_terms(SEED, IDS, self_masks)
        assert np.array_equal(k, rk) and np.array_equal(s, rs) and k.dtype == np.uint64
        k, s = agg.server_terms(IDS[:3], IDS[3:])
        rk, rs = sr.server_terms(SEED, IDS[:3], IDS[3:], self_masks)
        assert np.array_equal(k, rk) and np.array_equal(s, rs)
    k, s = agg.client_terms([9])  # a lone client: its self mask only
    assert k.tolist() == [[sr.self_key(SEED, 9)]] and s.tolist() == [[1]]
    agg.self_masks = False
    k, s = agg.client_terms([9])  # or one slot, switched off
    assert k.shape == (1, 1) and s.tolist() == [[0]]


def test_aggregator_argument_ranges():
    for bad in (-1, 31):
        with pytest.raises(ValueError, match="frac_bits"):
            secure.SecureAggregator(frac_bits=bad, device="cpu")
    agg = secure.create_secure_aggregator(session_seed=1, device="cpu")
    assert type(agg) is secure.SecureAggregator and isinstance(agg, FedAvgAggregator)
    assert agg.frac_bits == 16 and agg.self_masks is False and agg.nonce == 0
    assert [agg.qmax(c) for c in (1, 2, 64)] == [2 ** 31 - 1, (2 ** 31 - 1) // 2,
                                                 (2 ** 31 - 1) // 64]
    assert 64 * agg.qmax(64) < 2 ** 31  # a sum of C saturated codes cannot wrap
    # two aggregators without a seed do not share keys
    a, b = (secure.SecureAggregator(device="cpu") for _ in range(2))
    assert a.session_seed != b.session_seed
    # refused before anything reaches the device
    with pytest.raises(FedAvgError, match="No updates"):
        agg.mask(torch.zeros(0, 8), [])
    with pytest.raises(FedAvgError, match="row_index"):
        agg.mask(torch.zeros(6, 8), [10] * 5, row_index=[0, 1])
    with pytest.raises(FedAvgError, match="no row_index"):
        agg.mask(torch.zeros(6, 8), [10] * 5)
    with pytest.raises(FedAvgError, match="distinct"):
        agg.mask(torch.zeros(2, 8), [10] * 2, client_ids=[4, 4])
    with pytest.raises(FedAvgError, match="at most 65"):
        agg.mask(torch.zeros(66, 8), [10] * 66)
    with pytest.raises(FedAvgError, match="mask call"):
        agg.unmask_sum(torch.zeros(2, 8, dtype=torch.int32), [0, 1])
    assert agg.nonce == 0  # nothing was masked


def test_entry_points_validate_on_the_host():
    """Bad arguments fail with a message before any launch (no device here)."""
    def enc(num_rows=4, P=8, frac_bits=16, qmax=1000, nterms=3):
        return _lib.call("fh_secagg_encode_mask_rows", None, 8, None, None, num_rows, P,
                         frac_bits, qmax, None, None, nterms, 7, None, 8, None, None)
    for kw, msg in (({"frac_bits": 31}, "frac_bits"), ({"frac_bits": -1}, "frac_bits"),
                    ({"qmax": 0}, "qmax"), ({"qmax": -5}, "qmax"), ({"nterms": 65}, "nterms"),
                    ({"nterms": -1}, "nterms"), ({"num_rows": 0}, "num_rows"),
                    ({"P": -1}, "bad sizes"), ({}, "null pointer")):
        with pytest.raises(_lib.FedHipError, match=r"rc=-1\).*" + msg):  # FH_E_INVALID
            enc(**kw)
    assert enc(P=0) == 0 and enc(P=0, nterms=64, frac_bits=30, qmax=2 ** 31 - 1) == 0

    def dec(num_rows=4, P=8, frac_bits=16, nterms=3, out=None, sum_out=None):
        return _lib.call("fh_secagg_sum_decode", None, 8, None, num_rows, P, None, None, nterms,
                         7, frac_bits, out, sum_out, None)
    for kw, msg in (({"frac_bits": 31}, "frac_bits"), ({"nterms": -1}, "nterms"),
                    ({"num_rows": 0}, "num_rows"), ({"P": -1}, "bad sizes"),
                    ({}, "out / sum_out"), ({"out": 64}, "null pointer"),
                    ({"sum_out": 64}, "null pointer")):
        with pytest.raises(_lib.FedHipError, match=r"rc=-1\).*" + msg):
            dec(**kw)
    assert dec(P=0) == 0 and dec(P=0, nterms=2 ** 31 - 1) == 0
