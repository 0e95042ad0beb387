"""tests/small_ref.py (the plain references the loss / metric / pooling / gather / statistics
GPU tests compare the HIP kernels with) pinned to torch's own CPU operators, so that a
reference cannot be wrong in the same way as a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_ref as sr

KS = [1, 2, 10, 16, 17, 63, 64, 65, 100, 200]


@pytest.mark.parametrize("K", KS)
def test_ce_rows_match_torch(K):
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(9, K, generator=g) * 3).double().requires_grad_(True)
    t = torch.randint(0, K, (9,), generator=g)
    loss, dl = sr.ce_rows(x.detach(), t)
    ref = F.cross_entropy(x, t, reduction="none")
    torch.testing.assert_close(loss, ref.detach(), rtol=1e-13, atol=1e-13)
    F.cross_entropy(x, t).backward()
    torch.testing.assert_close(dl, x.grad, rtol=1e-13, atol=1e-15)
    # the shifted, dominated rows of the stability case
    xs = x.detach().clone() + 80.0
    xs[:, 0] += 30.0
    loss, _ = sr.ce_rows(xs, t)
    torch.testing.assert_close(loss, F.cross_entropy(xs, t, reduction="none"), rtol=1e-12,
                               atol=1e-13)


@pytest.mark.parametrize("K", KS)
def test_first_argmax_and_tie_rows(K):
    rows, tg = sr.tie_rows(K)
    assert rows.shape[1] == K and int(tg.min()) >= 0 and int(tg.max()) < K
    assert torch.equal(rows, rows.round()) and float(rows.max()) == 3.0
    pred = sr.first_argmax(rows)
    assert torch.equal(pred, rows.argmax(dim=1))
    # the first maximal index really is the first: nothing before it reaches the maximum
    for r, p in zip(rows, pred.tolist()):
        assert float(r[p]) == 3.0 and (r[:p] < 3.0).all()
    if K >= 2:  # every pattern has a row with a repeated maximum
        assert ((rows == 3.0).sum(dim=1) >= 2).any()
        # targets cover the first index, a later maximal index (and a non-maximal one)
        assert (tg == pred).any() and ((tg != pred) & (rows[torch.arange(len(tg)), tg] == 3.0)).any()
    if K >= 3:
        assert (rows[torch.arange(len(tg)), tg] < 3.0).any()
    g = torch.Generator().manual_seed(K)
    x = torch.randint(-3, 4, (50, K), generator=g).float()
    assert torch.equal(sr.first_argmax(x), x.argmax(dim=1))


def test_class_counts_match_bincount():
    g = torch.Generator().manual_seed(5)
    K = 17
    pred = torch.randint(0, K, (200,), generator=g)
    t = torch.randint(0, K, (200,), generator=g)
    t[::3] = pred[::3]
    c, n = sr.class_counts(pred, t, K)
    assert torch.equal(n, torch.bincount(t, minlength=K))
    assert torch.equal(c, torch.bincount(t[pred == t], minlength=K))


@pytest.mark.parametrize("HW", [1, 3, 16, 49, 63, 64, 65, 196])
def test_avgpool_matches_torch(HW):
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(3, 5, HW, generator=g).double().requires_grad_(True)
    y = F.adaptive_avg_pool2d(x.view(3, 5, HW, 1), 1).view(3, 5)
    torch.testing.assert_close(sr.avgpool_fwd(x.detach(), HW), y.detach(), rtol=1e-14, atol=1e-15)
    dy = torch.randn(3, 5, generator=g).double()
    y.backward(dy)
    got = sr.avgpool_bwd(dy, HW)
    assert got.shape == x.shape
    torch.testing.assert_close(got, x.grad, rtol=1e-14, atol=0)


def test_ulp32():
    v = np.array([1.0, -1.0, 1.5, 2.0 ** -130, 0.0, 3.0e38], dtype=np.float32)
    u = sr.ulp32(v)
    assert u[0] == 2.0 ** -23 and u[1] == 2.0 ** -23 and u[2] == 2.0 ** -23
    assert u[3] == 2.0 ** -149 and u[4] == 2.0 ** -149
    t = torch.from_numpy(v[:3])
    nxt = torch.nextafter(t.abs(), torch.full_like(t, float("inf")))
    assert np.array_equal((nxt - t.abs()).double().numpy(), u[:3])


def test_gather_matches_index_select():
    bits = sr.awkward_bits(40 * 7, 3).view(40, 7)
    labels = torch.arange(40, dtype=torch.int64) * 3 - 7
    idx = torch.tensor([39, 0, 0, 17, 39, 5, 4, 3], dtype=torch.int64)
    x, y = sr.gather(bits, labels, idx)
    assert torch.equal(x, bits.index_select(0, idx))
    assert torch.equal(y, labels.index_select(0, idx))
    f = bits.view(torch.float32)
    assert torch.isnan(f).any() and (f == 0).any()
    assert ((f != 0) & (f.abs() < 2.0 ** -126)).any()  # denormals


def test_update_stats_matches_torch():
    g = torch.Generator().manual_seed(9)
    row = torch.randn(700, generator=g)
    offs = [0, 1, 64, 64, 320, 577, 700]
    row[63] = float("nan")
    row[320] = float("inf")
    row[699] = -float("inf")
    row[100] = -7.5
    row[1:63] = torch.tensor(1e-40)
    am, bad = sr.update_stats(row, offs)
    for t in range(len(offs) - 1):
        seg = row[offs[t]:offs[t + 1]]
        assert int(bad[t]) == int((~torch.isfinite(seg)).any())
        if not int(bad[t]):
            ref = seg.abs().amax() if seg.numel() else torch.tensor(0.0)
            assert sr.same_bits(am[t], ref)
    assert bad.tolist() == [0, 1, 0, 0, 1, 1]
    assert float(am[3]) == 7.5 and float(am[2]) == 0.0


def test_buffer_helpers():
    assert sr.ragged_counts(3, 8, 1)[:2] == [8, 1] and sr.ragged_counts(1, 8, 1) == [8]
    buf, view = sr.padded(2, 6, torch.float32, "cpu")
    assert view.stride(0) == 11 and view.shape == (2, 6)
    before = buf.clone()
    view[0, :4] = 1.0
    assert sr.untouched_outside(buf, before, [4, 0])
    assert not sr.untouched_outside(buf, before, [3, 0])
    buf[1, 8] = 0.0
    assert not sr.untouched_outside(buf, before, [4, 0])
    assert sr.same_bits(torch.tensor([float("nan")]), torch.tensor([float("nan")]))
    assert not sr.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
