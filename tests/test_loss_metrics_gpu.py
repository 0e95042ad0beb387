"""fh_ce_fwd_bwd and fh_eval_metrics against plain fp64 / integer references
(tests/small_ref.py, pinned to torch's CPU operators by test_small_ref_cpu.py).

* loss and dlogits: the kernel's maximum error against fp64 is at most 4 x the error of
  torch's own fp32 CPU F.cross_entropy (+ autograd) on the same inputs, with a floor of 2e-6
  relative (the floor test_classifier_gpu.py uses).  No figure comes from a HIP launch.
* correct / per-class counts: exact against the CPU argmax (first maximal index) and bincount,
  on rows built to tie across lanes, across the 64-wide stride and at index 0 / K-1.
* both ce_kernel paths (16 lanes per image for K <= 16 and <= 256 images; a wave per image
  otherwise) and the switches at K = 16 / 17 and 256 / 257 images; a client with no images;
  the accumulators over several launches and the per-client reset flag.
* every output is pre-filled with a sentinel and sits in a wider buffer: rows past a client's
  count and the padding between clients must come back bit for bit.
Targets stay inside [0, K) everywhere."""
import pytest
import torch
import torch.nn.functional as F

import small_ref as sr
from fedhip import ops
from fedhip._lib import FedHipError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KS = [1, 2, 10, 16, 17, 63, 64, 65, 100, 200]
FLOOR = 2e-6


def _inputs(nc, B, K, seed, ties=False):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(nc, B, K, generator=g) * 3.0
    tg = torch.randint(0, K, (nc, B), generator=g)
    if ties:  # client 0 is always full: its first rows become the tie rows
        rows, tt = sr.tie_rows(K)
        n = min(len(rows), B)
        lg[0, :n], tg[0, :n] = rows[:n], tt[:n]
    return lg, tg


def _dev_view(t):
    """Device copy of t [nc, ...] as a [nc, n] view into a wider buffer (client stride > n)."""
    nc = t.shape[0]
    flat = t.reshape(nc, -1)
    fill = sr.SENTINEL if t.is_floating_point() else 0
    buf, view = sr.padded(nc, flat.shape[1], t.dtype, DEV, fill=fill, pad=3)
    view.copy_(flat)
    return view


def _ce(lg, tg, counts, acc=None, reset=None, with_loss=True):
    """One fh_ce_fwd_bwd launch.  Returns (dlogits [nc, B, K], loss_out [nc]) on the CPU after
    checking that nothing outside the counted rows of dlogits / loss_out was written."""
    nc, B, K = lg.shape
    dbuf, dl = sr.padded(nc, B * K, torch.float32, DEV)
    before = dbuf.clone()
    loss = torch.full((nc + 2,), sr.SENTINEL, device=DEV)
    cd = torch.tensor(counts, dtype=torch.int32, device=DEV)
    a = acc if acc is not None else (None, None, None)
    ops.ce_fwd_bwd(_dev_view(lg), _dev_view(tg), dl, nc, B, K,
                   loss_out=loss if with_loss else None, acc_loss=a[0], acc_correct=a[1],
                   acc_seen=a[2], reset=reset, counts=cd)
    torch.cuda.synchronize()
    assert sr.untouched_outside(dbuf, before, [n * K for n in counts])
    assert sr.same_bits(loss[nc:], torch.full((2,), sr.SENTINEL))
    if not with_loss:
        assert sr.same_bits(loss, torch.full((nc + 2,), sr.SENTINEL))
    return dl.cpu().contiguous().view(nc, B, K), loss[:nc].cpu()


def _check_client(lg, tg, n, dl, loss):
    """The fp64 bound of the module docstring for one client's n images."""
    x32 = lg[:n].clone().requires_grad_(True)
    l32 = F.cross_entropy(x32, tg[:n])
    l32.backward()
    loss64, dl64 = sr.ce_rows(lg[:n], tg[:n])
    ref = loss64.mean().item()
    assert torch.isfinite(dl[:n]).all() and torch.isfinite(loss)
    ls = max(1.0, abs(ref))
    e_cpu, e_hip = abs(l32.item() - ref) / ls, abs(loss.item() - ref) / ls
    print(f"loss: hip {e_hip:.3e} cpu32 {e_cpu:.3e}")
    assert e_hip <= max(4 * e_cpu, FLOOR), (e_hip, e_cpu)
    scale = dl64.abs().max().item() + 1e-300
    e_cpu = (x32.grad.double() - dl64).abs().max().item() / scale
    e_hip = (dl[:n].double() - dl64).abs().max().item() / scale
    print(f"dlogits: hip {e_hip:.3e} cpu32 {e_cpu:.3e}")
    assert e_hip <= max(4 * e_cpu, FLOOR), (e_hip, e_cpu)


def _correct(lg, tg, n):
    return int((lg[:n].argmax(dim=1) == tg[:n]).sum())


def _acc(nc, loss0=0.0, corr0=0, seen0=0):
    return (torch.full((nc,), loss0, dtype=torch.float64, device=DEV),
            torch.full((nc,), corr0, dtype=torch.int64, device=DEV),
            torch.full((nc,), seen0, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("K,B", [(K, B) for K in KS for B in (1, 5, 32)] + [(10, 256), (10, 257)])
def test_ce_matches_fp64(K, B):
    nc = 3
    counts = sr.ragged_counts(nc, B, K + B)
    lg, tg = _inputs(nc, B, K, 7 * K + B)
    acc = _acc(nc)
    dl, loss = _ce(lg, tg, counts, acc=acc)
    for z, n in enumerate(counts):
        _check_client(lg[z], tg[z], n, dl[z], loss[z])
        assert int(acc[1][z]) == _correct(lg[z], tg[z], n)
    assert acc[2].tolist() == counts
    assert sr.same_bits(acc[0], loss.double())
    # no accumulators, no loss_out: the same dlogits
    dl2, _ = _ce(lg, tg, counts, with_loss=False)
    assert sr.same_bits(dl, dl2)


@pytest.mark.parametrize("K", KS)
def test_ce_tie_rows_first_index(K):
    rows, tt = sr.tie_rows(K)
    B, nc = len(rows), 3
    counts = [B, 1, max(1, B - 2)]
    lg, tg = _inputs(nc, B, K, 31 + K, ties=True)
    lg[1], tg[1] = rows.flip(0), tt.flip(0)   # the count-1 client sees the last pattern
    lg[2], tg[2] = rows, tt
    acc = _acc(nc)
    dl, loss = _ce(lg, tg, counts, acc=acc)
    for z, n in enumerate(counts):
        assert int(acc[1][z]) == _correct(lg[z], tg[z], n), z
        assert int(acc[1][z]) == int((sr.first_argmax(lg[z, :n]) == tg[z, :n]).sum())
        _check_client(lg[z], tg[z], n, dl[z], loss[z])


@pytest.mark.parametrize("K", [10, 100])
def test_ce_shifted_dominant_logits(K):
    """Logits shifted by +-80 with one logit 30 above the rest: exp() of the raw values
    overflows / underflows fp32, the shifted form must not."""
    nc, B = 3, 8
    counts = [8, 1, 5]
    g = torch.Generator().manual_seed(K)
    lg = torch.randn(nc, B, K, generator=g)
    dom = torch.randint(0, K, (nc, B), generator=g)
    lg.scatter_add_(2, dom.unsqueeze(-1), torch.full((nc, B, 1), 30.0))
    lg[0] += 80.0
    lg[1] -= 80.0
    lg[2, ::2] += 80.0
    lg[2, 1::2] -= 80.0
    tg = dom.clone()
    tg[:, ::2] = (dom[:, ::2] + 1) % K  # every client's first image misses the dominant class
    acc = _acc(nc)
    dl, loss = _ce(lg, tg, counts, acc=acc)
    for z, n in enumerate(counts):
        _check_client(lg[z], tg[z], n, dl[z], loss[z])
        assert int(acc[1][z]) == _correct(lg[z], tg[z], n)
        assert loss[z].item() > 1.0  # the missed images carry a loss of about 30 each


@pytest.mark.parametrize("K", [10, 100])
@pytest.mark.parametrize("empty", [0, 1])
def test_ce_client_without_images(K, empty):
    nc, B = 2, 5
    counts = [5, 5]
    counts[empty] = 0
    lg, tg = _inputs(nc, B, K, K + empty)
    for rs in (None, torch.tensor([1, 1], dtype=torch.int32, device=DEV)):
        acc = _acc(nc, 1.5, 7, 9)
        dl, loss = _ce(lg, tg, counts, acc=acc, reset=rs)  # checks dlogits rows untouched
        assert sr.same_bits(loss[empty], torch.tensor(0.0))
        base = (0.0, 0, 0) if rs is not None else (1.5, 7, 9)
        assert acc[0][empty].item() == base[0]
        assert int(acc[1][empty]) == base[1] and int(acc[2][empty]) == base[2]
        z = 1 - empty
        _check_client(lg[z], tg[z], 5, dl[z], loss[z])
        assert acc[0][z].item() == base[0] + float(loss[z])
        assert int(acc[1][z]) == base[1] + _correct(lg[z], tg[z], 5)
        assert int(acc[2][z]) == base[2] + 5


@pytest.mark.parametrize("K", [10, 100])
def test_ce_accumulators_and_reset(K):
    nc, B = 4, 32
    acc = _acc(nc)
    want = [[0.0, 0, 0] for _ in range(nc)]
    resets = [None, None, [1, 0, 1, 0]]
    for step, rs in enumerate(resets):
        counts = sr.ragged_counts(nc, B, 11 * step + K)
        lg, tg = _inputs(nc, B, K, 100 * step + K)
        rd = None if rs is None else torch.tensor(rs, dtype=torch.int32, device=DEV)
        _, loss = _ce(lg, tg, counts, acc=acc, reset=rd)
        for z, n in enumerate(counts):
            if rs is not None and rs[z]:
                want[z] = [0.0, 0, 0]
            want[z][0] = want[z][0] + float(loss[z])  # fp64 sum of the fp32 batch losses
            want[z][1] += _correct(lg[z], tg[z], n)
            want[z][2] += n
    assert acc[0].tolist() == [w[0] for w in want]
    assert acc[1].tolist() == [w[1] for w in want]
    assert acc[2].tolist() == [w[2] for w in want]


# ------------------------------------------------------------------ fh_eval_metrics
def _eval(lg, tg, counts, loss_sum, correct, cc, ct):
    nc, B, K = lg.shape
    cd = torch.tensor(counts, dtype=torch.int32, device=DEV)
    ops.eval_metrics(_dev_view(lg), _dev_view(tg), nc, B, K, counts=cd, loss_sum=loss_sum,
                     correct=correct, class_correct=cc, class_total=ct)
    torch.cuda.synchronize()


def _eval_buffers(nc, K):
    """loss_sum, correct, class_correct, class_total: each with two guard entries behind the
    payload, the integer ones starting from non-zero totals."""
    ls = torch.zeros(nc + 2, dtype=torch.float64, device=DEV)
    ls[nc:] = sr.SENTINEL
    co = torch.full((nc + 2,), 3, dtype=torch.int64, device=DEV)
    cc = torch.full((K + 2,), 5, dtype=torch.int64, device=DEV)
    ct = torch.full((K + 2,), 11, dtype=torch.int64, device=DEV)
    return ls, co, cc, ct


@pytest.mark.parametrize("K,B", [(K, B) for K in KS for B in (1, 32, 77)])
def test_eval_metrics_match_reference(K, B):
    nc = 3
    ls, co, cc, ct = _eval_buffers(nc, K)
    ref_loss, cpu_loss = [0.0] * nc, [0.0] * nc
    ref_corr = [0] * nc
    ref_cc, ref_ct = torch.zeros(K, dtype=torch.int64), torch.zeros(K, dtype=torch.int64)
    for step in range(3):
        counts = sr.ragged_counts(nc, B, 5 * step + K + B)
        lg, tg = _inputs(nc, B, K, 1000 * step + 3 * K + B, ties=step == 0)
        _eval(lg, tg, counts, ls, co, cc, ct)
        for z, n in enumerate(counts):
            x, t = lg[z, :n], tg[z, :n]
            ref_loss[z] += sr.ce_rows(x, t)[0].sum().item()
            cpu_loss[z] += float(F.cross_entropy(x, t, reduction="sum"))
            pred = x.argmax(dim=1)
            ref_corr[z] += int((pred == t).sum())
            ref_ct += torch.bincount(t, minlength=K)
            ref_cc += torch.bincount(t[pred == t], minlength=K)
            c2, t2 = sr.class_counts(sr.first_argmax(x), t, K)
            assert torch.equal(c2, torch.bincount(t[pred == t], minlength=K))
            assert torch.equal(t2, torch.bincount(t, minlength=K))
    assert (co[:nc].cpu() - 3).tolist() == ref_corr
    assert torch.equal(cc[:K].cpu() - 5, ref_cc) and torch.equal(ct[:K].cpu() - 11, ref_ct)
    assert co[nc:].tolist() == [3, 3] and cc[K:].tolist() == [5, 5] and ct[K:].tolist() == [11, 11]
    assert sr.same_bits(ls[nc:], torch.full((2,), sr.SENTINEL, dtype=torch.float64))
    for z in range(nc):
        s = max(1.0, abs(ref_loss[z]))
        e_hip, e_cpu = abs(ls[z].item() - ref_loss[z]) / s, abs(cpu_loss[z] - ref_loss[z]) / s
        print(f"loss_sum: hip {e_hip:.3e} cpu32 {e_cpu:.3e}")
        assert e_hip <= max(4 * e_cpu, FLOOR), (z, e_hip, e_cpu)


def test_eval_metrics_nullable_outputs():
    nc, B, K = 3, 32, 10
    counts = sr.ragged_counts(nc, B, 2)
    lg, tg = _inputs(nc, B, K, 77, ties=True)
    full = _eval_buffers(nc, K)
    _eval(lg, tg, counts, *full)
    for drop in ("loss_sum", "correct", "classes"):
        ls, co, cc, ct = _eval_buffers(nc, K)
        _eval(lg, tg, counts, None if drop == "loss_sum" else ls,
              None if drop == "correct" else co, None if drop == "classes" else cc,
              None if drop == "classes" else ct)
        fresh = _eval_buffers(nc, K)
        for name, got, want, init in zip(("loss_sum", "correct", "classes", "classes"),
                                         (ls, co, cc, ct), full, fresh):
            assert sr.same_bits(got, init if name == drop else want), (drop, name)
    # one class counter without the other is refused before any launch
    ls, co, cc, ct = _eval_buffers(nc, K)
    for a, b in ((cc, None), (None, ct)):
        with pytest.raises(FedHipError, match="class_correct and class_total go together"):
            _eval(lg, tg, counts, ls, co, a, b)
    for got, init in zip((ls, co, cc, ct), _eval_buffers(nc, K)):
        assert sr.same_bits(got, init)


@pytest.mark.parametrize("K", KS)
def test_eval_metrics_agree_with_ce_and_repeat(K):
    nc, B = 3, 32
    counts = sr.ragged_counts(nc, B, K)
    lg, tg = _inputs(nc, B, K, 5 + K, ties=True)
    acc = _acc(nc)
    _ce(lg, tg, counts, acc=acc)
    runs = []
    for _ in range(2):
        ls = torch.zeros(nc, dtype=torch.float64, device=DEV)
        co = torch.zeros(nc, dtype=torch.int64, device=DEV)
        _eval(lg, tg, counts, ls, co, None, None)
        runs.append((ls, co))
    assert torch.equal(runs[0][1], acc[1])
    assert sr.same_bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
