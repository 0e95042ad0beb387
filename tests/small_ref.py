"""Plain fp64 / integer references of the small kernels — TEST HELPER (not a test).

The loss, metric, pooling, gather and update-statistics kernels (fh_ce_fwd_bwd,
fh_eval_metrics, fh_avgpool_fwd / _bwd, fh_gather_batch, fh_update_stats) are compared with
these restatements, written from the definitions with elementary tensor arithmetic only:

    cross-entropy   loss_i = logsumexp(x_i) - x_i[t_i];  dlogits = (softmax - onehot) / n
    prediction      the FIRST index holding the row maximum (torch.max / argmax rule)
    average pool    y = sum over the map / HW;  dx = dy / HW on every pixel of the plane
    gather          x[b] = data[idx[b]], y[b] = labels[idx[b]]
    update stats    per segment: any non-finite value; max |v| over the finite ones (0 if none)

tests/test_small_ref_cpu.py pins every helper to torch's own CPU operator, so a helper cannot
be wrong in the way a kernel is.  The helpers that build test inputs (tie rows, ragged counts,
sentinel-padded buffers) live here too, shared by the GPU test files.
"""
from __future__ import annotations

import numpy as np
import torch

SENTINEL = -12345.678  # fp32 fill of every output buffer: a kernel never produces it


# ------------------------------------------------------------------ cross-entropy / argmax
def ce_rows(logits, targets):
    """Per-image CE losses [n] and the gradient of their MEAN w.r.t. the logits [n, K], fp64."""
    x = logits.double()
    n, K = x.shape
    m = x.max(dim=1, keepdim=True).values
    lse = m + (x - m).exp().sum(dim=1, keepdim=True).log()
    rows = torch.arange(n)
    loss = lse[:, 0] - x[rows, targets]
    onehot = torch.zeros(n, K, dtype=torch.float64)
    onehot[rows, targets] = 1.0
    return loss, ((x - lse).exp() - onehot) / max(n, 1)


def first_argmax(logits):
    """Index of the first maximal entry of every row (comparisons only)."""
    K = logits.shape[1]
    m = logits.max(dim=1, keepdim=True).values
    k = torch.arange(K).expand_as(logits)
    return torch.where(logits == m, k, torch.full_like(k, K)).min(dim=1).values


def class_counts(pred, targets, K):
    """(correct, total) per class, int64 [K], by a plain loop."""
    correct, total = [0] * K, [0] * K
    for p, t in zip(pred.tolist(), targets.tolist()):
        total[t] += 1
        correct[t] += int(p == t)
    return torch.tensor(correct, dtype=torch.int64), torch.tensor(total, dtype=torch.int64)


def tie_rows(K):
    """Integer-valued logit rows [n, K] whose maximum (3) is repeated, the rest in [-5, 0],
    and targets [n]: for every tie pattern the target is the first maximal index, the last
    one, and (when there is one) an index that is not maximal.  Patterns: index 0 and K-1;
    neighbouring indices (different lanes of one wave); 64 apart (same lane, next stride
    step); a lower lane holding the LATER index (5 and 67: first index 5 sits in the higher
    lane); four maxima 64 apart."""
    pats = [[0]]
    if K >= 2:
        pats.append([0, K - 1])
    if K >= 3:
        pats.append([1, 2, min(5, K - 1)] if K > 3 else [1, 2])
    if K >= 65:
        pats.append([0, 64])
    if K >= 68:
        pats += [[3, 67], [5, 67]]
    if K >= 100:
        pats.append([35, 99])
    if K >= 198:
        pats += [[5, 69, 133, 197], [70, 134, 7 + 128]]
    g = torch.Generator().manual_seed(1000 + K)
    rows, tg = [], []
    for p in pats:
        p = sorted(set(p))
        others = [k for k in range(K) if k not in p]
        for t in [p[0], p[-1]] + ([others[len(others) // 2]] if others else []):
            r = -torch.randint(0, 6, (K,), generator=g).float()
            r[p] = 3.0
            rows.append(r)
            tg.append(t)
    return torch.stack(rows), torch.tensor(tg, dtype=torch.int64)


# ------------------------------------------------------------------ global average pool
def avgpool_fwd(x, HW):
    """x [..., HW] -> fp64 means [...]."""
    return x.double().sum(dim=-1) / HW


def avgpool_bwd(dy, HW):
    """dy [...] -> fp64 [..., HW]: every pixel of a plane gets dy / HW."""
    return (dy.double() / HW).unsqueeze(-1).repeat(*([1] * dy.dim()), HW)


def ulp32(v):
    """Spacing of fp32 at |v| (numpy array in, fp64 out)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------ gather
def gather(data, labels, idx):
    """data [N, E] (any dtype, moved as bits), labels [N], idx [n] -> (x [n, E], y [n])."""
    x = torch.empty(len(idx), data.shape[1], dtype=data.dtype)
    y = torch.empty(len(idx), dtype=labels.dtype)
    for b, s in enumerate(idx.tolist()):
        x[b] = data[s]
        y[b] = labels[s]
    return x, y


def awkward_bits(n, seed):
    """n int32 bit patterns of fp32 values a copy must not alter: uniformly random words
    (NaNs with payloads, infinities, denormals among them) with -0.0, quiet / signalling NaN
    payloads and the smallest / largest denormals planted at the front."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64)
    special = [-2 ** 31, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC12345 - 2 ** 32,
               0xFF800001 - 2 ** 32, 0x00000001, 0x007FFFFF, 0x80000001 - 2 ** 32,
               0x7F800000, 0xFF800000 - 2 ** 32]
    k = min(n, len(special))
    bits[:k] = torch.tensor(special[:k], dtype=torch.int64)
    return bits.to(torch.int32)


# ------------------------------------------------------------------ update statistics
def update_stats(row, offsets):
    """row: 1-D fp32 tensor; offsets: segment boundaries.  (absmax fp32 [nseg], flag [nseg]):
    flag = a NaN / Inf in the segment, absmax = max |v| over its finite values (0 if none)."""
    v = row.numpy()
    am = np.zeros(len(offsets) - 1, dtype=np.float32)
    bad = np.zeros(len(offsets) - 1, dtype=np.int32)
    for t in range(len(offsets) - 1):
        for j in range(offsets[t], offsets[t + 1]):
            e = v[j]
            if e != e or e == np.inf or e == -np.inf:
                bad[t] = 1
            elif abs(e) > am[t]:
                am[t] = abs(e)
    return torch.from_numpy(am), torch.from_numpy(bad)


# ------------------------------------------------------------------ buffers and counts
def ragged_counts(nc, B, seed):
    """A full client, a client with one image, the rest in [1, B]."""
    g = torch.Generator().manual_seed(seed)
    c = [B, 1] + [int(v) for v in torch.randint(1, B + 1, (max(nc - 2, 0),), generator=g)]
    return c[:nc]


def padded(nc, n, dtype, device, fill=SENTINEL, pad=5):
    """(buffer [nc, n + pad] filled with `fill`, its [nc, n] view): the view's client stride
    is larger than its payload, so writes past a row show up in the buffer's padding."""
    buf = torch.full((nc, n + pad), fill, dtype=dtype, device=device)
    return buf, buf[:, :n]


def bits(t):
    """Bit pattern of a tensor (fp32 -> int32, fp64 -> int64; integers as they are)."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def untouched_outside(buf, before, lens):
    """True when buf [nc, W] equals `before` bit for bit outside the first lens[z] entries of
    every row."""
    a, b = bits(buf.cpu()).clone(), bits(before.cpu()).clone()
    for z, n in enumerate(lens):
        a[z, :n] = 0
        b[z, :n] = 0
    return torch.equal(a, b)
