"""Plain numpy references for the robust aggregation kernels (csrc/robust.hip); no GPU.

trimmed_mean     the definition of fh_trimmed_mean_rows (include/fedhip.h): the key transform,
                 a stable argsort of the keys per coordinate, a sequential fp32 sum of the kept
                 values in ascending order, one fp32 division, one quiet NaN for a NaN result.
pairwise_sqdist  fp32 differences, squared and summed in fp64.
krum_select      Krum scoring and selection, written as the O(n^2) loops of the paper.

tests/test_robust_ref_cpu.py pins these against np.sort / np.median and hand-made cases.
"""
import numpy as np

KEY_NAN = np.uint32(0xFFC00000)
QNAN_BITS = np.uint32(0x7FC00000)


def keys(x):
    """uint32 keys whose unsigned order is -Inf < .. < -0 < +0 < .. < +Inf < NaN."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    k = np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), KEY_NAN, k)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k).view(np.float32)


def sorted_rows(rows):
    """rows [C, P] sorted per coordinate by key; every NaN comes back as the one quiet NaN."""
    k = np.sort(keys(rows), axis=0, kind="stable")
    return unkey(k)


def trimmed_mean(rows, trim):
    """[P] fp32.  rows: [C, P] fp32 (already the selected clients)."""
    rows = np.asarray(rows, dtype=np.float32)
    C = rows.shape[0]
    assert 1 <= C and 0 <= 2 * trim < C
    order = np.argsort(keys(rows), axis=0, kind="stable")
    s = unkey(np.take_along_axis(keys(rows), order, axis=0))
    with np.errstate(invalid="ignore", over="ignore"):
        acc = s[trim].copy()
        for k in range(trim + 1, C - trim):
            acc = (acc + s[k]).astype(np.float32)
        out = (acc / np.float32(C - 2 * trim)).astype(np.float32)
    out = out.copy()
    out.view(np.uint32)[np.isnan(out)] = QNAN_BITS
    return out


def median(rows):
    return trimmed_mean(rows, (np.asarray(rows).shape[0] - 1) // 2)


def pairwise_sqdist(rows):
    """[C, C] fp64: sum_j ((double)(fl32(x_a[j] - x_b[j])))^2."""
    rows = np.asarray(rows, dtype=np.float32)
    C = rows.shape[0]
    d = np.zeros((C, C), dtype=np.float64)
    for a in range(C):
        for b in range(a + 1, C):
            diff = (rows[a] - rows[b]).astype(np.float32).astype(np.float64)
            d[a, b] = d[b, a] = np.sum(diff * diff)
    return d


def krum_select(dist, f, m):
    """Brute force: score_i = sum of the n - f - 2 smallest dist[i][k], k != i (ascending);
    the m lowest scores, ties to the lowest index.  Returns (ascending rows, scores)."""
    n = len(dist)
    assert n >= 2 * f + 3
    scores = []
    for i in range(n):
        others = sorted(float(dist[i][k]) for k in range(n) if k != i)
        s = 0.0
        for x in others[:n - f - 2]:
            s += x
        scores.append(s)
    chosen = []
    for _ in range(m):
        best = None
        for i in range(n):
            if i not in chosen and (best is None or scores[i] < scores[best]):
                best = i
        chosen.append(best)
    return sorted(chosen), scores


def uniform_mean(rows, m):
    """The FedAvg kernel's arithmetic with weight fl32(1/m) each: acc = 0; acc += w * x."""
    w = np.float32(1.0 / m)
    acc = np.zeros_like(np.asarray(rows[0], dtype=np.float32))
    for r in rows:
        acc = (acc + (w * np.asarray(r, dtype=np.float32)).astype(np.float32)).astype(np.float32)
    return acc


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
