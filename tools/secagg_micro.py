"""Micro-benchmark of the secure-aggregation kernels (csrc/secagg.hip) against the FedAvg
kernel at the same shape.

    python tools/secagg_micro.py [--iters 20] [--warmup 3] [--out FILE]

Shapes: (32 clients, P = 1,470,890) and (64, 2,777,674), the shapes of tools/robust_micro.py.
Per shape, with HIP events (warm-up, then the median of --iters launches):
  fh_fedavg_weighted_sum      the yardstick: reads C*P floats, writes P
  fh_secagg_encode_mask_rows  every client's row in one launch, C - 1 pair masks each (what
                              SecureAggregator.mask issues): reads C*P floats, writes C*P
                              words, C*(C-1)*ceil(P/4) Philox4x32-10 blocks
  the same with no terms      the encoding alone: the memory-bound floor of that launch
  fh_secagg_sum_decode        nobody dropped (no terms: reads C*P words, writes P floats), and
                              C/8 clients dropped (the survivors' rows, S*D leftover terms)
Rows are random normal draws scaled by 0.1; padded row stride as the engine packs them.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "federated-learning-for-privacy-preserving-image-classification_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from fedhip import ops  # noqa: E402
from src.aggregation.secure import SecureAggregator  # noqa: E402

SHAPES = [(32, 1470890), (64, 2777674)]
FRAC_BITS = 16


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        ts.append((a, b))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ts) * 1e3  # us


def _dev(a, dev):
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    lines = [f"# secagg_micro: {torch.cuda.get_device_name(0)}, median of {a.iters} launches "
             f"after {a.warmup} warm-up; frac_bits {FRAC_BITS}; GB/s = bytes the launch must "
             "move / time; Gblk/s = Philox4x32-10 blocks / time",
             "# clients P | kernel: us | GB/s | Philox blocks, Gblk/s | time / FedAvg's"]
    for C, P in SHAPES:
        stride = (P + 63) // 64 * 64
        g = torch.Generator(device=dev).manual_seed(C)
        rows = (0.1 * torch.randn(C, stride, device=dev, generator=g))[:, :P]
        out = torch.empty(P, device=dev)
        masked = torch.empty(C, stride, dtype=torch.int32, device=dev)[:, :P]
        clipped = torch.zeros(C, dtype=torch.int32, device=dev)
        w32 = torch.full((C,), 1.0 / C, device=dev)
        agg = SecureAggregator(frac_bits=FRAC_BITS, session_seed=1, device=dev)
        ids = list(range(C))
        keys, signs = (_dev(t, dev) for t in agg.client_terms(ids))
        qmax = agg.qmax(C)
        nq = (P + 3) // 4
        D = C // 8
        surv = ids[:C - D]
        sidx = torch.tensor(surv, dtype=torch.int32, device=dev)
        skeys, ssigns = (_dev(t, dev) for t in agg.server_terms(surv, ids[C - D:]))

        def encode(k=keys, s=signs):
            ops.secagg_encode_mask_rows(rows, masked, FRAC_BITS, qmax, k, s, 5, weights=w32,
                                        clipped=clipped)

        t_avg = timed(lambda: ops.fedavg_weighted_sum(rows, w32, out, P=P), a.warmup, a.iters)
        res = [("fedavg_weighted_sum", t_avg, 4.0 * (C + 1) * P, 0)]
        res.append((f"encode_mask_rows, {C - 1} terms / row", timed(encode, a.warmup, a.iters),
                    8.0 * C * P, C * (C - 1) * nq))
        res.append(("encode_mask_rows, no terms", timed(lambda: encode(None, None), a.warmup,
                                                        a.iters), 8.0 * C * P, 0))
        encode()  # leave the masked rows of the full term list behind
        res.append(("sum_decode, nobody dropped",
                    timed(lambda: ops.secagg_sum_decode(masked, FRAC_BITS, nonce=5, out=out),
                          a.warmup, a.iters), 4.0 * (C + 1) * P, 0))
        res.append((f"sum_decode, {D} dropped ({len(surv) * D} terms)",
                    timed(lambda: ops.secagg_sum_decode(masked, FRAC_BITS, skeys, ssigns, 5,
                                                        row_index=sidx, out=out),
                          a.warmup, a.iters), 4.0 * (C - D + 1) * P, len(surv) * D * nq))
        assert int(clipped.sum()) == 0
        for name, us, nbytes, blocks in res:
            rate = f"{blocks / us * 1e-3:7.1f} Gblk/s" if blocks else " " * 14
            lines.append(f"{C:3d} {P:8d} | {name:40s} {us:10.1f} us | {nbytes / us * 1e-3:7.1f} "
                         f"GB/s | {blocks:13d} {rate} | {us / t_avg:7.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
