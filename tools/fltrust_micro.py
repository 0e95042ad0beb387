"""Micro-benchmark of the FLTrust call (csrc/fltrust.hip), in one process, one shape after the
other:

  (y) fh_qfedavg_rows PARTIAL   the yardstick, NOT the code under test: an existing kernel that
                                reads the same C rows and g once with one fp64 accumulator per
                                client, (C+1)*P floats read (and P written)
  (s) fh_fltrust_rows SCORE     the stats pass, (C+2)*P floats read (33..64 clients: (C+4)*P, g
                                and the root row are read by both launches), two fp64
                                accumulators per client, then the one-workgroup coefficient launch
  (t) fh_fltrust_rows STEP      (s), then fh_center_iter's DELTA pass: (C+1)*P more floats read
                                (from HBM or from the last-level cache), P written

    python tools/fltrust_micro.py [--clients 8 16 32 64] [--P 1470890 2800000] [--launches 50]
                                  [--repeats 15] [--warmup 5] [--out FILE]

Default shapes: the CIFAR10CNN round (P = 1,470,890) and a 2.8 M-parameter model at four client
counts, one per register-slot count of the stats kernel's widths, row stride padded to 64 floats
as the engine packs it.  A timing is HIP events around --launches back-to-back calls; the variants
alternate inside every repeat, and the table gives the median and the min..max spread over
--repeats.  Bytes per second are the bytes each variant must move (the counts above) over its own
time, beside their share of the HBM peak; for (t) a figure above what (s) reaches says the second
pass found rows in the cache.
"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "federated-learning-for-privacy-preserving-image-classification_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from fedhip import ops  # noqa: E402

HBM_PEAK_TBS = 6.3


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per call


def one_shape(C, P, args, dev):
    stride = (P + 63) // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(C)
    glob = torch.randn(P, device=dev, generator=gen)
    step = torch.randn(P, device=dev, generator=gen) * 0.05
    root = glob + step
    rows = torch.randn(C, stride, device=dev, generator=gen)[:, :P]  # padded stride, as packed
    rows.mul_(0.03).add_(glob).add_(step)        # every client near the root's direction ...
    rows[C // 2].copy_(glob - step)              # ... but one that points away
    a32 = torch.full((C,), 1.0 / C, device=dev)
    b64 = torch.zeros(C, dtype=torch.float64, device=dev)
    out_y, out_t = torch.empty(P, device=dev), torch.empty(P, device=dev)
    sq = torch.empty(C, dtype=torch.float64, device=dev)
    qstate = torch.empty(ops.QFA_STATE_DOUBLES, dtype=torch.float64, device=dev)
    coef = torch.empty(C, device=dev)
    trust = torch.empty(C, dtype=torch.float64, device=dev)
    stats = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
    state = torch.empty(ops.FLT_STATE_DOUBLES, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.fltrust_workspace(C, P), dtype=torch.uint8, device=dev)

    def run_y():
        ops.qfedavg_rows(rows, a32, b64, glob, out_y, ops.QFA_PARTIAL, P=P, sqdist=sq,
                         state=qstate)

    def run_s():
        ops.fltrust_rows(rows, root, glob, None, ops.FLT_SCORE, P=P, coef=coef, trust=trust,
                         stats=stats, state=state, workspace=ws)

    def run_t():
        ops.fltrust_rows(rows, root, glob, out_t, ops.FLT_STEP, P=P, coef=coef, trust=trust,
                         stats=stats, state=state, workspace=ws)

    score_floats = (C + 2 + (2 if C > 32 else 0)) * P
    variants = [("y", "qfedavg PARTIAL (yardstick)", run_y, (C + 2) * P),
                ("s", "fltrust SCORE", run_s, score_floats),
                ("t", "fltrust STEP", run_t, score_floats + (C + 2) * P)]
    for _ in range(args.warmup):
        for _, _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _, _ in variants}
    for _ in range(args.repeats):
        for k, _, fn, _ in variants:
            ts[k].append(timed(fn, args.launches))
    trusted = int(state.tolist()[ops.FLT_TRUSTED])
    lines = [f"# C={C} P={P} (row stride {stride}); the rows are {4.0 * C * P / 1e6:.1f} MB; "
             f"{trusted} of {C} clients trusted",
             "# variant | us median [min..max] | MB moved | bytes / time | share of HBM peak"]
    for k, name, _, floats in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        mb = 4.0 * floats / 1e6
        tbs = mb / med
        lines.append(f"({k}) {name:28s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | {mb:7.1f} | "
                     f"{tbs:5.2f} TB/s | {100 * tbs / HBM_PEAK_TBS:5.1f} %")
    my, ms, mt = (statistics.median(ts[k]) for k in "yst")
    lines.append(f"# (s) / (y) = {ms / my:.2f}, (t) - (s) = {mt - ms:.1f} us for the second pass "
                 f"({4.0 * (C + 2) * P / 1e6 / max(mt - ms, 1e-9):.2f} TB/s); spread of (y) = "
                 f"{max(ts['y']) - min(ts['y']):.1f} us, of (s) = "
                 f"{max(ts['s']) - min(ts['s']):.1f} us, of (t) = "
                 f"{max(ts['t']) - min(ts['t']):.1f} us")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--P", type=int, nargs="+", default=[1470890, 2800000])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fltrust_micro: no HIP device; there is nothing to measure on a CPU")
    dev = torch.device("cuda")
    lines = [f"# fltrust_micro: {torch.cuda.get_device_name(0)}; per-call time = HIP events around "
             f"{args.launches} calls, median [min..max] of {args.repeats} alternating repeats "
             f"after {args.warmup} warm-up; share of the {HBM_PEAK_TBS} TB/s HBM peak from the "
             f"bytes each variant must move"]
    for P in args.P:
        for C in args.clients:
            lines += one_shape(C, P, args, dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
