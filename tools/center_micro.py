"""Micro-benchmark of the fused centre-iteration kernel (csrc/center.hip) against the unfused
iteration the older kernels already allow, in one process, one shape after the other:

  (a) fh_dpfa_row_sqnorm + fh_fedavg_weighted_sum   the unfused iteration: the distances to the
                                                    current centre, then the weighted sum;
                                                    (2C+2)*P floats, two passes over the rows
  (b) fh_center_iter MEAN                           (C+1)*P floats: the new centre and the
                                                    distances to it, one pass over the rows
  (c) fh_center_iter DELTA                          (C+2)*P floats, in place on the centre

    python tools/center_micro.py [--clients 32] [--P 1470890 2800000] [--launches 50]
                                 [--repeats 15] [--warmup 5] [--out FILE]

Default shapes: the 32-client CIFAR10CNN round (P = 1,470,890) and a 2.8 M-parameter model, row
stride padded to 64 floats as the engine packs it.  A timing is HIP events around --launches
back-to-back calls; the variants alternate inside every repeat, and the table gives the median
and the min..max spread over --repeats.  The byte model says (a) / (b) = (2C+2)/(C+1) = 2 in
floats moved ((a) reads the rows twice and the centre once and writes the sum; (b) reads the rows
once and writes the centre); the run prints the measured ratio beside it and checks that (a) and
(b) end with the same `out` bits.  Every variant includes its small second launch (the partials'
sum), so the comparison is call for call.
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


def one_shape(C, P, a, dev):
    stride = (P + 63) // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(C)
    glob = torch.randn(P, device=dev, generator=gen)
    rows = torch.randn(C, stride, device=dev, generator=gen)[:, :P]  # padded stride, as packed
    rows.mul_(0.05).add_(glob)
    c32 = torch.full((C,), 1.0 / C, dtype=torch.float32, device=dev)
    out_a, out_b = torch.empty(P, device=dev), torch.empty(P, device=dev)
    out_c = glob.clone()
    sq_a, sq_b, sq_c = (torch.empty(C, dtype=torch.float64, device=dev) for _ in range(3))

    def run_a():
        ops.dpfa_row_sqnorm(rows, glob, P=P, out=sq_a)
        ops.fedavg_weighted_sum(rows, c32, out_a, P=P)

    def run_b():
        ops.center_iter(rows, c32, out_b, ops.CENTER_MEAN, P=P, sqdist=sq_b)

    def run_c():  # in place; the centre converges to the mean, the traffic stays the same
        ops.center_iter(rows, c32, out_c, ops.CENTER_DELTA, center=out_c, P=P, sqdist=sq_c)

    floats = {"a": (2 * C + 2) * P, "b": (C + 1) * P, "c": (C + 2) * P}
    variants = [("a", "row_sqnorm + fedavg_sum", run_a), ("b", "center_iter MEAN", run_b),
                ("c", "center_iter DELTA", run_c)]
    for _ in range(a.warmup):
        for _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _ in variants}
    for _ in range(a.repeats):
        for k, _, fn in variants:
            ts[k].append(timed(fn, a.launches))
    same = torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
    lines = [f"# C={C} P={P} (row stride {stride})",
             "# variant | us median [min..max] | MB moved | TB/s | share of HBM peak"]
    for k, name, _ in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        mb = 4.0 * floats[k] / 1e6
        tbs = mb / med
        lines.append(f"({k}) {name:26s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | {mb:7.1f} MB "
                     f"| {tbs:5.2f} TB/s | {100 * tbs / HBM_PEAK_TBS:5.1f} %")
    ma, mb_, mc_ = (statistics.median(ts[k]) for k in "abc")
    clear = min(ts["a"]) > max(ts["b"])
    lines.append(f"# (a) / (b) = {ma / mb_:.3f}, float ratio (2C+2)/(C+1) = "
                 f"{(2 * C + 2) / (C + 1):.3f}; "
                 f"(a) - (b) = {ma - mb_:.1f} us, spread of (a) = "
                 f"{max(ts['a']) - min(ts['a']):.1f} us, of (b) = "
                 f"{max(ts['b']) - min(ts['b']):.1f} us; min (a) above max (b): {clear}; "
                 f"(c) / (b) = {mc_ / mb_:.3f}; (a) and (b) end with the same out bits: {same}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--P", type=int, nargs="+", default=[1470890, 2800000])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("center_micro: no HIP device; there is nothing to measure on a CPU")
    dev = torch.device("cuda")
    lines = [f"# center_micro: {torch.cuda.get_device_name(0)}; per-call time = HIP events around "
             f"{a.launches} calls, median [min..max] of {a.repeats} alternating repeats after "
             f"{a.warmup} warm-up; share of the {HBM_PEAK_TBS} TB/s HBM peak from the floats each "
             f"variant must move"]
    for P in a.P:
        lines += one_shape(a.clients, P, a, dev)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
