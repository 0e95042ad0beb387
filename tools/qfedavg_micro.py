"""Micro-benchmark of the q-FedAvg call (csrc/qfedavg.hip) against the route the same rule takes
through the kernels that were there before it, in one process, one shape after the other:

  (a) fh_dpfa_row_sqnorm, a host read of the C norms, fh_fednova_rows STEP with tau = 1/den
                                             the two-pass route: (2C+2)*P floats and a round trip
  (b) the same two launches without the read (tau fixed ahead): the route's kernels alone
  (c) fh_qfedavg_rows STEP                   (C+1)*P floats in the main pass, 3*P in the apply
                                             pass, den kept on the device

    python tools/qfedavg_micro.py [--clients 32] [--P 1470890 2800000] [--launches 50]
                                  [--repeats 15] [--warmup 5] [--out FILE]

Default shapes: the 32-client CIFAR10CNN round (P = 1,470,890) and a 2.8 M-parameter model, row
stride padded to 64 floats as the engine packs it.  A timing is HIP events around --launches
back-to-back calls; the variants alternate inside every repeat, and the table gives the median
and the min..max spread over --repeats.  The share of the HBM peak is taken against the floor of
the rule, (C+1)*P floats read once, for every variant.  The last line of a shape reports the
largest difference between the results of (a) and (c) beside the largest step either takes (the
two routes round 1/den differently); it is a sanity figure, the tests hold the bits.
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
    rows = torch.randn(C, stride, device=dev, generator=gen)[:, :P]  # padded stride, as packed
    rows.mul_(0.05).add_(glob)
    losses = [0.2 + (37 * k) % 23 / 10.0 for k in range(C)]  # uneven losses, 0.2 .. 2.4
    a, b = ops.qfedavg_coefficients([1.0 / C] * C, losses, 1.0, 100.0)
    a32 = torch.tensor(a, dtype=torch.float32, device=dev)
    b64 = torch.tensor(b, dtype=torch.float64, device=dev)
    out_a, out_b, out_c = (torch.empty(P, device=dev) for _ in range(3))
    sq = torch.empty(C, dtype=torch.float64, device=dev)
    state = torch.empty(ops.QFA_STATE_DOUBLES, dtype=torch.float64, device=dev)
    tau_fixed = [1.0]

    def run_a():
        ops.dpfa_row_sqnorm(rows, glob, P=P, out=sq)
        host = sq.tolist()  # the round trip
        den = 0.0
        for ak, bk, sk in zip(a, b, host):
            den = den + (bk * sk + ak)
        tau_fixed[0] = 1.0 / den
        ops.fednova_rows(rows, a32, glob, out_a, tau_fixed[0], ops.NOVA_STEP, P=P)

    def run_b():
        ops.dpfa_row_sqnorm(rows, glob, P=P, out=sq)
        ops.fednova_rows(rows, a32, glob, out_b, tau_fixed[0], ops.NOVA_STEP, P=P)

    def run_c():
        ops.qfedavg_rows(rows, a32, b64, glob, out_c, ops.QFA_STEP, P=P, sqdist=sq, state=state)

    floor = (C + 1) * P
    variants = [("a", "row_sqnorm + read + fednova", run_a),
                ("b", "row_sqnorm + fednova", run_b), ("c", "qfedavg STEP", run_c)]
    for _ in range(args.warmup):
        for _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _ in variants}
    for _ in range(args.repeats):
        for k, _, fn in variants:
            ts[k].append(timed(fn, args.launches))
    err = (out_a.double() - out_c.double()).abs().max().item()
    scale = (out_c.double() - glob.double()).abs().max().item()
    lines = [f"# C={C} P={P} (row stride {stride}); floor (C+1)*P*4 = {4.0 * floor / 1e6:.1f} MB = "
             f"{4.0 * floor / 1e6 / HBM_PEAK_TBS:.1f} us at {HBM_PEAK_TBS} TB/s",
             "# variant | us median [min..max] | floor bytes / time | share of HBM peak"]
    for k, name, _ in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        tbs = 4.0 * floor / 1e6 / med
        lines.append(f"({k}) {name:28s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | "
                     f"{tbs:5.2f} TB/s | {100 * tbs / HBM_PEAK_TBS:5.1f} %")
    ma, mb_, mc_ = (statistics.median(ts[k]) for k in "abc")
    lines.append(f"# (a) / (c) = {ma / mc_:.2f}, (b) / (c) = {mb_ / mc_:.2f}; spread of (b) = "
                 f"{max(ts['b']) - min(ts['b']):.1f} us, of (c) = "
                 f"{max(ts['c']) - min(ts['c']):.1f} us; max |(a) - (c)| = {err:.3e} at a largest "
                 f"step of {scale:.3e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--P", type=int, nargs="+", default=[1470890, 2800000])
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("qfedavg_micro: no HIP device; there is nothing to measure on a CPU")
    dev = torch.device("cuda")
    lines = [f"# qfedavg_micro: {torch.cuda.get_device_name(0)}; per-call time = HIP events around "
             f"{args.launches} calls, median [min..max] of {args.repeats} alternating repeats "
             f"after {args.warmup} warm-up; share of the {HBM_PEAK_TBS} TB/s HBM peak from the "
             f"(C+1)*P floats the rule must read"]
    for P in args.P:
        lines += one_shape(args.clients, P, args, dev)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
