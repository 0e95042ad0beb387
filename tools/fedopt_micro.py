"""Micro-benchmark of the server-optimizer step (csrc/fedopt.hip) against the FedAvg kernel it
extends, in one process at one shape:

  (a) fh_fedavg_weighted_sum alone                     (C+1)*P floats
  (b) (a) followed by a single-row fh_server_opt_step  (C+1)*P + (1+3+3)*P floats, two launches
  (c) the fused rows-mode fh_server_opt_step           (C+3)*P + 3*P floats, one launch

    python tools/fedopt_micro.py [--clients 32] [--P 1470890] [--rule 3] [--launches 50]
                                 [--repeats 15] [--warmup 5] [--out FILE]

Default shape: the 32-client CIFAR10CNN round (P = 1,470,890, row stride padded to 64 floats as
the engine packs it).  A timing is HIP events around --launches back-to-back launches; the
three variants alternate inside every repeat, and the table gives the median and the min..max
spread over --repeats.  (b) and (c) compute the same bits (tests/test_fedopt_gpu.py); FedAvgM
(--rule 0) has no second moment and moves 2*P floats less each way.
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
RULE_NAMES = ["FedAvgM", "FedAdagrad", "FedAdam", "FedYogi"]


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--P", type=int, default=1470890)
    ap.add_argument("--rule", type=int, default=ops.SOPT_YOGI)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    C, P, rule = a.clients, a.P, a.rule
    stride = (P + 63) // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(C)
    glob = torch.randn(P, device=dev, generator=gen)
    rows = torch.randn(C, stride, device=dev, generator=gen)[:, :P]  # padded stride, as packed
    rows.mul_(0.05).add_(glob)
    w32 = torch.full((C,), 1.0 / C, device=dev)
    agg = torch.empty(P, device=dev)
    sc = dict(server_lr=1e-3, beta1=0.9, beta2=0.99, tau=1e-3)
    # each variant owns its global / m / v, so every launch sees a state like a round's
    state = {k: (glob.clone(), torch.zeros(P, device=dev), torch.full((P,), 1e-6, device=dev))
             for k in "bc"}

    def run_a():
        ops.fedavg_weighted_sum(rows, w32, agg, P=P)

    def run_b():
        ops.fedavg_weighted_sum(rows, w32, agg, P=P)
        g, m, v = state["b"]
        ops.server_opt_step(agg.view(1, -1), g, m, v, rule, P=P, **sc)

    def run_c():
        g, m, v = state["c"]
        ops.server_opt_step(rows, g, m, v, rule, weights_f32=w32, P=P, **sc)

    nv = 0 if rule == ops.SOPT_MOMENTUM else 1
    floats = {"a": (C + 1) * P, "b": (C + 1) * P + (5 + 2 * nv) * P, "c": (C + 4 + 2 * nv) * P}
    variants = [("a", "fedavg_weighted_sum", run_a),
                ("b", "fedavg + single-row step", run_b),
                ("c", "fused rows-mode step", run_c)]
    for _ in range(a.warmup):
        for _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _ in variants}
    for _ in range(a.repeats):
        for k, _, fn in variants:
            ts[k].append(timed(fn, a.launches))
    same = all(torch.equal(x, y) for x, y in zip(state["b"], state["c"]))
    lines = [f"# fedopt_micro: {torch.cuda.get_device_name(0)}, {RULE_NAMES[rule]}, C={C} P={P} "
             f"(row stride {stride}); per-call time = HIP events around {a.launches} launches, "
             f"median [min..max] of {a.repeats} alternating repeats after {a.warmup} warm-up; "
             f"share of the {HBM_PEAK_TBS} TB/s HBM peak from the floats each variant must move",
             "# variant | us median [min..max] | MB moved | TB/s | share of HBM peak"]
    for k, name, _ in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        mb = 4.0 * floats[k] / 1e6
        tbs = mb / med
        lines.append(f"({k}) {name:26s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | {mb:7.1f} MB "
                     f"| {tbs:5.2f} TB/s | {100 * tbs / HBM_PEAK_TBS:5.1f} %")
    mb_, mc_ = statistics.median(ts["b"]), statistics.median(ts["c"])
    lines.append(f"# (b) - (c) = {mb_ - mc_:.1f} us; spread of (a) = "
                 f"{max(ts['a']) - min(ts['a']):.1f} us; (b) and (c) end with the same bits: {same}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
