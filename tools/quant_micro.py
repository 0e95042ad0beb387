"""Micro-benchmark of the packed quantised-update launches (csrc/quantpack.hip) in one process,
each against the bytes its definition must move, and against the dense sum they replace:

  (a) fh_quant_pack_rows      reads one code per byte, writes cw bits per code     C*P + C*P*cw/8
  (b) fh_quant_unpack_rows    reads the codes and base, writes C rows      C*P*cw/8 + 4*P + 4*C*P
  (c) fh_quant_fedavg         reads the codes and base, writes one row     C*P*cw/8 + 8*P
  (d) fh_fedavg_weighted_sum  over the same clients' dense rows (the sum (c) replaces)
                                                                           4*C*P + 4*P

    python tools/quant_micro.py [--clients 32] [--P 2800804] [--launches 20] [--repeats 15]
                                [--warmup 3] [--out profiles/quantpack/quant_micro.txt]

Shapes: 32 clients at P = 1,470,890 (CIFAR10CNN's own parameter segments) and at --P (the same
segments and one more, see layouts()), 8 and 4 bits, symmetric; row stride padded to 64 floats as
the engine packs it, one broadcast base row (the global model).  A timing is HIP events around
--launches back-to-back calls; the variants alternate inside every repeat, and the table gives
the median and the min..max spread over --repeats.  Before timing, (b) is checked bit for bit
against fh_quantize_rows' own output and (c) against (d) over those rows.
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

from fedhip import compress as fc  # noqa: E402
from fedhip import ops  # noqa: E402
from fedhip import quantpack as fq  # noqa: E402
from fedhip.net import ParamLayout  # noqa: E402
from src.shared import models_pytorch as hm  # noqa: E402

HBM_PEAK_TBS = 6.3


def layouts(P2):
    """name -> segment offsets.  The second layout keeps CIFAR10CNN's segments and adds one
    dense layer's worth of weights to reach P = P2."""
    seg = ParamLayout.from_module(hm.ModelFactory.create_model("cifar10_cnn")).seg_offsets()
    out = {"cifar10_cnn": seg}
    if P2 > seg[-1]:
        out[f"P={P2}"] = seg + [P2]
    return out


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per call


def bench(name, seg, bits, a, dev, lines):
    C = a.clients
    P = seg[-1]
    plan = fc.SegmentPlan(seg, dev)
    qp = fq.QuantPlan(plan, bits)
    stride = (P + 63) // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(C)
    glob = torch.randn(P, device=dev, generator=gen)
    base = glob.view(1, -1).expand(C, -1)
    x = torch.randn(C, stride, device=dev, generator=gen).mul_(0.05)[:, :P].add_(glob)
    dense = torch.zeros(C, stride, device=dev)[:, :P]
    rebuilt = torch.zeros(C, stride, device=dev)[:, :P]
    codes = torch.zeros(C, stride, dtype=torch.uint8, device=dev)[:, :P]
    upd = qp.empty(C)
    fc.quantize_rows(plan, x, C, bits, True, base=base, out=dense, codes=codes,
                     scale_out=upd.scale, zp_out=upd.zp)
    w = (torch.rand(C, device=dev, generator=gen) / C).float()
    out_q, out_d = torch.empty(P, device=dev), torch.empty(P, device=dev)
    nb = C * qp.B  # code bytes of all clients (the 16-byte padding of each segment included)

    variants = [
        ("a", "quant_pack_rows", C * P + nb,
         lambda: fq.quant_pack_rows(upd, x, codes, C, base=base)),
        ("b", "quant_unpack_rows", nb + 4 * P + 4 * C * P,
         lambda: fq.quant_unpack_rows(upd, rebuilt, C, base=base)),
        ("c", "quant_fedavg", nb + 8 * P,
         lambda: fq.quant_fedavg(upd, w, glob, out_q)),
        ("d", "fedavg_weighted_sum (dense)", 4 * C * P + 4 * P,
         lambda: ops.fedavg_weighted_sum(dense, w, out_d, P=P)),
    ]
    for _ in range(a.warmup):
        for _, _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    same = torch.equal(out_q.view(torch.int32), out_d.view(torch.int32)) and \
        torch.equal(rebuilt.view(torch.int32), dense.view(torch.int32)) and \
        not bool(fq.quant_validate(upd).any())
    if not same:
        sys.exit(f"quant_micro: {name} {bits} bits: the results from the packed codes differ "
                 "from the dense ones; no timing of wrong results")
    ts = {k: [] for k, _, _, _ in variants}
    for _ in range(a.repeats):
        for k, _, _, fn in variants:
            ts[k].append(timed(fn, a.launches))
    lines.append(f"## {name}: P={P} ({plan.nseg} segments, {plan.nchunks} chunks), {bits} bits "
                 f"(cw={qp.cw}): B={qp.B} code bytes per client, C={C}; (b) and (c) bit-identical "
                 f"to the dense path")
    for k, label, nbytes, _ in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        mb = nbytes / 1e6
        gbs = mb / med * 1e3
        lines.append(f"({k}) {label:28s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | {mb:7.1f} MB "
                     f"| {gbs:7.0f} GB/s | {100 * gbs / 1e3 / HBM_PEAK_TBS:5.1f} %")
    sc, sd = statistics.median(ts["c"]), statistics.median(ts["d"])
    lines.append(f"    sum from codes / dense sum: time {sc / sd:.2f}x, bytes "
                 f"{(nb + 8 * P) / (4 * C * P + 4 * P):.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=32)
    ap.add_argument("--P", type=int, default=2_800_804)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quantpack",
                                                  "quant_micro.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quant_micro: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    lines = [f"# quant_micro: {torch.cuda.get_device_name(0)}; per-call time = HIP events around "
             f"{a.launches} calls, median [min..max] of {a.repeats} alternating repeats after "
             f"{a.warmup} warm-up; share of the {HBM_PEAK_TBS} TB/s HBM peak from the bytes each "
             f"call must move",
             "# call | us median [min..max] | MB moved | GB/s | share of HBM peak"]
    for name, seg in layouts(a.P).items():
        for bits in (8, 4):
            bench(name, seg, bits, a, dev, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
