"""Micro-benchmark of the error-feedback / stochastic-rounding launches (csrc/efcomp.hip), in one
process at one shape, each against the bytes its definition must move:

  (a) fh_ef_fold                         reads x, resid, base; writes resid        (3C+1)*P floats
  (b) fh_ef_topk_finish                  reads resid, keep, base; writes x, resid  3C*P floats + C*P bytes + P floats
  (c) fh_ef_quant_finish                 reads c, resid, base; writes x, resid     (4C+1)*P floats
  (d) fh_squant_rows, v = x - base       min/max pass + apply pass, out only       (3C+2)*P floats
  (e) fh_squant_rows, v = resid          min/max pass + apply pass, out + resid    (4C+1)*P floats

    python tools/efcomp_micro.py [--clients 32] [--launches 20] [--repeats 15] [--warmup 3]
                                 [--bits 4] [--out FILE]

Shape: the 32-client CIFAR10CNN round — the model's own parameter segments (P = 1,470,890), row
stride padded to 64 floats as the engine packs it, one broadcast base row (the global model).
fh_squant_rows is two launches behind one entry point; (d) and (e) time the pair.  A timing is
HIP events around --launches back-to-back calls; the variants alternate inside every repeat, and
the table gives the median and the min..max spread over --repeats.  For scale, the last lines
time the whole compress_rows chains (fold + the existing select / quantiser + finish).
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
from fedhip.net import ParamLayout  # noqa: E402
from src.shared import models_pytorch as hm  # noqa: E402

HBM_PEAK_TBS = 6.3


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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("efcomp_micro: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda")
    C = a.clients
    layout = ParamLayout.from_module(hm.ModelFactory.create_model("cifar10_cnn"))
    P = layout.P
    plan = fc.SegmentPlan(layout.seg_offsets(), dev)
    stride = (P + 63) // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(C)

    def rows(scale=1.0):
        return torch.randn(C, stride, device=dev, generator=gen).mul_(scale)[:, :P]

    glob = torch.randn(P, device=dev, generator=gen)
    base = glob.view(1, -1).expand(C, -1)
    x = rows(0.05).add_(glob)
    resid, resid2, c, out = rows(0.02), rows(0.0), rows(0.05), rows(0.0)
    keep = (torch.rand(C, stride, device=dev, generator=gen) < 0.1).to(torch.uint8)[:, :P]
    ids = torch.arange(C, dtype=torch.int64, device=dev)
    key = 0x5DEECE66D
    cfg_topk = fc.CompressionConfig("topk", sparsity_ratio=0.9, error_feedback=True)
    cfg_sq = fc.CompressionConfig("quantization", bits=a.bits, error_feedback=True,
                                  stochastic=True)

    variants = [
        ("a", "ef_fold", (3 * C + 1) * P * 4,
         lambda: fc.ef_fold(plan, x, resid, C, base=base)),
        ("b", "ef_topk_finish", 3 * C * P * 4 + C * P + P * 4,
         lambda: fc.ef_topk_finish(plan, keep, resid, out, C, base=base)),
        ("c", "ef_quant_finish", (4 * C + 1) * P * 4,
         lambda: fc.ef_quant_finish(plan, c, resid, out, C, base=base)),
        ("d", f"squant_rows {a.bits}b (x - base)", (3 * C + 2) * P * 4,
         lambda: fc.squant_rows(plan, x, C, a.bits, True, key, ids, base=base, out=out)),
        ("e", f"squant_rows {a.bits}b (resid)", (4 * C + 1) * P * 4,
         lambda: fc.squant_rows(plan, None, C, a.bits, True, key, ids, base=base, resid=c,
                                out=out, resid_out=resid2)),
    ]
    chains = [
        ("compress_rows top-k 0.9 + EF", lambda: fc.compress_rows(plan, cfg_topk, out, C,
                                                                  base=base, resid=resid)),
        (f"compress_rows squant {a.bits}b + EF", lambda: fc.compress_rows(
            plan, cfg_sq, out, C, base=base, resid=resid, key=key, row_ids=ids)),
    ]
    everything = [fn for _, _, _, fn in variants] + [fn for _, fn in chains]
    for _ in range(a.warmup):
        for fn in everything:
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k, _, _, _ in variants}
    tc = {n: [] for n, _ in chains}
    for _ in range(a.repeats):
        for k, _, _, fn in variants:
            ts[k].append(timed(fn, a.launches))
        for n, fn in chains:
            out.copy_(x)
            tc[n].append(timed(fn, max(1, a.launches // 4)))
    lines = [f"# efcomp_micro: {torch.cuda.get_device_name(0)}, C={C} P={P} (row stride {stride}, "
             f"{plan.nseg} segments, {plan.nchunks} chunks per row); per-call time = HIP events "
             f"around {a.launches} calls, median [min..max] of {a.repeats} alternating repeats "
             f"after {a.warmup} warm-up; share of the {HBM_PEAK_TBS} TB/s HBM peak from the bytes "
             f"each call must move",
             "# call | us median [min..max] | MB moved | GB/s | share of HBM peak"]
    for k, name, nbytes, _ in variants:
        med, lo, hi = statistics.median(ts[k]), min(ts[k]), max(ts[k])
        mb = nbytes / 1e6
        gbs = mb / med * 1e3
        lines.append(f"({k}) {name:28s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us | {mb:7.1f} MB "
                     f"| {gbs:7.0f} GB/s | {100 * gbs / 1e3 / HBM_PEAK_TBS:5.1f} %")
    for n, _ in chains:
        med, lo, hi = statistics.median(tc[n]), min(tc[n]), max(tc[n])
        lines.append(f"# chain {n:32s} | {med:8.1f} [{lo:8.1f} .. {hi:8.1f}] us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
