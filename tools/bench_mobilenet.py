"""Round-level throughput of LightweightMobileNet (width 0.5) on one GPU.

    python tools/bench_mobilenet.py [--steps 3] [--warmup 1] [--out FILE]

One RankRound round of 32 Dirichlet(0.5) clients (bench.py's KT data recipe: 50k synthetic
CIFAR-shaped uint8 images, the on-device train transform), SGD, timed as bench.py times its
rounds (graph / program replay), reported as client-images/s.  Then one instrumented round
(every launch eager, HIP events around each: ops.LaunchProbe) gives the share of the summed
launch time spent in the depthwise, pointwise / stem and BatchNorm launches — the ranking the
follow-up fusions need.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "federated-learning-for-privacy-preserving-image-classification_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from fedhip import ops  # noqa: E402
from fedhip.round import RankRound  # noqa: E402
from src.shared import models_pytorch as hm  # noqa: E402

# launches the probe does not tag by itself, timed here under their own name
UNTAGGED = ["bn_fwd_train", "bn_bwd", "avgpool_fwd", "avgpool_bwd", "gather_u8", "gather_batch",
            "sgd_step", "sgd_step_slabs", "ce_fwd_bwd"]


def tag_untagged():
    for name in UNTAGGED:
        fn = getattr(ops, name)

        def wrapped(*a, _fn=fn, _name=name, **kw):
            ev = ops.PROBE.begin(_name)
            out = _fn(*a, **kw)
            ops.PROBE.end(ev, 0.0)
            return out
        setattr(ops, name, wrapped)


def group_of(tag):
    if tag.startswith("dwconv_"):
        return "depthwise"
    if tag.startswith("conv_"):
        return "pointwise" if "k1s1" in tag else "stem"
    if tag.startswith("bn_"):
        return "batchnorm"
    return "other"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg = dict(bench.CONFIGS["KT"])
    _, train = bench.build_clients(cfg, 1)
    torch.manual_seed(0)
    model = hm.ModelFactory.get_lightweight_model().to(dev)
    tf = ops.DataTransform.cifar10()
    rr = RankRound(model, train, list(range(len(train))), epochs=1, device=dev, transform=tf)
    data, lab, offs = bench.make_rank_data(cfg, train, rr.slots, dev, 0, raw=True)
    gen = torch.Generator().manual_seed(7)
    for w in range(a.warmup):
        rr.run(data, lab, offs, "sgd", 0.01, seed=w, generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(a.steps):
        rr.run(data, lab, offs, "sgd", 0.01, seed=100 + s, generator=gen)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / max(a.steps, 1)
    # instrumented round
    tag_untagged()
    ops.PROBE.reset()
    ops.PROBE.tag, ops.PROBE.enabled = "*", True
    rr.run(data, lab, offs, "sgd", 0.01, seed=999, generator=gen, serialize_lanes=True)
    ops.PROBE.enabled = False
    groups = {}
    for tag, (n, ms, _) in ops.PROBE.by_tag().items():
        g = groups.setdefault(group_of(tag), [0, 0.0])
        g[0] += n
        g[1] += ms
    total = sum(v[1] for v in groups.values()) or 1.0
    out = {"metric": "client-images/sec", "model": "lightweight_mobilenet(width 0.5)",
           "clients": len(train), "images_per_round": int(sum(train)),
           "value": round(sum(train) / dt, 1), "round_ms": round(dt * 1e3, 2),
           "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "instrumented_launch_ms": round(total, 2),
           "share": {k: {"launches": v[0], "ms": round(v[1], 2),
                         "fraction": round(v[1] / total, 4)} for k, v in sorted(groups.items())}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
