"""Generate tests/golden/golden_mobilenet.json by running the REFERENCE LightweightMobileNet
and LocalTrainer.

Run only in the development container (the reference is not present on the GPU box), with
the reference repository first on PYTHONPATH:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python <repo>/tests/golden/make_golden_mobilenet.py

Inputs are NOT stored: they are regenerated from the seeds recorded here.  Per width
multiplier (0.5 and 1.0) the fixture holds sha256 + a few samples of every initial parameter,
of the eval-mode logits on a seeded batch, and of the parameters, BatchNorm statistics and
metrics after a short seeded run (2 batches of 8; SGD and Adam).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))

_tv = types.ModuleType("torchvision")
_tv.datasets = types.ModuleType("torchvision.datasets")
_tv.transforms = types.ModuleType("torchvision.transforms")
sys.modules.setdefault("torchvision", _tv)
sys.modules.setdefault("torchvision.datasets", _tv.datasets)
sys.modules.setdefault("torchvision.transforms", _tv.transforms)

from src.shared import models_pytorch as ref_models  # noqa: E402
from src.shared.training import LocalTrainer  # noqa: E402

torch.set_num_threads(8)
INIT_SEED, DATA_SEED, N, BS = 4, 5, 16, 8
RUNS = [("sgd", 0.01), ("adam", 1e-3)]


def digest(t):
    a = np.ascontiguousarray(t.detach().cpu().reshape(-1).numpy().astype(np.float32))
    idx = np.linspace(0, a.size - 1, min(a.size, 4)).astype(np.int64)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "numel": int(a.size),
            "idx": idx.tolist(), "val": [float(v) for v in a[idx]]}


def make_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 32, 32, generator=g), torch.randint(0, 10, (n,), generator=g)


def main():
    out = {}
    x, y = make_batch(N, DATA_SEED)
    for width in (0.5, 1.0):
        torch.manual_seed(INIT_SEED)
        model = ref_models.LightweightMobileNet(num_classes=10, width_multiplier=width)
        entry = {"width_multiplier": width, "init_seed": INIT_SEED, "data_seed": DATA_SEED,
                 "n": N, "bs": BS, "names": [n for n, _ in model.named_parameters()],
                 "init": {n: digest(p) for n, p in model.named_parameters()}}
        model.eval()
        with torch.no_grad():
            entry["eval_logits"] = digest(model(x))
        init = {k: v.clone() for k, v in model.state_dict().items()}
        entry["runs"] = {}
        for opt, lr in RUNS:
            model.load_state_dict(init)
            dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=BS,
                                             shuffle=False)
            tr = LocalTrainer(model, device=torch.device("cpu"))
            m = tr.train_local_model(dl, epochs=1, learning_rate=lr, optimizer_type=opt,
                                     save_checkpoints=False)
            sd = model.state_dict()
            entry["runs"][opt] = {
                "lr": lr, "epochs": 1,
                "metrics": {"loss": m.loss, "accuracy": m.accuracy,
                            "epochs_completed": m.epochs_completed,
                            "samples_processed": m.samples_processed},
                "params": {n: digest(p) for n, p in model.named_parameters()},
                "buffers": {k: digest(v.float()) for k, v in sd.items() if "running" in k}}
        out[f"width_{width}"] = entry
    with open(os.path.join(OUT, "golden_mobilenet.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
