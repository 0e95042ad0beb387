"""tests/mobilenet_ref.py (the CPU restatement of the reference LightweightMobileNet the GPU
tests compare against) reproduces the reference's recorded results bit for bit, and the
product's parameter container draws the same initial values under the same seed.

Fixture: tests/golden/golden_mobilenet.json (make_golden_mobilenet.py, run on the
reference)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import mobilenet_ref as mr
from src.shared import models_pytorch as hm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "golden_mobilenet.json")))


def check(t, g, what):
    a = np.ascontiguousarray(t.detach().cpu().reshape(-1).numpy().astype(np.float32))
    assert a.size == g["numel"], what
    np.testing.assert_array_equal(a[g["idx"]], np.asarray(g["val"], np.float32), err_msg=what)
    assert hashlib.sha256(a.tobytes()).hexdigest() == g["sha256"], what


def batch(g):
    gen = torch.Generator().manual_seed(g["data_seed"])
    return (torch.randn(g["n"], 3, 32, 32, generator=gen),
            torch.randint(0, 10, (g["n"],), generator=gen))


@pytest.mark.parametrize("key", sorted(GOLD))
def test_helper_reproduces_reference(key):
    g = GOLD[key]
    torch.set_num_threads(8)
    net = mr.init_model(g["init_seed"], g["width_multiplier"])
    assert [n for n, _ in net.named_parameters()] == g["names"]
    for n, p in net.named_parameters():
        check(p, g["init"][n], f"init {n}")
    x, y = batch(g)
    check(mr.eval_logits(net, x), g["eval_logits"], "eval logits")
    batches = [(x[i:i + g["bs"]], y[i:i + g["bs"]]) for i in range(0, g["n"], g["bs"])]
    for opt, run in g["runs"].items():
        r = net.clone()
        m = mr.train_epochs(r, batches, run["epochs"], run["lr"], opt)
        for k, v in run["metrics"].items():
            assert m[k] == v, (opt, k, m[k], v)
        for n, p in r.named_parameters():
            check(p, run["params"][n], f"{opt} {n}")
        for n, d in run["buffers"].items():
            check(r.buffers[n].float(), d, f"{opt} {n}")
        assert len(m["masks"]) == len(batches) and len(m["masks"][0]) == 13


@pytest.mark.parametrize("key", sorted(GOLD))
def test_product_container_initial_parameters(key):
    g = GOLD[key]
    torch.manual_seed(g["init_seed"])
    model = hm.LightweightMobileNet(num_classes=10, width_multiplier=g["width_multiplier"])
    assert [n for n, _ in model.named_parameters()] == g["names"]
    for n, p in model.named_parameters():
        check(p, g["init"][n], n)
    ref = mr.init_model(g["init_seed"], g["width_multiplier"])
    assert [k for k in ref.buffers] == [k for k, _ in model.named_buffers()]


def test_fp64_mask_replay_matches_own_masks():
    """Replaying a run's own ReLU masks reproduces that run (x * mask == relu(x) for its own
    mask), in fp64 to rounding."""
    net = mr.init_model(1, 0.5).double()
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(4, 3, 32, 32, generator=g).double(), torch.randint(0, 10, (4,), generator=g)
    a, b = net.clone(), net.clone()
    la, _, _, used = mr.train_step(a, mr.make_optimizer(a, "sgd", 0.01), x, y)
    lb, _, _, _ = mr.train_step(b, mr.make_optimizer(b, "sgd", 0.01), x, y, relus=used)
    assert la == lb
    assert torch.equal(mr.param_vector(a), mr.param_vector(b))
