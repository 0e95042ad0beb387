"""CPU restatement of the reference LightweightMobileNet — TEST HELPER (not a test).

Reference: src/shared/models_pytorch.py MobileNetBlock / LightweightMobileNet and the
LocalTrainer hot path (src/shared/training.py: _train_epoch, _create_optimizer).  The model
is functional code over a parameter dict (``named_parameters()`` order and names) and a
buffer dict (BatchNorm running statistics), in fp32 or fp64:

    conv1 3x3 -> bn1 -> ReLU
    6 x [depthwise 3x3(s), groups = C -> bn1 -> ReLU -> pointwise 1x1 -> bn2 -> ReLU]
    mean over the map -> classifier

with F.conv2d(groups=C), F.batch_norm, ReLU, mean and F.linear — the ATen CPU ops the
reference's modules call, so an fp32 run reproduces the reference bit for bit
(tests/golden/golden_mobilenet.json pins that).  ReLU masks can be replayed (the fp64 "same
decisions" run of the GPU tests) and the masks a run used are returned.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

BLOCKS = [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2)]
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def make_divisible(v, divisor=8):
    nv = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if nv < 0.9 * v:
        nv += divisor
    return nv


def config(width_multiplier=1.0):
    """(stem channels, [(cin, cout, stride)] of the six blocks)."""
    c = make_divisible(32 * width_multiplier)
    stem, blocks = c, []
    for co, s in BLOCKS:
        co = make_divisible(co * width_multiplier)
        blocks.append((c, co, s))
        c = co
    return stem, blocks


class RefNet:
    """Parameters + buffers of one model instance.  ``named_parameters()`` makes it usable
    where the GPU tests' criteria (check_params) take an oracle module."""

    def __init__(self, params, buffers, width_multiplier, num_classes):
        self.params, self.buffers = params, buffers
        self.width_multiplier, self.num_classes = width_multiplier, num_classes
        self.blocks = config(width_multiplier)[1]

    def named_parameters(self):
        return list(self.params.items())

    def parameters(self):
        return list(self.params.values())

    def clone(self, dtype=None):
        cv = lambda t: (t.detach().to(dtype) if dtype is not None and t.is_floating_point()
                        else t.detach().clone()).clone()
        p = {k: cv(v).requires_grad_(True) for k, v in self.params.items()}
        b = {k: cv(v) for k, v in self.buffers.items()}
        return RefNet(p, b, self.width_multiplier, self.num_classes)

    def double(self):
        return self.clone(torch.float64)


def init_model(seed, width_multiplier=1.0, num_classes=10, input_channels=3):
    """The initial parameters the reference constructor draws under torch.manual_seed(seed):
    the same layers created in the same order (each draws its own initialisation)."""
    if seed is not None:
        torch.manual_seed(seed)
    stem, blocks = config(width_multiplier)
    params, buffers = {}, {}

    def take(prefix, mod):
        for n, p in mod.named_parameters():
            params[f"{prefix}.{n}"] = p.detach().clone().requires_grad_(True)
        for n, b in mod.named_buffers():
            buffers[f"{prefix}.{n}"] = b.detach().clone()

    take("conv1", nn.Conv2d(input_channels, stem, 3, 1, 1, bias=False))
    take("bn1", nn.BatchNorm2d(stem))
    for i, (ci, co, s) in enumerate(blocks):
        take(f"features.{i}.depthwise", nn.Conv2d(ci, ci, 3, s, 1, groups=ci, bias=False))
        take(f"features.{i}.bn1", nn.BatchNorm2d(ci))
        take(f"features.{i}.pointwise", nn.Conv2d(ci, co, 1, bias=False))
        take(f"features.{i}.bn2", nn.BatchNorm2d(co))
    take("classifier", nn.Linear(blocks[-1][1], num_classes))
    return RefNet(params, buffers, width_multiplier, num_classes)


class _Relu:
    def __init__(self, replay=None):
        self.replay = list(replay) if replay is not None else None
        self.used = []

    def __call__(self, x):
        if self.replay is None:
            y = F.relu(x)
            self.used.append((y > 0).detach())
            return y
        m = self.replay.pop(0)
        self.used.append(m)
        return x * m.to(x.dtype)


def forward(net, x, training=True, relus=None):
    """Logits and the 13 ReLU masks used (forward order).  training: batch-statistics
    BatchNorm that updates net.buffers in place, as nn.BatchNorm2d does."""
    P, Bf = net.params, net.buffers
    relu = _Relu(relus)

    def bn(name, t):
        if training and f"{name}.num_batches_tracked" in Bf:
            Bf[f"{name}.num_batches_tracked"] += 1
        return F.batch_norm(t, Bf[f"{name}.running_mean"], Bf[f"{name}.running_var"],
                            P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)

    x = relu(bn("bn1", F.conv2d(x, P["conv1.weight"], None, 1, 1)))
    for i, (ci, co, s) in enumerate(net.blocks):
        pf = f"features.{i}"
        x = relu(bn(f"{pf}.bn1", F.conv2d(x, P[f"{pf}.depthwise.weight"], None, s, 1, 1, ci)))
        x = relu(bn(f"{pf}.bn2", F.conv2d(x, P[f"{pf}.pointwise.weight"], None, 1, 0)))
    x = F.adaptive_avg_pool2d(x, (1, 1))
    x = x.view(x.size(0), -1)
    return F.linear(x, P["classifier.weight"], P["classifier.bias"]), relu.used


def make_optimizer(net, optimizer_type, lr):
    """The reference's _create_optimizer settings."""
    t = optimizer_type.lower()
    if t == "adam":
        return torch.optim.Adam(net.parameters(), lr=lr)
    if t == "sgd":
        return torch.optim.SGD(net.parameters(), lr=lr, momentum=0.9)
    if t == "adamw":
        return torch.optim.AdamW(net.parameters(), lr=lr)
    raise ValueError(f"Unknown optimizer type: {optimizer_type}")


def train_step(net, opt, data, targets, relus=None):
    """One iteration of the reference's _train_epoch.  Returns (loss, n_correct, logits,
    masks used)."""
    opt.zero_grad()
    out, used = forward(net, data, True, relus)
    loss = F.cross_entropy(out, targets)
    loss.backward()
    opt.step()
    _, pred = torch.max(out.data, 1)
    return loss.item(), int((pred == targets).sum().item()), out.detach(), used


def train_epochs(net, batches, epochs, lr, optimizer_type, relus=None):
    """train_local_model minus validation / checkpoints: batches is one epoch's list of
    (data, targets), replayed each epoch; relus one mask list per step.  Returns the
    reference's metrics dict plus 'masks' (per step)."""
    opt = make_optimizer(net, optimizer_type, lr)
    ri = iter(relus) if relus is not None else None
    total, loss, acc, masks = 0, 0.0, 0.0, []
    for _ in range(epochs):
        running, correct, seen = 0.0, 0, 0
        for data, targets in batches:
            li, c, _, used = train_step(net, opt, data, targets,
                                        next(ri) if ri is not None else None)
            masks.append(used)
            running += li
            correct += c
            seen += targets.size(0)
        loss, acc = running / len(batches), correct / seen
        total += seen
    return dict(loss=loss, accuracy=acc, epochs_completed=epochs, samples_processed=total,
                masks=masks)


def eval_logits(net, data, batch=32):
    with torch.no_grad():
        return torch.cat([forward(net, data[i:i + batch], False)[0]
                          for i in range(0, data.shape[0], batch)])


def param_vector(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])
