"""fh_update_stats (per client row and segment: max |w| over the finite values, and a
NaN / Inf flag) against the plain loop of tests/small_ref.py (pinned to isfinite /
abs().amax() by test_small_ref_cpu.py).

Three client rows with a row stride larger than the payload (the padding holds NaN: a read
past a segment would raise a flag), segments of 1, 63, 64, 255, 256, 257, 1000 and 0 elements
(an empty segment: absmax 0, flag 0), the maximum carried by a negative value at the first
element, the last, and at offset 256 of a segment (the block's second pass), a segment of
denormals only, and NaN / +Inf / -Inf at those positions and on both sides of a clean
segment and of the empty one.  Flags are asserted everywhere, absmax exactly wherever the
flag is 0."""
from datetime import datetime

import pytest
import torch

import small_ref as sr
from fedhip import ops
from src.shared.models import ModelUpdate
from src.shared.validation import ModelUpdateValidator, ValidationError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LENS = [1000, 257, 64, 0, 1, 63, 255, 256, 257, 1000, 300]
OFFS = [0]
for _n in LENS:
    OFFS.append(OFFS[-1] + _n)
P = OFFS[-1]
NC = 3
DENORMAL_SEG = 5


def _pos(z, t):
    """Client z's marked element of segment t: first, last, offset 256 (else the middle)."""
    n = LENS[t]
    return OFFS[t] + (0, n - 1, 256 if n > 256 else n // 2)[z]


def _rows(seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.rand(NC, P, generator=g) * 2 - 1
    for z in range(NC):
        for t, n in enumerate(LENS):
            if n:
                rows[z, _pos(z, t)] = -(2.0 + t + 0.25 * z)  # the maximum is a negative value
        rows[z, OFFS[DENORMAL_SEG]:OFFS[DENORMAL_SEG + 1]] = torch.linspace(
            -1e-39, 1e-39, LENS[DENORMAL_SEG]) + 1e-42 * (z + 1)
    return rows


def _run(rows):
    buf = torch.full((NC, P + 37), float("nan"), device=DEV)
    view = buf[:, :P]  # row stride P + 37
    view.copy_(rows)
    seg = torch.tensor(OFFS, dtype=torch.int64, device=DEV)
    absmax, bad = ops.update_stats(view, seg, NC)
    torch.cuda.synchronize()
    assert absmax.shape == (NC, len(LENS)) and bad.shape == (NC, len(LENS))
    return absmax.cpu(), bad.cpu()


def _check(rows, absmax, bad):
    for z in range(NC):
        wm, wb = sr.update_stats(rows[z], OFFS)
        assert bad[z].tolist() == wb.tolist(), z
        for t in range(len(LENS)):
            seg = rows[z, OFFS[t]:OFFS[t + 1]]
            assert int(bad[z, t]) == int((~torch.isfinite(seg)).any()), (z, t)
            if not int(bad[z, t]):
                assert sr.same_bits(absmax[z, t], wm[t]), (z, t, absmax[z, t].item(), wm[t].item())
                ref = seg.abs().amax() if seg.numel() else torch.tensor(0.0)
                assert sr.same_bits(absmax[z, t], ref), (z, t)


def test_update_stats_finite_rows():
    rows = _rows(1)
    absmax, bad = _run(rows)
    assert not bad.any()
    _check(rows, absmax, bad)
    for z in range(NC):
        for t, n in enumerate(LENS):
            if t == DENORMAL_SEG:  # denormals are not flushed
                assert 0.0 < absmax[z, t].item() < 2.0 ** -126
            elif n:
                assert absmax[z, t].item() == 2.0 + t + 0.25 * z
            else:
                assert sr.same_bits(absmax[z, t], torch.tensor(0.0))


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf"])
def test_update_stats_nonfinite(kind):
    v = float(kind)
    rows = _rows(2)
    flagged = {0, 1, 2, 4, 5, 7, 9}
    for z in range(NC):
        rows[z, _pos(z, 0)] = v   # first / last / offset 256 of a 1000-element segment
        rows[z, _pos(z, 1)] = v   # ... of a 257-element one (offset 256 is its last element)
        rows[z, _pos(z, 9)] = v
        # the elements on both sides of the empty segment 3 and of the clean segment 6
        rows[z, OFFS[3] - 1] = v
        rows[z, OFFS[4]] = v
        rows[z, OFFS[6] - 1] = v
        rows[z, OFFS[7]] = v
    absmax, bad = _run(rows)
    for z in range(NC):
        assert {t for t in range(len(LENS)) if int(bad[z, t])} == flagged, z
    assert not bad[:, 3].any() and not bad[:, 6].any() and not bad[:, 8].any()
    _check(rows, absmax, bad)


def _update(w):
    return ModelUpdate(client_id="c0", round_number=1, model_weights=w, num_samples=10,
                       training_loss=0.5, privacy_budget_used=0.5, compression_ratio=0.8,
                       timestamp=datetime.now())


@pytest.mark.parametrize("v", [float("inf"), -float("inf")])
def test_validator_rejects_infinite_values(v):
    g = torch.Generator().manual_seed(3)
    w = {"fc1.weight": torch.randn(10, 257, generator=g) * 0.05,
         "fc1.bias": torch.randn(10, generator=g) * 0.05,
         "fc2.weight": torch.randn(3, 64, generator=g) * 0.05}
    assert ModelUpdateValidator().validate_model_update(_update(w))
    for name, at in (("fc1.weight", -1), ("fc1.bias", 0), ("fc2.weight", 0)):
        bad = {k: t.clone() for k, t in w.items()}
        bad[name].view(-1)[at] = v
        with pytest.raises(ValidationError, match=f"Infinite values found in layer {name}"):
            ModelUpdateValidator().validate_model_update(_update(bad))
