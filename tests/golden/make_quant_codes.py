"""Generate tests/golden/quant_codes.json by running the REFERENCE quantiser.

Run only where the reference checkout is available, with it on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python tests/golden/make_quant_codes.py

For tensors of 1, 7 and 300 elements at 1, 2, 3, 4 and 8 bits, symmetric and (where the tensor is
not constant: the reference raises on a constant one) asymmetric, the file records what the
reference's QuantizationCompressor._quantize_tensor / _dequantize_tensor
(src/shared/compression.py:203-244) return: the uint8 codes, the scale as the Python float's hex,
the zero point and the dequantised tensor's uint32 bit patterns, next to the inputs' bit
patterns.  Data only.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
SIZES = [1, 7, 300]
BITS = [1, 2, 3, 4, 8]


def tensor(n, seed):
    """n fp32 values around zero; the 300-element one also holds +0.0, -0.0 and a repeated
    extreme."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    if n >= 300:
        x[3], x[4] = 0.0, -0.0
        x[17] = x[np.argmax(x)]
    return x


def _stub_lz4():
    # compression.py imports lz4 at module level; the LZ4 compressor is not exercised
    lz4 = types.ModuleType("lz4")
    lz4.frame = types.ModuleType("lz4.frame")
    sys.modules.setdefault("lz4", lz4)
    sys.modules.setdefault("lz4.frame", lz4.frame)


def _bits(a):
    return [int(b) for b in np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()]


def main():
    _stub_lz4()
    from src.shared.compression import QuantizationCompressor
    out = {"generator": "tests/golden/make_quant_codes.py", "torch": torch.__version__,
           "numpy": np.__version__, "inputs_u32": {}, "cases": {}}
    for n in SIZES:
        x = tensor(n, 200 + n)
        out["inputs_u32"][str(n)] = _bits(x)
        for bits in BITS:
            for symmetric in (True, False):
                if not symmetric and float(x.min()) == float(x.max()):
                    continue
                c = QuantizationCompressor(bits=bits, symmetric=symmetric)
                t = torch.from_numpy(x.copy())
                q, scale, zp = c._quantize_tensor(t)
                assert q.dtype == torch.uint8
                dense = c._dequantize_tensor(q, scale, zp, t.shape, str(t.dtype))
                out["cases"][f"n{n}_b{bits}_{'sym' if symmetric else 'asym'}"] = {
                    "numel": n, "bits": bits, "symmetric": symmetric,
                    "codes": [int(v) for v in q.reshape(-1).tolist()],
                    "scale_hex": float(scale).hex(), "zero_point": int(zp),
                    "dense_u32": _bits(dense.contiguous().numpy()),
                }
    with open(os.path.join(OUT, "quant_codes.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
