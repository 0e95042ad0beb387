"""Generate tests/golden/compress_edges.json by running the REFERENCE quantiser.

Run only where the reference checkout is available, with it on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python tests/golden/make_compress_edges.py

For every input of tests/compress_cases.fixture_inputs() (values on exact halves at
scale 1.0, a narrow range far from zero, a 16-bit spread) the file records what the
reference's QuantizationCompressor._quantize_tensor / _dequantize_tensor
(src/shared/compression.py:203-244) return: scale, zero point, the codes and the
dense tensor's uint32 bit patterns.  Inputs are not stored: the tests rebuild them
from the same builders.  Data only.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))

import compress_cases as cc  # noqa: E402


def _stub_lz4():
    # compression.py imports lz4 at module level; the LZ4 compressor is not exercised
    lz4 = types.ModuleType("lz4")
    lz4.frame = types.ModuleType("lz4.frame")
    sys.modules.setdefault("lz4", lz4)
    sys.modules.setdefault("lz4.frame", lz4.frame)


def main():
    _stub_lz4()
    from src.shared.compression import QuantizationCompressor
    out = {"generator": "tests/golden/make_compress_edges.py", "torch": torch.__version__,
           "numpy": np.__version__, "cases": {}}
    for name, (x, bits, sym) in cc.fixture_inputs().items():
        q = QuantizationCompressor(bits=bits, symmetric=sym)
        t = torch.from_numpy(x.copy())
        codes, scale, zp = q._quantize_tensor(t)
        deq = q._dequantize_tensor(codes, scale, zp, t.shape, str(t.dtype))
        out["cases"][name] = {
            "bits": bits, "symmetric": sym, "numel": int(x.size),
            "scale": float(scale), "zero_point": int(zp),
            "codes_dtype": str(codes.dtype).replace("torch.", ""),
            "codes": [int(c) for c in codes.reshape(-1).tolist()],
            "dense_u32": [int(b) for b in deq.contiguous().numpy().view(np.uint32).tolist()],
        }
    with open(os.path.join(OUT, "compress_edges.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
