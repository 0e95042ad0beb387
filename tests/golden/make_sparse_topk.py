"""Generate tests/golden/sparse_topk.json by running the REFERENCE top-k compressor.

Run only where the reference checkout is available, with it on PYTHONPATH:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python tests/golden/make_sparse_topk.py

For tie-free tensors of 1, 7 and 300 elements (every magnitude distinct, so torch.topk's
selection is unique) at sparsity ratios 0.0, 0.5, 0.9 and 1.0 the file records what the
reference's TopKSparsificationCompressor._sparsify_tensor / _desparsify_tensor
(src/shared/compression.py:327-365) return: the indices in the reference's own (magnitude)
order, the values' and the desparsified tensor's uint32 bit patterns, next to the inputs' bit
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
RATIOS = [0.0, 0.5, 0.9, 1.0]


def tie_free(n, seed):
    """n fp32 values with n distinct magnitudes (multiples of 2^-10) and mixed signs."""
    rng = np.random.default_rng(seed)
    mag = rng.permutation(np.arange(1, n + 1)).astype(np.float32) * np.float32(2.0 ** -10)
    return (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=n)).astype(np.float32)


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
    from src.shared.compression import TopKSparsificationCompressor
    out = {"generator": "tests/golden/make_sparse_topk.py", "torch": torch.__version__,
           "numpy": np.__version__, "inputs_u32": {}, "cases": {}}
    for n in SIZES:
        x = tie_free(n, 100 + n)
        assert np.unique(np.abs(x)).size == n
        out["inputs_u32"][str(n)] = _bits(x)
        for ratio in RATIOS:
            c = TopKSparsificationCompressor(sparsity_ratio=ratio)
            t = torch.from_numpy(x.copy())
            values, indices, shape = c._sparsify_tensor(t)
            dense = c._desparsify_tensor(values, indices, shape, str(t.dtype))
            out["cases"][f"n{n}_r{ratio}"] = {
                "numel": n, "sparsity_ratio": ratio, "k": int(indices.numel()),
                "indices": [int(i) for i in indices.tolist()],
                "values_u32": _bits(values.numpy()),
                "dense_u32": _bits(dense.contiguous().numpy()),
            }
    with open(os.path.join(OUT, "sparse_topk.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
