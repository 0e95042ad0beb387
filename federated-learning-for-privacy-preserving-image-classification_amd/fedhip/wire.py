"""The gRPC edge of the packed path: wire format and convergence norms.

Wire format.  The reference ships a client's weights as
``torch.save(get_model_weights())`` bytes, hex-encoded into the message
(src/shared/serialization.py:28-48, :105; grpc_utils.py:127).  A packed round
holds every client as a row of one device matrix, so the edge is one
device->host copy of the [clients, P] block, then per client the same dict of
fresh tensors (named_parameters order, clones — never views, or torch.save would
write the whole packed storage) serialised exactly as the reference does:
byte-identical output (golden G9).  The inverse stacks received updates into
packed rows with one host->device copy.

Convergence.  ConvergenceDetector._calculate_weight_change_metrics
(src/aggregation/convergence.py:189-217): per layer ||current - previous|| and
||current|| (torch fp32 norms, .item()), squared and summed in double.  Here the
two per-layer reductions over P run on the chip (fh_dp_delta_sqnorm, fp64
accumulation), each layer's norm is rounded to fp32 like torch's result, and the
nseg-long sums are finished on the host in double.  The reference's torch CPU
norm accumulates in fp32, so the two agree to ~1e-6 relative (tested at 1e-5).
"""
from __future__ import annotations

import io
import math
from typing import Dict, List, Sequence

import torch

from . import ops


def client_weights(rows_cpu: torch.Tensor, layout, slot: int) -> Dict[str, torch.Tensor]:
    """get_model_weights() of packed client `slot` (models_pytorch.py:25-28): fresh tensors
    in named_parameters order."""
    return {n: rows_cpu[slot, o:o + _numel(s)].reshape(s).clone()
            for n, s, o in zip(layout.names, layout.shapes, layout.offsets)}


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def serialize_weights(weights: Dict[str, torch.Tensor]) -> bytes:
    """ModelWeightSerializer.serialize_weights (serialization.py:28-48): torch.save bytes."""
    buf = io.BytesIO()
    torch.save(weights, buf)
    return buf.getvalue()


def packed_to_weight_dicts(rows: torch.Tensor, layout, nclients: int) -> List[Dict[str, torch.Tensor]]:
    """All clients' weight dicts from device rows [>=nclients, >=P] with ONE D2H copy."""
    host = rows[:nclients, :layout.P].to("cpu")
    return [client_weights(host, layout, z) for z in range(nclients)]


def weight_dicts_to_packed(dicts: Sequence[Dict[str, torch.Tensor]], layout, device,
                           row_stride: int = None) -> torch.Tensor:
    """Received weight dicts -> packed device rows [C, row_stride] (one H2D copy); rows are
    zero-padded to `row_stride` (default: P rounded up to 64 floats, as PackedTrainer)."""
    P = layout.P
    stride = row_stride or ((P + 63) // 64) * 64
    host = torch.zeros(len(dicts), stride, dtype=torch.float32, pin_memory=False)
    for z, d in enumerate(dicts):
        for n, s, o in zip(layout.names, layout.shapes, layout.offsets):
            t = d[n]
            if tuple(t.shape) != tuple(s):
                raise ValueError(f"client {z}: {n} has shape {tuple(t.shape)}, expected {s}")
            host[z, o:o + t.numel()] = t.reshape(-1).to(torch.float32)
    return host.to(device)


# ------------------------------------------------------------------ sparse top-k payloads
def sparse_to_payloads(updates, layout, nclients: int) -> List[Dict]:
    """The clients' top-k uploads as TopKSparsificationCompressor.compress builds them
    (compression.py:262-297), from device payload rows (fedhip.sparse.SparseUpdates) with ONE
    D2H copy.  Per client ``{'compressed_weights': {name: {'values': fp32 [k], 'indices':
    int64 [k]}}, 'metadata': {...}}``; the indices are flat and ascending (D15)."""
    sp = updates.plan
    K = sp.K
    host = torch.stack([updates.idx[:nclients, :K],
                        updates.val[:nclients, :K].view(torch.int32)]).to("cpu")
    idx, val = host[0].to(torch.int64), host[1].view(torch.float32)
    ratio = max(0.0, min(1.0, sp.ratio))
    out = []
    for z in range(nclients):
        cw, params = {}, {}
        for s, (n, shape) in enumerate(zip(layout.names, layout.shapes)):
            a, b = sp.koff_host[s], sp.koff_host[s + 1]
            cw[n] = {"values": val[z, a:b].clone(), "indices": idx[z, a:b].clone()}
            params[n] = {"original_shape": torch.Size(shape), "original_dtype": "torch.float32",
                         "sparsity_ratio": ratio}
        out.append({"compressed_weights": cw,
                    "metadata": {"algorithm": f"topk_sparsification_{ratio}",
                                 "sparsity_ratio": ratio, "sparsification_params": params}})
    return out


def sort_segment(indices: torch.Tensor, values: torch.Tensor):
    """One layer's received (indices, values) in ascending index order (the reference ships
    them in magnitude order); stable, so equal indices stay for validation to flag."""
    order = torch.sort(indices.reshape(-1).to(torch.int64), stable=True).indices
    return indices.reshape(-1)[order], values.reshape(-1)[order]


def payloads_to_sparse(payloads: Sequence[Dict], layout, plan, device):
    """Received top-k uploads -> validated device payload rows (one H2D copy).  payloads: per
    client the ``compressed_weights`` dict, or a dict holding it under that key (what
    sparse_to_payloads returns); plan: the fedhip.sparse.SparsePlan of the layout and ratio.
    Indices may come in any order.  A layer with a wrong k, or one fh_sparse_validate flags
    (index out of range, repeated index), raises FedHipError naming client and layer before any
    consumer sees the payload."""
    from .sparse import SparseUpdates, sparse_validate
    K, C = plan.K, len(payloads)
    stride = (K + 3) // 4 * 4
    host = torch.zeros(2, max(C, 1), stride, dtype=torch.int32)
    lim = 2 ** 31 - 1
    for z, p in enumerate(payloads):
        cw = p.get("compressed_weights", p)
        for s, n in enumerate(layout.names):
            a, b = plan.koff_host[s], plan.koff_host[s + 1]
            if n not in cw:
                raise ops.FedHipError(f"client {z}: layer {n} is missing from the payload")
            ind, v = cw[n]["indices"], cw[n]["values"]
            if ind.numel() != b - a or v.numel() != b - a:
                raise ops.FedHipError(f"client {z}: layer {n} carries {ind.numel()} indices / "
                                      f"{v.numel()} values, expected k = {b - a}")
            ind, v = sort_segment(ind, v)
            # an index no int32 holds is out of range for every layer: keep it so after the cast
            host[0, z, a:b] = ind.clamp(-1, lim).to(torch.int32)
            host[1, z, a:b] = v.to(torch.float32).view(torch.int32)
    dev = host.to(device)
    upd = SparseUpdates(dev[0, :C, :K], dev[1, :C, :K].view(torch.float32), plan)
    bad = sparse_validate(upd).to("cpu")
    if bool(bad.any()):
        z, s = [int(t) for t in bad.nonzero()[0]]
        raise ops.FedHipError(f"client {z}: layer {layout.names[s]} has indices outside "
                              f"[0, {plan.plan.lengths[s]}) or repeated")
    return upd


# ------------------------------------------------------------------ quantised payloads
def _codes_per_byte(raw, cw: int, n: int):
    """numpy uint8 [n]: the first n codes of cw bits each in the bytes raw, low bits first."""
    import numpy as np
    if cw == 8:
        return raw[:n].copy()
    sh = (np.arange(8 // cw, dtype=np.uint8) * cw)[None, :]
    return ((raw[:, None] >> sh) & np.uint8((1 << cw) - 1)).reshape(-1)[:n].copy()


def _bytes_of_codes(codes, cw: int):
    """The inverse: numpy uint8 [ceil(n * cw / 8)], unused high bits of the last byte zero."""
    import numpy as np
    if cw == 8:
        return codes
    per = 8 // cw
    pad = np.zeros(-(-codes.size // per) * per, np.uint8)
    pad[:codes.size] = codes
    sh = (np.arange(per, dtype=np.uint8) * cw)[None, :]
    return np.bitwise_or.reduce(pad.reshape(-1, per) << sh, axis=1).astype(np.uint8)


def quant_to_payloads(updates, layout, nclients: int, symmetric: bool = None) -> List[Dict]:
    """The clients' quantised uploads as QuantizationCompressor.compress builds them
    (compression.py:138-172), from a device payload (fedhip.quantpack.QuantUpdates) with ONE
    D2H copy.  Per client ``{'compressed_weights': {name: uint8 tensor of the layer's shape},
    'metadata': {'algorithm', 'bits', 'symmetric', 'quantization_params': {name: {'scale',
    'zero_point', 'original_shape', 'original_dtype'}}}}``, one code per byte.  A layer the
    quantiser passed through (asymmetric mode on a constant layer: the reference raises there)
    has no such form: FedHipError naming client and layer.  symmetric: the quantiser's mode for
    the metadata; by default ``updates.symmetric``, which compress_rows and payloads_to_quant
    record.  It is never guessed from the zero points: a payload of unknown mode is refused."""
    from .quantpack import INT64_MIN
    qp = updates.plan
    B, nseg, n = qp.B, qp.plan.nseg, int(nclients)
    dev = torch.cat([updates.codes[:n, :B].reshape(-1),
                     updates.scale[:n].reshape(-1).view(torch.uint8),
                     updates.zp[:n].reshape(-1).view(torch.uint8)]).to("cpu")
    codes = dev[:n * B].view(n, B).numpy()
    scale = dev[n * B:n * B + 8 * n * nseg].view(torch.float64).view(n, nseg).tolist()
    zp = dev[n * B + 8 * n * nseg:].view(torch.int64).view(n, nseg).tolist()
    if symmetric is None:
        symmetric = updates.symmetric
    if symmetric is None:
        raise ops.FedHipError("quant_to_payloads: the quantiser's mode is not recorded in the "
                              "payload (updates.symmetric is None): pass symmetric=")
    out = []
    for z in range(n):
        cw, params = {}, {}
        for s, (name, shape) in enumerate(zip(layout.names, layout.shapes)):
            if zp[z][s] == INT64_MIN:
                raise ops.FedHipError(f"client {z}: layer {name} is constant and was passed "
                                      "through unquantised: the reference's upload format "
                                      "cannot express it")
            a = qp.boff_host[s]
            flat = _codes_per_byte(codes[z, a:a + qp.seg_bytes[s]], qp.cw, qp.plan.lengths[s])
            cw[name] = torch.from_numpy(flat).reshape(tuple(shape))
            params[name] = {"scale": scale[z][s], "zero_point": zp[z][s],
                            "original_shape": torch.Size(shape),
                            "original_dtype": "torch.float32"}
        out.append({"compressed_weights": cw,
                    "metadata": {"algorithm": f"quantization_{qp.bits}bit", "bits": qp.bits,
                                 "symmetric": bool(symmetric), "quantization_params": params}})
    return out


def payloads_to_quant(payloads: Sequence[Dict], layout, plan, device):
    """Received quantised uploads -> validated device payload (one H2D copy).  payloads: per
    client what quant_to_payloads returns, or a dict with ``compressed_weights`` and
    ``quantization_params`` alone; plan: the fedhip.quantpack.QuantPlan of the layout and bit
    width.  A missing layer, a wrong shape or dtype, a zero point no int64 holds, and whatever
    fh_quant_validate flags (a code >= 2^bits, a scale that is not finite or negative) raise
    FedHipError naming client and layer before any consumer sees the payload."""
    import numpy as np
    from .quantpack import INT64_MIN, QuantUpdates, quant_validate
    B, nseg, C = plan.B, plan.plan.nseg, len(payloads)
    n = max(C, 1)
    host = np.zeros(n * B + 20 * n * nseg, np.uint8)
    codes = host[:n * B].reshape(n, B)
    scale = host[n * B:n * B + 8 * n * nseg].view(np.float64).reshape(n, nseg)
    zp = host[n * B + 8 * n * nseg:n * B + 16 * n * nseg].view(np.int64).reshape(n, nseg)
    modes = set()
    for z, p in enumerate(payloads):
        cw = p["compressed_weights"]
        params = p["metadata"]["quantization_params"] if "metadata" in p \
            else p["quantization_params"]
        modes.add(p.get("metadata", {}).get("symmetric"))
        for s, (name, shape) in enumerate(zip(layout.names, layout.shapes)):
            if name not in cw or name not in params:
                raise ops.FedHipError(f"client {z}: layer {name} is missing from the payload")
            t = cw[name]
            if t.dtype != torch.uint8:
                raise ops.FedHipError(f"client {z}: layer {name} has dtype {t.dtype}, expected "
                                      "torch.uint8")
            if tuple(t.shape) != tuple(shape):
                raise ops.FedHipError(f"client {z}: layer {name} has shape {tuple(t.shape)}, "
                                      f"expected {tuple(shape)}")
            zero = int(params[name]["zero_point"])
            if not INT64_MIN < zero < 2 ** 63:
                raise ops.FedHipError(f"client {z}: layer {name} has a zero point no int64 holds")
            flat = t.reshape(-1).cpu().numpy()
            if plan.cw < 8 and int(flat.max()) >> plan.cw:  # would not survive the packing
                raise ops.FedHipError(f"client {z}: layer {name} has a code >= 2^{plan.bits}")
            a = plan.boff_host[s]
            codes[z, a:a + plan.seg_bytes[s]] = _bytes_of_codes(flat, plan.cw)
            scale[z, s] = float(params[name]["scale"])
            zp[z, s] = zero
    dev = torch.from_numpy(host).to(device)
    f64 = dev[n * B:n * B + 8 * n * nseg].view(torch.float64).view(n, nseg)
    i64 = dev[n * B + 8 * n * nseg:n * B + 16 * n * nseg].view(torch.int64).view(n, nseg)
    f32 = dev[n * B + 16 * n * nseg:].view(torch.float32).view(n, nseg)
    mode = modes.pop() if len(modes) == 1 else None   # what every client's metadata states
    upd = QuantUpdates(dev[:n * B].view(n, B)[:C], f64[:C], i64[:C], f32[:C], plan,
                       None if mode is None else bool(mode))
    bad = quant_validate(upd).to("cpu")
    if bool(bad.any()):
        z, s = [int(t) for t in bad.nonzero()[0]]
        raise ops.FedHipError(f"client {z}: layer {layout.names[s]} has a code >= "
                              f"2^{plan.bits}, or a scale that is not finite or negative")
    return upd


def weight_change_metrics(current: torch.Tensor, previous: torch.Tensor,
                          seg_offsets: torch.Tensor) -> Dict[str, float]:
    """{'norm': ||current - previous||, 'relative': norm / ||current||} over the layers
    (convergence.py:189-217).  current / previous: flat device rows [>=P]; seg_offsets:
    device int64 [nseg+1] layer boundaries."""
    nseg = seg_offsets.numel() - 1
    cur = current.reshape(1, -1)
    diff_sq = ops.dp_delta_sqnorm(cur, previous.reshape(1, -1), seg_offsets, 1)
    cur_sq = ops.dp_delta_sqnorm(cur, None, seg_offsets, 1)
    d = diff_sq.reshape(-1).tolist()
    c = cur_sq.reshape(-1).tolist()
    total, total_cur = 0.0, 0.0
    for t in range(nseg):
        dn = float(torch.tensor(math.sqrt(d[t]), dtype=torch.float32))  # torch fp32 .item()
        cn = float(torch.tensor(math.sqrt(c[t]), dtype=torch.float32))
        total += dn ** 2
        total_cur += cn ** 2
    norm = math.sqrt(total)
    cur_norm = math.sqrt(total_cur)
    return {"norm": norm, "relative": norm / cur_norm if cur_norm > 0 else 0.0}
