"""Packed quantised updates on HIP (csrc/quantpack.hip): what a client uploads
under 1..8-bit quantisation — one code per element plus a scale and a zero point per parameter
tensor — and the aggregation from it.

Reference: QuantizationCompressor.compress ships a ``uint8`` tensor per layer and
``quantization_params`` (src/shared/compression.py:138-172); ``_dequantize_tensor`` (:230-244)
rebuilds the dense tensor.  Here a client's payload is one code row of B bytes: segment s starts
at byte ``boff[s]`` (a multiple of 16) and holds its elements' codes ``cw`` bits each, low bits
first (cw = 1, 2, 4, 8 for bits 1, 2, 3..4, 5..8), next to ``scale`` (float64) and ``zp`` (int64)
exactly as ``fh_quantize_rows`` writes them.  A segment the quantiser passed through (asymmetric
mode on a constant segment, ``zp == INT64_MIN``) ships the sign bits of its elements as codes and
its first element as ``passv``.

    quant_pack_rows     the one-byte codes of ``compress.quantize_rows`` -> payload rows
    quant_validate      per (client, segment): codes below 2^bits, scale finite and >= 0
    quant_unpack_rows   payload -> dense rows, bit for bit ``quantize_rows``' output
    quant_fedavg        payload -> weighted sum, bit for bit ``ops.fedavg_weighted_sum`` over
                        the unpacked rows, without materialising them

``quant_unpack_rows`` and ``quant_fedavg`` take validated payloads only: what ``quant_pack_rows``
wrote, or what passed ``quant_validate`` (``wire.payloads_to_quant`` runs it on everything it
receives).  The deterministic quantiser only: the stochastic one has another header.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ._lib import FedHipError, call, ptr, stream_handle
from .compress import SegmentPlan

INT64_MIN = -2 ** 63  # zp of a segment fh_quantize_rows passed through


def code_width(bits: int) -> int:
    """Bits a packed code occupies: 1, 2, 4 or 8."""
    bits = int(bits)
    if not 1 <= bits <= 8:
        raise FedHipError(f"packed quantised updates hold uint8 codes: bits must be in [1, 8] "
                          f"(got {bits})")
    return 1 if bits == 1 else 2 if bits == 2 else 4 if bits <= 4 else 8


class QuantPlan:
    """Payload layout of one SegmentPlan at one bit width: cw, boff [nseg+1] (exclusive prefix
    sum of the segments' ceil(len * cw / 8) bytes, each rounded up to 16; host list and device
    int64), B = boff[nseg] and seg_lens [nseg] (device int64)."""

    def __init__(self, plan: SegmentPlan, bits: int):
        self.plan = plan
        self.bits = int(bits)
        self.cw = code_width(bits)
        self.seg_bytes = [(n * self.cw + 7) // 8 for n in plan.lengths]
        off = [0]
        for nb in self.seg_bytes:
            off.append(off[-1] + (nb + 15) // 16 * 16)
        if max(plan.lengths) >= 2 ** 31:
            raise FedHipError("packed quantised updates: a segment is too large")
        self.boff_host, self.B = off, off[-1]
        self.device = plan.device
        self.boff = torch.tensor(off, dtype=torch.int64, device=self.device)
        self.seg_lens = torch.tensor(plan.lengths, dtype=torch.int64, device=self.device)

    def empty(self, nclients: int) -> "QuantUpdates":
        """Uninitialised payload rows for nclients clients."""
        n, nseg = max(nclients, 1), self.plan.nseg
        dev = self.device
        return QuantUpdates(torch.empty(n, self.B, dtype=torch.uint8, device=dev)[:nclients],
                            torch.empty(n, nseg, dtype=torch.float64, device=dev)[:nclients],
                            torch.empty(n, nseg, dtype=torch.int64, device=dev)[:nclients],
                            torch.empty(n, nseg, dtype=torch.float32, device=dev)[:nclients], self)


@dataclass
class QuantUpdates:
    """Device tensors of one QuantPlan: codes (uint8 [nclients, B]), scale (float64), zp (int64)
    and passv (fp32), the last three contiguous [nclients, nseg].  symmetric: the mode of the
    quantiser that filled them (compress_rows and wire.payloads_to_quant set it; None: not
    known).  No kernel reads it; the upload metadata of wire.quant_to_payloads does."""
    codes: torch.Tensor
    scale: torch.Tensor
    zp: torch.Tensor
    passv: torch.Tensor
    plan: QuantPlan
    symmetric: Optional[bool] = None

    def __post_init__(self):
        p = self.plan
        c = self.codes
        if c.dtype != torch.uint8 or c.dim() != 2 or c.shape[1] < p.B or c.stride(1) != 1 \
                or c.device.type != p.device.type:
            raise FedHipError(f"quantised updates: codes must be uint8 device rows "
                              f"[nclients, >= {p.B}]")
        for t, dt, what in ((self.scale, torch.float64, "scale"), (self.zp, torch.int64, "zp"),
                            (self.passv, torch.float32, "passv")):
            if t.dtype != dt or tuple(t.shape) != (c.shape[0], p.plan.nseg) \
                    or not t.is_contiguous() or t.device.type != p.device.type:
                raise FedHipError(f"quantised updates: {what} must be contiguous {dt} "
                                  f"[nclients, nseg] on the device")

    @property
    def nclients(self) -> int:
        return self.codes.shape[0]


def _cs(t):
    return 0 if t is None else t.stride(0)


def _plan_args(qp: QuantPlan):
    p = qp.plan
    return ptr(p.seg_offsets), ptr(p.chunk_offsets), ptr(qp.boff), p.nseg, p.nchunks, qp.bits


def _rows(upd: QuantUpdates, nclients: Optional[int]) -> int:
    n = upd.nclients if nclients is None else int(nclients)
    if n > upd.nclients:
        raise FedHipError(f"quantised updates hold {upd.nclients} rows, {n} asked for")
    return n


def quant_pack_rows(upd: QuantUpdates, x, codes, nclients=None, base=None):
    """upd.codes / upd.passv <- the one-byte codes (uint8 rows indexed like x) that
    quantize_rows wrote for the same x / base, cw bits each (fh_quant_pack_rows).  upd.zp must
    already hold that call's zp_out: a passed-through segment packs the sign bits of x - base."""
    n = _rows(upd, nclients)
    call("fh_quant_pack_rows", ptr(codes), codes.stride(0), ptr(upd.zp), ptr(x), x.stride(0),
         ptr(base), _cs(base), ptr(upd.codes), upd.codes.stride(0), ptr(upd.passv), n,
         *_plan_args(upd.plan), stream_handle())
    return upd


def quant_validate(upd: QuantUpdates, nclients=None, bad_out=None):
    """int32 [nclients, nseg]: 1 where a segment holds a code >= 2^bits, a scale that is not
    finite or negative, or (passed through) a non-finite passv (fh_quant_validate).  No host
    sync."""
    qp = upd.plan
    n = _rows(upd, nclients)
    if bad_out is None:
        bad_out = torch.empty(n, qp.plan.nseg, dtype=torch.int32, device=qp.device)
    call("fh_quant_validate", ptr(upd.codes), upd.codes.stride(0), ptr(upd.scale), ptr(upd.zp),
         ptr(upd.passv), n, ptr(qp.seg_lens), ptr(qp.boff), qp.plan.nseg, qp.bits, ptr(bad_out),
         stream_handle())
    return bad_out


def quant_unpack_rows(upd: QuantUpdates, out, nclients=None, base=None):
    """out[:nclients] <- base + dequantize(upd) (fh_quant_unpack_rows): quantize_rows' output.
    out may be the base rows unless the base is one broadcast row."""
    n = _rows(upd, nclients)
    call("fh_quant_unpack_rows", ptr(upd.codes), upd.codes.stride(0), ptr(upd.scale), ptr(upd.zp),
         ptr(upd.passv), ptr(base), _cs(base), ptr(out), out.stride(0), n, *_plan_args(upd.plan),
         stream_handle())
    return out


def quant_fedavg(upd: QuantUpdates, weights_f32, base, out, row_index=None, accumulate=False):
    """out = [out +] sum_k fl32(w_k) * fl32(base + dequantize(upd)[row_index[k]]), sequential in
    k (fh_quant_fedavg).  base: the one row every update is a delta of, or None; out: another
    row."""
    C = weights_f32.numel()
    if row_index is None and C > upd.nclients:
        raise FedHipError(f"quant_fedavg: {C} weights for {upd.nclients} payload rows")
    seg, chunk, boff, nseg, nchunks, bits = _plan_args(upd.plan)
    call("fh_quant_fedavg", ptr(upd.codes), upd.codes.stride(0), ptr(upd.scale), ptr(upd.zp),
         ptr(upd.passv), ptr(row_index), ptr(weights_f32), C, ptr(base), seg, chunk, boff, nseg,
         nchunks, bits, ptr(out), int(bool(accumulate)), stream_handle())
    return out
