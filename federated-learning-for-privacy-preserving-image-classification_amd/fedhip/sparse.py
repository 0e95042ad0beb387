"""Sparse top-k updates on HIP (csrc/sparse.hip): what a client uploads under
top-k compression — k (index, value) pairs per parameter tensor — and the aggregation from it.

Reference: TopKSparsificationCompressor.compress ships ``{'values', 'indices'}`` per layer
(src/shared/compression.py:262-297) and ``_desparsify_tensor`` (:346-365) rebuilds the dense
tensor.  Here a client's payload is two packed rows of K = sum_s k_s entries, ``idx`` (int32,
segment-local flat index, strictly ascending inside a segment) and ``val`` (fp32); segment s
sits at ``[koff[s], koff[s+1])``.

    topk_pack_rows      the keep mask of ``compress.topk_rows`` -> payload rows
    sparse_validate     per (client, segment): indices in range and strictly ascending
    sparse_unpack_rows  payload -> dense rows, bit for bit ``topk_rows``' output
    sparse_fedavg       payload -> weighted sum, bit for bit ``ops.fedavg_weighted_sum`` over
                        the unpacked rows, without materialising them

``sparse_unpack_rows`` and ``sparse_fedavg`` take validated payloads only: what
``topk_pack_rows`` wrote, or what passed ``sparse_validate`` (``wire.payloads_to_sparse`` runs
it on everything it receives).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ._lib import FedHipError, call, load, ptr, stream_handle
from .compress import SegmentPlan, topk_k
from .ops import _ws


class SparsePlan:
    """Payload layout of one SegmentPlan at one sparsity ratio: k [nseg] (host), koff
    [nseg+1] (exclusive prefix sum of k; host list and device int32), K = koff[nseg] and
    seg_lens [nseg] (device int64)."""

    def __init__(self, plan: SegmentPlan, sparsity_ratio: float):
        self.plan = plan
        self.ratio = float(sparsity_ratio)
        self.k = [topk_k(n, self.ratio) for n in plan.lengths]
        off = [0]
        for k in self.k:
            off.append(off[-1] + k)
        if off[-1] >= 2 ** 31 or max(plan.lengths) >= 2 ** 31:
            raise FedHipError("sparse payloads index with int32: a segment or K is too large")
        self.koff_host, self.K = off, off[-1]
        self.device = plan.device
        self.koff = torch.tensor(off, dtype=torch.int32, device=self.device)
        self.seg_lens = torch.tensor(plan.lengths, dtype=torch.int64, device=self.device)

    def empty(self, nclients: int) -> "SparseUpdates":
        """Uninitialised payload rows for nclients clients (row stride K rounded up to 4)."""
        stride = (self.K + 3) // 4 * 4
        idx = torch.empty(max(nclients, 1), stride, dtype=torch.int32, device=self.device)
        val = torch.empty(max(nclients, 1), stride, dtype=torch.float32, device=self.device)
        return SparseUpdates(idx[:nclients, :self.K], val[:nclients, :self.K], self)


@dataclass
class SparseUpdates:
    """idx (int32) / val (fp32): device rows [nclients, K] of one SparsePlan."""
    idx: torch.Tensor
    val: torch.Tensor
    plan: SparsePlan

    def __post_init__(self):
        for t, dt, what in ((self.idx, torch.int32, "idx"), (self.val, torch.float32, "val")):
            if t.dtype != dt or t.dim() != 2 or t.shape[1] < self.plan.K or t.stride(1) != 1 \
                    or t.device.type != self.plan.device.type:
                raise FedHipError(f"sparse updates: {what} must be {dt} device rows "
                                  f"[nclients, >= {self.plan.K}]")
        if self.idx.shape[0] != self.val.shape[0]:
            raise FedHipError("sparse updates: idx and val differ in their row count")

    @property
    def nclients(self) -> int:
        return self.idx.shape[0]


def _cs(t):
    return 0 if t is None else t.stride(0)


def _plan_args(sp: SparsePlan):
    p = sp.plan
    return ptr(p.seg_offsets), ptr(p.chunk_offsets), ptr(sp.koff), p.nseg, p.nchunks


def _rows(upd: SparseUpdates, nclients: Optional[int]) -> int:
    n = upd.nclients if nclients is None else int(nclients)
    if n > upd.nclients:
        raise FedHipError(f"sparse updates hold {upd.nclients} rows, {n} asked for")
    return n


def topk_pack_rows(upd: SparseUpdates, x, keep, nclients=None, base=None, count_out=None):
    """upd <- the kept elements of x - base (x without a base) in ascending index order
    (fh_topk_pack_rows); keep: the uint8 mask topk_rows wrote for the same x / base.
    count_out: int32 [nclients, nseg], the kept elements found per segment."""
    sp = upd.plan
    n = _rows(upd, nclients)
    need = int(load().fh_topk_pack_workspace(n, sp.plan.nchunks))
    ws = _ws(x.device).get(max(need, 1))
    seg, chunk, koff, nseg, nchunks = _plan_args(sp)
    call("fh_topk_pack_rows", ptr(x), x.stride(0), ptr(base), _cs(base), ptr(keep),
         keep.stride(0), ptr(upd.idx), upd.idx.stride(0), ptr(upd.val), upd.val.stride(0),
         ptr(count_out), n, seg, chunk, koff, nseg, nchunks, ptr(ws), ws.numel(),
         stream_handle())
    return upd


def sparse_validate(upd: SparseUpdates, nclients=None, bad_out=None):
    """int32 [nclients, nseg]: 1 where a segment's indices leave [0, len) or are not strictly
    ascending (fh_sparse_validate).  No host sync."""
    sp = upd.plan
    n = _rows(upd, nclients)
    if bad_out is None:
        bad_out = torch.empty(n, sp.plan.nseg, dtype=torch.int32, device=sp.device)
    call("fh_sparse_validate", ptr(upd.idx), upd.idx.stride(0), n, ptr(sp.seg_lens),
         ptr(sp.koff), sp.plan.nseg, ptr(bad_out), stream_handle())
    return bad_out


def sparse_unpack_rows(upd: SparseUpdates, out, nclients=None, base=None):
    """out[:nclients] <- base + dense(upd) (fh_sparse_unpack_rows): topk_rows' output.  out may
    be the base rows unless the base is one broadcast row."""
    n = _rows(upd, nclients)
    call("fh_sparse_unpack_rows", ptr(upd.idx), upd.idx.stride(0), ptr(upd.val),
         upd.val.stride(0), ptr(base), _cs(base), ptr(out), out.stride(0), n, *_plan_args(upd.plan),
         stream_handle())
    return out


def sparse_fedavg(upd: SparseUpdates, weights_f32, base, out, row_index=None, accumulate=False):
    """out = [out +] sum_k fl32(w_k) * fl32(base + dense(upd)[row_index[k]]), sequential in k
    (fh_sparse_fedavg).  base: the one row every update is a delta of; out: another row."""
    C = weights_f32.numel()
    if row_index is None and C > upd.nclients:
        raise FedHipError(f"sparse_fedavg: {C} weights for {upd.nclients} payload rows")
    seg, chunk, koff, nseg, nchunks = _plan_args(upd.plan)
    call("fh_sparse_fedavg", ptr(upd.idx), upd.idx.stride(0), ptr(upd.val), upd.val.stride(0),
         ptr(row_index), ptr(weights_f32), C, ptr(base), seg, chunk, koff, nseg, nchunks,
         ptr(out), int(bool(accumulate)), stream_handle())
    return out
