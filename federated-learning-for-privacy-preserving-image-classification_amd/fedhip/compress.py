"""Update compression of packed client rows on HIP (csrc/compress.hip).

Reference: src/shared/compression.py — QuantizationCompressor (:123-247) and
TopKSparsificationCompressor (:250-368), applied per parameter tensor.  The
reference never wires compression into its live path; the
insertion point chosen here is the client update delta right
before FedAvg:

    w_k <- w_global + decompress(compress(w_k - w_global))     per tensor

which is what a server would reconstruct from a compressed upload of the delta.
``RankRound(compression=...)`` applies it to every client row of a round in
one pass per kernel (no host sync).

Not in the reference (csrc/efcomp.hip), off by default: error feedback
(``CompressionConfig(error_feedback=True)``: the client keeps what compression removed and
sends it with a later update) and unbiased stochastic rounding for the quantiser
(``stochastic=True``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from ._lib import FedHipError, call, load, ptr, stream_handle
from .ops import _ws


@dataclass
class CompressionConfig:
    """algorithm: "quantization" (bits, symmetric) or "topk" (sparsity_ratio).

    error_feedback: every client keeps what compression removed from its update and adds it
    to its next one (needs per-client residual rows).  stochastic
    ("quantization" only, bits >= 2): unbiased stochastic rounding instead of the reference's
    round-half-to-even.  sparse ("topk" only): a round also keeps every client's update as
    the packed (index, value) payload of fedhip/sparse.py and aggregates from it where it can
    (DESIGN.md D21); the global model is the same, bit for bit.  packed ("quantization" only,
    bits <= 8, not stochastic): the same for the quantiser, with the bit-packed codes of
    fedhip/quantpack.py as the payload.  All are off by default: the
    reference's compressors, bit for bit."""
    algorithm: str = "topk"
    sparsity_ratio: float = 0.9
    bits: int = 8
    symmetric: bool = True
    error_feedback: bool = False
    stochastic: bool = False
    sparse: bool = False
    packed: bool = False

    def __post_init__(self):
        if self.algorithm not in ("quantization", "topk"):
            raise FedHipError(f"unknown compression algorithm {self.algorithm!r}")
        if self.stochastic and self.algorithm != "quantization":
            raise FedHipError("stochastic rounding is an option of algorithm='quantization' "
                              f"(got {self.algorithm!r})")
        if self.stochastic and not 2 <= self.bits <= 16:
            raise FedHipError(f"stochastic quantisation needs bits in [2, 16] (got {self.bits})")
        if self.sparse and self.algorithm != "topk":
            raise FedHipError("sparse payloads are an option of algorithm='topk' "
                              f"(got {self.algorithm!r})")
        if self.packed:
            if self.algorithm != "quantization":
                raise FedHipError("packed payloads are an option of algorithm='quantization' "
                                  f"(got {self.algorithm!r})")
            if self.stochastic:
                raise FedHipError("packed payloads carry the deterministic quantiser's header: "
                                  "stochastic=True is not supported with packed=True")
            if not 1 <= self.bits <= 8:
                raise FedHipError("packed payloads hold uint8 codes: bits must be in [1, 8] "
                                  f"(got {self.bits})")


def topk_k(numel: int, sparsity_ratio: float) -> int:
    """k = int(n * (1 - ratio)), at least 1 (compression.py:255, 333-338)."""
    r = max(0.0, min(1.0, sparsity_ratio))
    k = int(numel * (1 - r))
    return 1 if k == 0 else k


class SegmentPlan:
    """Device-side segment table of one parameter layout: seg_offsets [nseg+1] (int64),
    chunk_offsets [nseg+1] (int32, cumulative chunk counts) and per-ratio k tables."""

    def __init__(self, seg_offsets: Sequence[int], device):
        lib = load()
        self.device = torch.device(device)
        self.chunk = int(lib.fh_compress_chunk_elems())
        offs = [int(o) for o in seg_offsets]
        self.end = offs[-1]  # one past the last element of a row the plan covers
        self.lengths = [b - a for a, b in zip(offs[:-1], offs[1:])]
        if not self.lengths or min(self.lengths) <= 0:
            raise FedHipError("compression needs non-empty segments")
        co = [0]
        for n in self.lengths:
            co.append(co[-1] + -(-n // self.chunk))
        self.nseg, self.nchunks = len(self.lengths), co[-1]
        self.seg_offsets = torch.tensor(offs, dtype=torch.int64, device=self.device)
        self.chunk_offsets = torch.tensor(co, dtype=torch.int32, device=self.device)
        self._k = {}

    def seg_k(self, ratio: float) -> torch.Tensor:
        if ratio not in self._k:
            self._k[ratio] = torch.tensor([topk_k(n, ratio) for n in self.lengths],
                                          dtype=torch.int64, device=self.device)
        return self._k[ratio]


def _cs(t):
    return 0 if t is None else t.stride(0)


def quantize_rows(plan: SegmentPlan, x, nclients, bits=8, symmetric=True, base=None, out=None,
                  codes=None, scale_out=None, zp_out=None):
    """out = base + dequantize(quantize(x - base)) per (client row, segment)."""
    lib = load()
    need = int(lib.fh_quantize_workspace(nclients, plan.nchunks))
    ws = _ws(x.device).get(max(need, 1))
    call("fh_quantize_rows", ptr(x), x.stride(0), ptr(base), _cs(base), ptr(out), _cs(out),
         ptr(codes), _cs(codes), nclients, ptr(plan.seg_offsets), ptr(plan.chunk_offsets),
         plan.nseg, plan.nchunks, int(bits), int(bool(symmetric)), ptr(scale_out), ptr(zp_out),
         ptr(ws), ws.numel(), stream_handle())
    return out


def topk_rows(plan: SegmentPlan, x, nclients, sparsity_ratio=0.9, base=None, out=None,
              keep=None):
    """out = base + topk_dense(x - base) per (client row, segment)."""
    lib = load()
    need = int(lib.fh_topk_workspace(nclients, plan.nseg, plan.nchunks))
    ws = _ws(x.device).get(max(need, 1))
    call("fh_topk_rows", ptr(x), x.stride(0), ptr(base), _cs(base), ptr(out), _cs(out),
         ptr(keep), _cs(keep), nclients, ptr(plan.seg_offsets), ptr(plan.chunk_offsets),
         ptr(plan.seg_k(float(sparsity_ratio))), plan.nseg, plan.nchunks, ptr(ws), ws.numel(),
         stream_handle())
    return out


# ------------------------------------------------------------------ error feedback, stochastic
def _plan_args(plan: SegmentPlan):
    return ptr(plan.seg_offsets), ptr(plan.chunk_offsets), plan.nseg, plan.nchunks


def ef_fold(plan: SegmentPlan, x, resid, nclients, base=None):
    """resid <- (x - base) + resid, the compensated update v (fh_ef_fold)."""
    call("fh_ef_fold", ptr(x), x.stride(0), ptr(base), _cs(base), ptr(resid), resid.stride(0),
         nclients, *_plan_args(plan), stream_handle())
    return resid


def ef_topk_finish(plan: SegmentPlan, keep, resid, x_out, nclients, base=None):
    """With keep = the top-k mask of v = resid: x_out <- base + (keep ? v : 0), resid <- keep ?
    0 : v (fh_ef_topk_finish)."""
    call("fh_ef_topk_finish", ptr(base), _cs(base), ptr(keep), keep.stride(0), ptr(resid),
         resid.stride(0), ptr(x_out), x_out.stride(0), nclients, *_plan_args(plan),
         stream_handle())
    return x_out


def ef_quant_finish(plan: SegmentPlan, c, resid, x_out, nclients, base=None):
    """With c = dequantize(quantize(v)), v = resid: x_out <- base + c, resid <- v - c
    (fh_ef_quant_finish); x_out may be c."""
    call("fh_ef_quant_finish", ptr(base), _cs(base), ptr(c), c.stride(0), ptr(resid),
         resid.stride(0), ptr(x_out), x_out.stride(0), nclients, *_plan_args(plan),
         stream_handle())
    return x_out


def squant_rows(plan: SegmentPlan, x, nclients, bits, symmetric, key, row_ids, base=None,
                resid=None, out=None, codes=None, resid_out=None, scale_out=None, lo_out=None,
                words=None):
    """Stochastic-rounding quantiser (fh_squant_rows): out = base + deq(v) with v = x - base, or
    v = resid when given (the folded residual; x may then be None).  row_ids: int64 global
    client ids; words (uint32 rows) replaces the Philox draw."""
    lib = load()
    dev = (resid if x is None else x).device
    need = int(lib.fh_squant_workspace(nclients, plan.nchunks))
    ws = _ws(dev).get(max(need, 1))
    call("fh_squant_rows", ptr(x), _cs(x), ptr(base), _cs(base), ptr(resid), _cs(resid), ptr(out),
         _cs(out), ptr(codes), _cs(codes), ptr(resid_out), _cs(resid_out), nclients,
         *_plan_args(plan), int(bits), int(bool(symmetric)), int(key) & ((1 << 64) - 1),
         ptr(row_ids), ptr(words), _cs(words), ptr(scale_out), ptr(lo_out), ptr(ws), ws.numel(),
         stream_handle())
    return out


_KEEP: dict = {}


def _keep_scratch(like, nclients):
    """uint8 scratch [nclients, row stride of `like`], one per (device, stream), grow-only:
    the top-k keep mask, or the quantiser's one-byte codes on their way to a packed payload."""
    k = (str(like.device), torch.cuda.current_stream(like.device).cuda_stream)
    n, w = nclients, like.stride(0)
    t = _KEEP.get(k)
    if t is None or t.shape[0] < n or t.shape[1] < w:
        t = _KEEP[k] = torch.empty(n, w, dtype=torch.uint8, device=like.device)
    return t


def compress_rows(plan: SegmentPlan, cfg: CompressionConfig, rows, nclients,
                  base: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                  key: Optional[int] = None, row_ids: Optional[torch.Tensor] = None,
                  words: Optional[torch.Tensor] = None, sparse_out=None,
                  rewrite_rows: bool = True, quant_out=None):
    """In place: rows[:nclients] <- base + decompress(compress(rows - base)).

    cfg.error_feedback: the update compressed is v = (rows - base) + resid and resid
    ([>= nclients, >= P] fp32, updated in place) keeps v - decompress(compress(v)).
    cfg.stochastic: key (the round's Philox key) and row_ids (int64 global client ids) select
    the random words; words (uint32 rows) replaces them.
    sparse_out (a fedhip.sparse.SparseUpdates of this plan at cfg.sparsity_ratio, "topk" only)
    also receives the kept (index, value) pairs of every client.  rewrite_rows=False (with
    sparse_out, without error feedback) then leaves rows as they came: the payload is the
    update.
    quant_out (a fedhip.quantpack.QuantUpdates of this plan at cfg.bits, the deterministic
    "quantization" with bits <= 8 only) receives every client's packed codes, scale, zero point
    and pass-through value in the same way; rewrite_rows=False works as with sparse_out."""
    if quant_out is not None:
        if cfg.algorithm != "quantization":
            raise FedHipError("quant_out= needs algorithm='quantization'")
        if cfg.stochastic:
            raise FedHipError("quant_out= carries the deterministic quantiser's header: "
                              "stochastic=True is not supported")
        if not 1 <= cfg.bits <= 8:
            raise FedHipError(f"quant_out= holds uint8 codes: bits must be in [1, 8] "
                              f"(got {cfg.bits})")
        if quant_out.plan.plan is not plan or quant_out.plan.bits != int(cfg.bits):
            raise FedHipError("quant_out= was laid out for another segment plan or bit width")
        from .quantpack import quant_pack_rows, quant_unpack_rows
        quant_out.symmetric = bool(cfg.symmetric)
    if sparse_out is not None:
        if cfg.algorithm != "topk" or cfg.stochastic:
            raise FedHipError("sparse_out= needs algorithm='topk'")
        if sparse_out.plan.plan is not plan or sparse_out.plan.ratio != float(cfg.sparsity_ratio):
            raise FedHipError("sparse_out= was laid out for another segment plan or ratio")
        from .sparse import sparse_unpack_rows, topk_pack_rows
    if cfg.error_feedback:
        if resid is None:
            raise FedHipError("compression with error_feedback needs the residual rows (resid=)")
        if resid.dtype != torch.float32 or resid.dim() != 2 or resid.shape[0] < nclients \
                or resid.shape[1] < plan.end or resid.stride(1) != 1:
            raise FedHipError("compression: resid must be fp32 [>= nclients, >= P] rows")
    if cfg.stochastic and (key is None or row_ids is None):
        raise FedHipError("stochastic compression needs key= and row_ids=")
    if cfg.stochastic:
        if not cfg.error_feedback:
            return squant_rows(plan, rows, nclients, cfg.bits, cfg.symmetric, key, row_ids,
                               base=base, out=rows, words=words)
        ef_fold(plan, rows, resid, nclients, base=base)
        return squant_rows(plan, None, nclients, cfg.bits, cfg.symmetric, key, row_ids, base=base,
                           resid=resid, out=rows, resid_out=resid, words=words)
    if not cfg.error_feedback:
        if sparse_out is not None:
            keep = _keep_scratch(rows, nclients)
            topk_rows(plan, rows, nclients, cfg.sparsity_ratio, base=base, keep=keep)
            topk_pack_rows(sparse_out, rows, keep, nclients, base=base)
            if rewrite_rows:
                sparse_unpack_rows(sparse_out, rows, nclients, base=base)
            return rows
        if cfg.algorithm == "topk":
            return topk_rows(plan, rows, nclients, cfg.sparsity_ratio, base=base, out=rows)
        if quant_out is not None:
            # the pack reads x - base of a passed-through segment: the rows are rewritten last
            codes = _keep_scratch(rows, nclients)
            quantize_rows(plan, rows, nclients, cfg.bits, cfg.symmetric, base=base, codes=codes,
                          scale_out=quant_out.scale, zp_out=quant_out.zp)
            quant_pack_rows(quant_out, rows, codes, nclients, base=base)
            if rewrite_rows:
                quant_unpack_rows(quant_out, rows, nclients, base=base)
            return rows
        return quantize_rows(plan, rows, nclients, cfg.bits, cfg.symmetric, base=base, out=rows)
    ef_fold(plan, rows, resid, nclients, base=base)
    if cfg.algorithm == "topk":
        keep = _keep_scratch(rows, nclients)
        topk_rows(plan, resid, nclients, cfg.sparsity_ratio, keep=keep)
        if sparse_out is not None:  # before the finish: it clears the kept v from resid
            topk_pack_rows(sparse_out, resid, keep, nclients)
        return ef_topk_finish(plan, keep, resid, rows, nclients, base=base)
    # the rows are rewritten by the finish anyway: they hold c in between
    if quant_out is not None:  # the pack before the finish: it turns resid from v into v - c
        codes = _keep_scratch(rows, nclients)
        quantize_rows(plan, resid, nclients, cfg.bits, cfg.symmetric, out=rows, codes=codes,
                      scale_out=quant_out.scale, zp_out=quant_out.zp)
        quant_pack_rows(quant_out, resid, codes, nclients)
        return ef_quant_finish(plan, rows, resid, rows, nclients, base=base)
    quantize_rows(plan, resid, nclients, cfg.bits, cfg.symmetric, out=rows)
    return ef_quant_finish(plan, rows, resid, rows, nclients, base=base)
