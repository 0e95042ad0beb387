"""Byzantine-robust aggregation rules beside FedAvg; the reductions run on HIP.

The reference repository has only the weighted mean (src/aggregation/fedavg.py), which one
poisoned or broken client moves in every coordinate.  These rules replace the FedAvg launch
and nothing else: ``aggregate_updates`` keeps FedAvgAggregator's filtering, truncation,
history and FedAvgError wrapping; only ``_weighted_average`` and ``aggregate_packed`` change.

  TrimmedMeanAggregator  coordinate-wise trimmed mean (Yin et al. 2018)   fh_trimmed_mean_rows
  MedianAggregator       coordinate-wise median (Yin et al. 2018)         fh_trimmed_mean_rows
  KrumAggregator         Krum / multi-Krum (Blanchard et al. 2017)        fh_pairwise_sqdist
                                                                          + fh_fedavg_weighted_sum

The coordinate-wise rules are unweighted: a sample count is the client's own claim.  The
counts are still recorded in the aggregation history.  Definitions: include/fedhip.h and
DESIGN.md §5.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from fedhip import ops

from ..shared.models import ModelUpdate, ModelWeights
from .fedavg import FedAvgAggregator, FedAvgError

def trim_count(trim_ratio: float, num_clients: int) -> int:
    """Rows dropped per side: floor(trim_ratio * C)."""
    return int(math.floor(trim_ratio * num_clients))


def krum_scores(dist: np.ndarray, num_byzantine: int) -> List[float]:
    """score_i = sum (fp64, ascending order) of the n - f - 2 smallest dist[i][k], k != i."""
    dist = np.asarray(dist, dtype=np.float64)
    n, f = dist.shape[0], int(num_byzantine)
    if f < 0 or n < 2 * f + 3:
        raise FedAvgError(f"Krum needs n >= 2f + 3 clients: n={n}, f={f}")
    scores = []
    for i in range(n):
        d = np.sort(np.delete(dist[i], i))  # NaN sorts last
        s = 0.0
        for x in d[:n - f - 2]:
            s += float(x)
        scores.append(s)
    return scores


def lowest_scores(scores: Sequence[float], num_selected: int) -> List[int]:
    """The `num_selected` positions with the lowest score, ties to the lowest index; returned
    in ascending order.  A NaN score ranks last."""
    n = len(scores)
    if not 1 <= num_selected <= n:
        raise FedAvgError(f"Krum cannot select {num_selected} of {n} clients")
    order = sorted(range(n), key=lambda i: (scores[i] if scores[i] == scores[i] else math.inf, i))
    return sorted(order[:num_selected])


def krum_select(dist: np.ndarray, num_byzantine: int, num_selected: int) -> List[int]:
    """Rows kept by (multi-)Krum on the [n, n] squared-distance matrix, ascending."""
    return lowest_scores(krum_scores(dist, num_byzantine), num_selected)


class _RowRule(FedAvgAggregator):
    """A rule that reduces packed client rows [C, P] to one row on the device."""

    def _reduce_rows(self, rows: torch.Tensor, idx: Optional[torch.Tensor],
                     idx_host: Optional[List[int]], C: int, out: torch.Tensor) -> torch.Tensor:
        """out = the rule over the C rows rows[idx] (idx: device int32, idx_host: the same on
        the host; both None = rows 0..C-1)."""
        raise NotImplementedError

    def _weighted_average(self, updates: List[ModelUpdate], weights: List[float]) -> ModelWeights:
        rows, names, offs, sizes = self._pack_updates(updates)
        out = torch.empty(offs[-1], dtype=torch.float32, device=self.device)
        self._reduce_rows(rows, None, None, len(updates), out)
        return self._unpack_row(out, updates[0].model_weights, names, offs, sizes)

    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rule over client rows already on the device ([clients, P] fp32), the clients
        being `row_index` (default: every row, in order).  `num_samples` only gives the
        number of clients: the rules do not weight by it."""
        C = len(num_samples)
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        idx = host = None
        if row_index is not None:
            host = [int(i) for i in row_index]
            if len(host) != C:
                raise FedAvgError("row_index and num_samples differ in length")
            idx = torch.tensor(host, dtype=torch.int32, device=packed.device)
        elif packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        if out is None:
            out = torch.empty(packed.shape[1], dtype=torch.float32, device=packed.device)
        return self._reduce_rows(packed, idx, host, C, out)


class TrimmedMeanAggregator(_RowRule):
    """Per coordinate: drop the floor(trim_ratio * C) smallest and as many largest values,
    average the rest.  Up to that many NaN / Inf / arbitrarily scaled rows per coordinate
    have no effect on the result beyond which honest values are dropped with them."""

    def __init__(self, trim_ratio: float = 0.1, min_clients: int = 2,
                 max_clients: Optional[int] = None, validate_updates: bool = True,
                 device: Optional[torch.device] = None):
        if not 0.0 <= trim_ratio < 0.5:
            raise ValueError(f"trim_ratio must be in [0, 0.5): {trim_ratio}")
        super().__init__(min_clients, max_clients, validate_updates, device)
        self.trim_ratio = float(trim_ratio)

    def _trim(self, C: int) -> int:
        return trim_count(self.trim_ratio, C)

    def _reduce_rows(self, rows, idx, idx_host, C, out):
        return ops.trimmed_mean_rows(rows, out, self._trim(C), row_index=idx, P=out.numel())


class MedianAggregator(TrimmedMeanAggregator):
    """Coordinate-wise median: the trimmed mean with (C - 1) // 2 rows dropped per side (the
    middle value for odd C, the fp32 mean of the two middle values for even C)."""

    def __init__(self, min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None):
        super().__init__(0.0, min_clients, max_clients, validate_updates, device)

    def _trim(self, C: int) -> int:
        return (C - 1) // 2


class KrumAggregator(_RowRule):
    """Krum (num_selected = 1) and multi-Krum (default num_selected = n - f): score every
    client by the summed squared distance to its n - f - 2 nearest neighbours, keep the
    lowest-scoring ones and average them with weight fl32(1/m) each, in ascending row order,
    by the FedAvg kernel.  `last_selected` holds the kept positions of the last call."""

    def __init__(self, num_byzantine: int, num_selected: Optional[int] = None,
                 min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None):
        if num_byzantine < 0:
            raise ValueError(f"num_byzantine must be >= 0: {num_byzantine}")
        if num_selected is not None and num_selected < 1:
            raise ValueError(f"num_selected must be >= 1: {num_selected}")
        super().__init__(min_clients, max_clients, validate_updates, device)
        self.num_byzantine, self.num_selected = int(num_byzantine), num_selected
        self.last_selected: List[int] = []
        self.last_scores: List[float] = []

    def _reduce_rows(self, rows, idx, idx_host, C, out):
        f = self.num_byzantine
        if C < 2 * f + 3:
            raise FedAvgError(f"Krum needs n >= 2f + 3 clients: n={C}, f={f}")
        m = C - f if self.num_selected is None else self.num_selected
        P = out.numel()
        dist = ops.pairwise_sqdist(rows, row_index=idx, P=P).cpu().numpy()  # 8*C*C bytes
        self.last_scores = krum_scores(dist, f)
        sel = self.last_selected = lowest_scores(self.last_scores, m)
        src = sel if idx_host is None else [idx_host[i] for i in sel]
        sel_idx = torch.tensor(src, dtype=torch.int32, device=rows.device)
        w32 = torch.full((m,), 1.0 / m, dtype=torch.float32, device=rows.device)
        return ops.fedavg_weighted_sum(rows, w32, out, row_index=sel_idx, P=P)


def create_robust_aggregator(kind: str, **kwargs) -> FedAvgAggregator:
    """"trimmed_mean" | "median" | "krum" (one client kept) | "multi_krum" (n - f kept)."""
    if kind == "trimmed_mean":
        return TrimmedMeanAggregator(**kwargs)
    if kind == "median":
        return MedianAggregator(**kwargs)
    if kind == "krum":
        return KrumAggregator(num_selected=1, **kwargs)
    if kind == "multi_krum":
        return KrumAggregator(**kwargs)
    raise ValueError(f"unknown robust aggregator: {kind!r}")
