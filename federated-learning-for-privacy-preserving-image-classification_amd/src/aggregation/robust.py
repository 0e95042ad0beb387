"""Byzantine-robust aggregation rules beside FedAvg; the reductions run on HIP.

The reference repository has only the weighted mean (src/aggregation/fedavg.py), which one
poisoned or broken client moves in every coordinate.  These rules replace the FedAvg launch
and nothing else: ``aggregate_updates`` keeps FedAvgAggregator's filtering, truncation,
history and FedAvgError wrapping; only ``_weighted_average`` and ``aggregate_packed`` change.

  TrimmedMeanAggregator  coordinate-wise trimmed mean (Yin et al. 2018)   fh_trimmed_mean_rows
  MedianAggregator       coordinate-wise median (Yin et al. 2018)         fh_trimmed_mean_rows
  KrumAggregator         Krum / multi-Krum (Blanchard et al. 2017)        fh_pairwise_sqdist
                                                                          + fh_fedavg_weighted_sum
  GeometricMedianAggregator  smoothed Weiszfeld / RFA (Pillutla et al. 2022)  fh_center_iter
  CenteredClipAggregator     centered clipping (Karimireddy et al. 2021)      + fh_center_coef
  FLTrustAggregator          trust scores against a server root update        fh_fltrust_rows
                             (Cao et al. 2021); not majority-based

The coordinate-wise rules are unweighted: a sample count is the client's own claim.  The
counts are still recorded in the aggregation history.  The last two rules weight the clients
(sample counts or uniform) and iterate around a centre: every iteration is one fused launch
that reads the rows once and one small launch for the next coefficients, with no host round
trip in between.  Definitions: include/fedhip.h and DESIGN.md §5.
"""
from __future__ import annotations

import logging
import math
from datetime import datetime
from typing import List, Optional, Sequence

import numpy as np
import torch

from fedhip import ops

from ..shared.models import GlobalModel, ModelUpdate, ModelWeights
from .fedavg import FedAvgAggregator, FedAvgError

logger = logging.getLogger(__name__)


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


class _CenterRule(_RowRule):
    """A rule that iterates a weighted sum of the rows around a centre: `iters` times
    (fh_center_iter: the new centre and every client's squared distance to it, the rows read
    once; fh_center_coef: the next coefficients), all on the device.  After the last launch
    the small state is read back once:

      last_coef       the coefficients of the last iteration (what produced the result)
      last_rejected   the positions whose last coefficient is 0 (NaN / Inf rows, weight 0)
      last_objective  sum_k alpha_k * ||x_k - result|| over the live clients
      last_sqdist     device float64 [iters + 1, C]: the squared distances to the start centre
                      and to the centre after every iteration
    """
    uses_center = True
    _rule = None   # ops.CENTER_GEOMED / ops.CENTER_CCLIP
    _mode = None   # ops.CENTER_MEAN / ops.CENTER_DELTA

    def __init__(self, param: float, what: str, iters: int, weighting: str, min_clients: int,
                 max_clients: Optional[int], validate_updates: bool,
                 device: Optional[torch.device]):
        if isinstance(param, bool) or not isinstance(param, (int, float)) \
                or not math.isfinite(param) or param <= 0:
            raise ValueError(f"{what} must be a finite positive number: {param!r}")
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise ValueError(f"iters must be an integer >= 1: {iters!r}")
        if weighting not in ("samples", "uniform"):
            raise ValueError(f"weighting must be 'samples' or 'uniform': {weighting!r}")
        super().__init__(min_clients, max_clients, validate_updates, device)
        self._param, self.iters, self.weighting = float(param), iters, weighting
        self.last_coef: List[float] = []
        self.last_rejected: List[int] = []
        self.last_objective: Optional[float] = None
        self.last_sqdist: Optional[torch.Tensor] = None

    def _alpha(self, num_samples: Sequence[float]) -> List[float]:
        """alpha_k = n_k / sum n in Python double, or 1/C."""
        C = len(num_samples)
        if self.weighting == "uniform":
            return [1.0 / C] * C
        return self._calculate_sample_weights_n(list(num_samples))

    def _start(self, rows, idx, C, P, out, center):
        """Puts the start centre where the first distance pass reads it; returns that tensor."""
        raise NotImplementedError

    def _iterate(self, rows: torch.Tensor, idx: Optional[torch.Tensor], alpha: List[float],
                 out: torch.Tensor, center: Optional[torch.Tensor]) -> torch.Tensor:
        C, P, n, dev = len(alpha), out.numel(), self.iters + 1, rows.device
        if not 1 <= C <= 64:
            raise FedAvgError(f"{type(self).__name__} takes 1..64 clients: {C}")
        if center is not None and (center.numel() != P or center.dtype != torch.float32
                                   or not center.is_contiguous()):
            raise FedAvgError(f"center must be a contiguous float32 vector of {P} elements")
        # one small buffer for everything the host reads back: n states, then n x C coefficients
        S = ops.CENTER_STATE_DOUBLES
        small = torch.zeros(n * S + (n * C + 1) // 2, dtype=torch.float64, device=dev)
        state = small[:n * S].view(n, S)
        coef = small[n * S:].view(torch.float32)[:n * C].view(n, C)
        a64 = torch.tensor(alpha, dtype=torch.float64, device=dev)
        sq = self.last_sqdist = torch.empty(n, C, dtype=torch.float64, device=dev)
        v0 = self._start(rows, idx, C, P, out, center)
        ops.dpfa_row_sqnorm(rows, v0, row_index=idx, P=P, out=sq[0])
        ops.center_coef(sq[0], a64, self._rule, self._param, coef=coef[0], state=state[0])
        for i in range(self.iters):
            ops.center_iter(rows, coef[i], out, self._mode, row_index=idx, P=P, sqdist=sq[i + 1],
                            center=out if self._mode == ops.CENTER_DELTA else None)
            ops.center_coef(sq[i + 1], a64, self._rule, self._param, coef=coef[i + 1],
                            state=state[i + 1])
        host = small.cpu()  # the one read-back
        st = host[:n * S].view(n, S)
        self.last_coef = host[n * S:].view(torch.float32)[:n * C].view(n, C)[n - 2].tolist()
        self.last_rejected = [k for k, c in enumerate(self.last_coef) if c == 0.0]
        self.last_objective = float(st[n - 1, ops.CENTER_OBJECTIVE])
        if float(st[:, ops.CENTER_LIVE].min()) == 0.0:
            raise FedAvgError(f"{type(self).__name__}: no live client (every row is non-finite "
                              f"or has weight 0)")
        return out

    def _reduce_rows(self, rows, idx, idx_host, C, out):
        return self._iterate(rows, idx, self._alpha([1] * C), out, None)

    def _weighted_average(self, updates: List[ModelUpdate], weights: List[float]) -> ModelWeights:
        rows, names, offs, sizes = self._pack_updates(updates)
        out = torch.empty(offs[-1], dtype=torch.float32, device=self.device)
        alpha = list(weights) if self.weighting == "samples" else self._alpha(weights)
        self._iterate(rows, None, alpha, out, None)
        return self._unpack_row(out, updates[0].model_weights, names, offs, sizes)

    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None,
                         center: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rule over client rows already on the device ([clients, >= P] fp32), the clients
        being `row_index` (default: every row, in order), weighted by `num_samples` (or
        uniformly), around `center` (fp32 [P]; `out` may be `center` itself)."""
        C = len(num_samples)
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        idx = None
        if row_index is not None:
            host = [int(i) for i in row_index]
            if len(host) != C:
                raise FedAvgError("row_index and num_samples differ in length")
            idx = torch.tensor(host, dtype=torch.int32, device=packed.device)
        elif packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        if out is None:
            P = center.numel() if center is not None else packed.shape[1]
            out = torch.empty(P, dtype=torch.float32, device=packed.device)
        return self._iterate(packed, idx, self._alpha(num_samples), out, center)

    def _aggregate_around(self, updates: List[ModelUpdate], global_model: GlobalModel,
                          weights: Optional[List[float]]) -> GlobalModel:
        """The reference-style entry point around a global model (shaped like
        FedNovaAggregator.aggregate_updates): the base class's filtering, truncation, weights,
        packing and history, then the rule around `global_model`."""
        name = type(self).__name__
        try:
            t0 = datetime.now()
            self._validate_aggregation_inputs(updates, weights)
            valid = self._filter_and_validate_updates(updates)
            if len(valid) < self.min_clients:
                raise FedAvgError(f"Insufficient valid updates: {len(valid)} < {self.min_clients}")
            if self.max_clients and len(valid) > self.max_clients:
                valid = sorted(valid, key=lambda u: u.num_samples, reverse=True)[:self.max_clients]
            agg_w = self._calculate_sample_weights(valid) if weights is None \
                else self._normalize_weights(weights[:len(valid)])
            alpha = agg_w if weights is not None or self.weighting == "samples" \
                else self._alpha(agg_w)
            rows, names, offs, sizes = self._pack_updates(valid)
            prev = global_model.model_weights
            ref = valid[0].model_weights
            for n in names:
                if n not in prev or prev[n].shape != ref[n].shape:
                    raise FedAvgError(f"global model has no layer {n} of shape "
                                      f"{tuple(ref[n].shape)}")
            g = torch.cat([prev[n].detach().to(device=self.device, dtype=torch.float32)
                           .reshape(-1) for n in names]) if names \
                else torch.empty(0, dtype=torch.float32, device=self.device)
            self._iterate(rows, None, alpha, g, g)
            total = sum(u.num_samples for u in valid)
            avg_loss = sum(u.training_loss * w for u, w in zip(valid, agg_w))
            gm = GlobalModel(round_number=valid[0].round_number,
                             model_weights=self._unpack_row(g, ref, names, offs, sizes),
                             accuracy_metrics={},
                             participating_clients=[u.client_id for u in valid],
                             convergence_score=0.0, created_at=datetime.now())
            self._record_aggregation_stats(valid, agg_w, total, avg_loss,
                                           (datetime.now() - t0).total_seconds())
            return gm
        except Exception as e:
            logger.error(f"{name} aggregation failed: {e}")
            raise FedAvgError(f"{name} aggregation failed: {e}") from e


class GeometricMedianAggregator(_CenterRule):
    """The geometric median argmin_v sum_k alpha_k ||x_k - v|| by `iters` smoothed Weiszfeld
    steps ("RFA", Pillutla, Kakade, Harchaoui 2022):  v <- sum_k b_k x_k / sum_k b_k,
    b_k = alpha_k / max(nu, ||x_k - v||).  Starts from `center` when one is given (RankRound
    passes the previous global model), else from the coordinate-wise median.  Fewer than half
    the total weight in arbitrary rows cannot move the result arbitrarily far; NaN / Inf rows
    get coefficient 0."""
    _rule, _mode = ops.CENTER_GEOMED, ops.CENTER_MEAN

    def __init__(self, nu: float = 1e-6, iters: int = 3, weighting: str = "samples",
                 min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None):
        super().__init__(nu, "nu", iters, weighting, min_clients, max_clients, validate_updates,
                         device)
        self.nu = self._param

    def _start(self, rows, idx, C, P, out, center):
        if center is not None:
            return center
        # no centre: the coordinate-wise median, parked in `out` (MEAN overwrites it later)
        return ops.trimmed_mean_rows(rows, out, (C - 1) // 2, row_index=idx, P=P)


class CenteredClipAggregator(_CenterRule):
    """Centered clipping (Karimireddy, He, Jaggi 2021):  v <- v + sum_k alpha_k (x_k - v)
    min(1, tau / ||x_k - v||), `iters` times, starting from the required `center` (the previous
    global model).  No client moves the centre by more than alpha_k * tau per iteration; NaN /
    Inf rows get coefficient 0.  The paper's client momentum is not part of this rule."""
    _rule, _mode = ops.CENTER_CCLIP, ops.CENTER_DELTA

    def __init__(self, tau: float, iters: int = 1, weighting: str = "uniform",
                 min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None):
        super().__init__(tau, "tau", iters, weighting, min_clients, max_clients,
                         validate_updates, device)
        self.tau = self._param

    def _start(self, rows, idx, C, P, out, center):
        if center is None:
            raise FedAvgError("CenteredClipAggregator needs a centre: pass center= (packed) or "
                              "the global model (aggregate_updates)")
        if out.data_ptr() != center.data_ptr():
            out.copy_(center)  # the iterations run in place on the copy
        return out

    def aggregate_updates(self, updates: List[ModelUpdate], global_model: GlobalModel,
                          weights: Optional[List[float]] = None) -> GlobalModel:
        """Clips the updates around `global_model`; explicit `weights` replace the rule's
        weighting."""
        return self._aggregate_around(updates, global_model, weights)


class FLTrustAggregator(_RowRule):
    """FLTrust (Cao, Fang, Liu, Gong 2021): the server trains on a small clean root shard as a
    client does; client k's delta d_k = x_k - g is scored by ts_k = max(0, cos(d_k, d0)) against
    the server's delta d0 = r - g, rescaled to ||d0|| and averaged with the scores as weights:
    g_new = g + sum_k ts_k (||d0|| / ||d_k||) d_k / sum_k ts_k.  Unlike the rules above it
    judges a row by its direction, not by its position among the other rows, so it holds with a
    malicious majority and against a scaled model-replacement row.  It needs both the global
    model the round started from (`center`) and the server's trained row (`root_row`), which is
    not one of the clients.  The rule ignores sample counts (the paper's Algorithm 2):
    `num_samples` only gives the number of clients and feeds the aggregation history.

    One fh_fltrust_rows call (FLT_STEP), then one small read-back:

      last_trust      the scores ts_k
      last_coef       the fp32 coefficients that produced the result
      last_rejected   the positions whose coefficient is 0 (negative cosine, NaN / Inf rows,
                      a client that did not move)
      last_root_norm  ||d0||
      last_sqdist     device float64 [C]: every client's squared distance to the result
    """
    uses_center = True
    uses_root = True

    def __init__(self, min_clients: int = 1, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None):
        super().__init__(min_clients, max_clients, validate_updates, device)
        self.last_trust: List[float] = []
        self.last_coef: List[float] = []
        self.last_rejected: List[int] = []
        self.last_root_norm: Optional[float] = None
        self.last_sqdist: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None

    def _step(self, rows: torch.Tensor, idx: Optional[torch.Tensor], C: int, root: torch.Tensor,
              center: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        P, dev = out.numel(), rows.device
        if not 1 <= C <= ops.FLT_MAX_CLIENTS:
            raise FedAvgError(f"FLTrustAggregator takes 1..64 clients beside the root: {C}")
        for t, what in ((center, "center"), (root, "root_row")):
            if t.numel() != P or t.dtype != torch.float32 or not t.is_contiguous():
                raise FedAvgError(f"{what} must be a contiguous float32 vector of {P} elements")
        # one small buffer for everything the host reads back: state, trust, then coefficients
        S = ops.FLT_STATE_DOUBLES
        small = torch.zeros(S + C + (C + 1) // 2, dtype=torch.float64, device=dev)
        state, trust = small[:S], small[S:S + C]
        coef = small[S + C:].view(torch.float32)[:C]
        stats = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        need = ops.fltrust_workspace(C, P)
        ws = self._ws
        if need and (ws is None or ws.numel() < need or ws.device != dev):
            ws = self._ws = torch.empty(need, dtype=torch.uint8, device=dev)  # grow-only
        ops.fltrust_rows(rows, root, center, out, ops.FLT_STEP, row_index=idx, P=P, coef=coef,
                         trust=trust, stats=stats, state=state, workspace=ws if need else None)
        self.last_sqdist = ws[:8 * C].view(torch.float64).clone() if need else None
        host = small.cpu()  # the one read-back
        self.last_trust = host[S:S + C].tolist()
        self.last_coef = host[S + C:].view(torch.float32)[:C].tolist()
        self.last_rejected = [k for k, c in enumerate(self.last_coef) if c == 0.0]
        n0 = self.last_root_norm = float(host[ops.FLT_ROOT_NORM])
        if not (math.isfinite(n0) and n0 > 0.0):
            raise FedAvgError(f"FLTrustAggregator: the root update is zero or not finite "
                              f"(norm {n0!r}); the global model is unchanged")
        total = float(host[ops.FLT_SUM])
        if not (math.isfinite(total) and total > 0.0):
            raise FedAvgError(f"FLTrustAggregator: no client is trusted (every cosine with the "
                              f"root update is <= 0 or its row is non-finite; sum of scores "
                              f"{total!r}); the global model is unchanged")
        return out

    def _reduce_rows(self, rows, idx, idx_host, C, out):
        raise FedAvgError("FLTrustAggregator needs the global model and the server's root "
                          "update: pass center= and root_row= (packed) or global_model and "
                          "server_update (aggregate_updates)")

    def _weighted_average(self, updates: List[ModelUpdate], weights: List[float]) -> ModelWeights:
        return self._reduce_rows(None, None, None, len(updates), None)  # never a plain FedAvg

    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None,
                         center: Optional[torch.Tensor] = None,
                         root_row=None) -> torch.Tensor:
        """FLTrust over client rows already on the device ([rows, >= P] fp32), the clients being
        `row_index` (default: every row, in order), around `center` (fp32 [P], the global model
        the round started from; `out` may be `center` itself).  `root_row` is the server's
        trained row: a row number of `packed` (not one of the clients') or an fp32 [P] device
        tensor.  `num_samples` only gives the number of clients: the rule does not weight by
        it."""
        C = len(num_samples)
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        if center is None or root_row is None:
            missing = " and ".join(n for n, v in (("center (the global model)", center),
                                                  ("root_row (the server's trained row)",
                                                   root_row)) if v is None)
            raise FedAvgError(f"FLTrustAggregator needs {missing}")
        P = center.numel()
        idx = host = None
        if row_index is not None:
            host = [int(i) for i in row_index]
            if len(host) != C:
                raise FedAvgError("row_index and num_samples differ in length")
            idx = torch.tensor(host, dtype=torch.int32, device=packed.device)
        if isinstance(root_row, torch.Tensor):
            root = root_row
            if root.dim() == 1 and root.numel() > P and root.is_contiguous():
                root = root[:P]
        else:
            r = int(root_row)
            if not 0 <= r < packed.shape[0]:
                raise FedAvgError(f"root_row={r} is not a row of the {packed.shape[0]}-row matrix")
            if r in (host if host is not None else range(C)):
                raise FedAvgError(f"root_row={r} is one of the clients: the server's row is the "
                                  f"reference direction and is left out of the sum")
            root = packed[r, :P]
        if row_index is None and packed.shape[0] != C:
            if isinstance(root_row, torch.Tensor) or packed.shape[0] < C:
                raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
            # the root is a later row of the matrix: the clients are rows 0..C-1, by name
            idx = torch.arange(C, dtype=torch.int32, device=packed.device)
        if out is None:
            out = torch.empty(P, dtype=torch.float32, device=packed.device)
        return self._step(packed, idx, C, root, center, out)

    def aggregate_updates(self, updates: List[ModelUpdate], global_model: GlobalModel = None,
                          server_update=None, weights: Optional[List[float]] = None) -> GlobalModel:
        """The reference-style entry point: the base class's filtering, truncation, packing and
        history, then FLTrust around `global_model` with `server_update` (a ModelUpdate, or a
        weights mapping with the global model's layers) as the root.  The rule defines its own
        weights: passing `weights=` raises, and sample counts only feed the history."""
        name = type(self).__name__
        try:
            t0 = datetime.now()
            if weights is not None:
                raise FedAvgError("FLTrust defines its own weights (the trust scores): weights= "
                                  "is not accepted")
            if not isinstance(global_model, GlobalModel) or server_update is None:
                missing = " and ".join(
                    n for n, ok in (("global_model (the GlobalModel the round started from)",
                                     isinstance(global_model, GlobalModel)),
                                    ("server_update (the server's update on its root data)",
                                     server_update is not None)) if not ok)
                raise FedAvgError(f"FLTrust needs {missing}; it does not fall back to FedAvg")
            self._validate_aggregation_inputs(updates, None)
            valid = self._filter_and_validate_updates(updates)
            if len(valid) < self.min_clients:
                raise FedAvgError(f"Insufficient valid updates: {len(valid)} < {self.min_clients}")
            if self.max_clients and len(valid) > self.max_clients:
                valid = sorted(valid, key=lambda u: u.num_samples, reverse=True)[:self.max_clients]
            agg_w = self._calculate_sample_weights(valid)  # the history's, not the rule's
            rows, names, offs, sizes = self._pack_updates(valid)
            prev = global_model.model_weights
            root_w = server_update.model_weights if isinstance(server_update, ModelUpdate) \
                else server_update
            ref = valid[0].model_weights
            for what, w in (("global model", prev), ("server update", root_w)):
                for n in names:
                    if n not in w or w[n].shape != ref[n].shape:
                        raise FedAvgError(f"{what} has no layer {n} of shape "
                                          f"{tuple(ref[n].shape)}")

            def flat(w):
                return torch.cat([w[n].detach().to(device=self.device, dtype=torch.float32)
                                  .reshape(-1) for n in names]) if names \
                    else torch.empty(0, dtype=torch.float32, device=self.device)
            g, root = flat(prev), flat(root_w)
            self._step(rows, None, len(valid), root, g, g)
            total = sum(u.num_samples for u in valid)
            avg_loss = sum(u.training_loss * w for u, w in zip(valid, agg_w))
            gm = GlobalModel(round_number=valid[0].round_number,
                             model_weights=self._unpack_row(g, ref, names, offs, sizes),
                             accuracy_metrics={},
                             participating_clients=[u.client_id for u in valid],
                             convergence_score=0.0, created_at=datetime.now())
            self._record_aggregation_stats(valid, agg_w, total, avg_loss,
                                           (datetime.now() - t0).total_seconds())
            return gm
        except Exception as e:
            logger.error(f"{name} aggregation failed: {e}")
            raise FedAvgError(f"{name} aggregation failed: {e}") from e


def create_robust_aggregator(kind: str, **kwargs) -> FedAvgAggregator:
    """"trimmed_mean" | "median" | "krum" (one client kept) | "multi_krum" (n - f kept) |
    "geometric_median" | "centered_clip" | "fltrust"."""
    if kind == "fltrust":
        return FLTrustAggregator(**kwargs)
    if kind == "geometric_median":
        return GeometricMedianAggregator(**kwargs)
    if kind == "centered_clip":
        return CenteredClipAggregator(**kwargs)
    if kind == "trimmed_mean":
        return TrimmedMeanAggregator(**kwargs)
    if kind == "median":
        return MedianAggregator(**kwargs)
    if kind == "krum":
        return KrumAggregator(num_selected=1, **kwargs)
    if kind == "multi_krum":
        return KrumAggregator(**kwargs)
    raise ValueError(f"unknown robust aggregator: {kind!r}")
