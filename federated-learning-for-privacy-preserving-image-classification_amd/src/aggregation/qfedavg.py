"""q-FedAvg beside FedAvg: fairness-aware aggregation (Li, Sanjabi, Beirami, Smith, "Fair
Resource Allocation in Federated Learning", ICLR 2020, Algorithm 2); the sums run on HIP.

FedAvg minimises the sample-weighted mean loss, so with heterogeneous shards a few clients are
left far behind the average.  q-FFL minimises sum_k pi_k * F_k^(q+1) / (q+1) instead; its
q-FedAvg solver reweights every client's delta by a power of its loss and divides by a
Lipschitz-style normaliser, so the step size needs no retuning when q changes.  With the global
model g the clients started from, client k's trained model x_k, its weight pi_k and its loss F_k:

    a_k = pi_k * F_k^q                     b_k = pi_k * q * L * F_k^(q-1)
    den = sum_k ( b_k * ||x_k - g||^2 + a_k )
    g_new = g + (1/den) * sum_k a_k * (x_k - g)

which is Algorithm 2 with one L cancelled from the numerator and the denominator.  q = 0 with
the sample weights is FedAvg written in delta form; a larger q shifts weight to the clients with
a high loss.  L estimates the Lipschitz constant of the gradient; the paper uses 1/lr, the
inverse of the clients' learning rate.  pi_k is uniform (1/m) by default, as in the paper, or the
FedAvg sample weights.  The coefficients are host bookkeeping (fedhip.ops.qfedavg_coefficients);
the exact arithmetic is fh_qfedavg_rows' (include/fedhip.h): the client rows are
read once and den never leaves the device.

F_k is the client's loss at g in the paper.  ``aggregate_updates`` defaults to each update's
``training_loss`` (what the reference's ModelUpdate carries), which is a proxy; pass ``losses=``
to use the exact quantity.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from datetime import datetime
from typing import List, Mapping, Optional, Sequence, Union

import torch

from fedhip import ops

from ..shared.models import GlobalModel, ModelUpdate
from .fedavg import FedAvgAggregator, FedAvgError

logger = logging.getLogger(__name__)


@dataclass
class QFedAvgConfig:
    """q >= 0: the fairness exponent (0: no reweighting).  lipschitz: L > 0, or None for 1/lr of
    the round (RankRound) / a per-call value (the aggregator).  weights: "uniform" (pi_k = 1/m,
    the paper's) or "samples" (the FedAvg weights n_k / sum n)."""
    q: float = 1.0
    lipschitz: Optional[float] = None
    weights: str = "uniform"

    def __post_init__(self):
        if self.weights not in ("uniform", "samples"):
            raise ValueError(f"qfedavg: weights must be 'uniform' or 'samples': {self.weights!r}")
        # a bad q or lipschitz is refused here, not in round one
        ops.qfedavg_coefficients([1.0], [1.0], self.q,
                                 1.0 if self.lipschitz is None else self.lipschitz)


class QFedAvgAggregator(FedAvgAggregator):
    def __init__(self, min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None,
                 q: float = 1.0, weights: str = "uniform", keep_stats: bool = False):
        super().__init__(min_clients, max_clients, validate_updates, device)
        try:
            self.config = QFedAvgConfig(q=q, weights=weights)
        except ValueError as e:
            raise FedAvgError(str(e)) from e
        self.q, self.weights = q, weights
        # last_den / last_sqdist cost a device read: filled only on request
        self.keep_stats = bool(keep_stats)
        self.last_den: Optional[float] = None
        self.last_sqdist: Optional[List[float]] = None

    def _pi(self, sample_weights: Sequence[float]) -> List[float]:
        m = len(sample_weights)
        return [1.0 / m] * m if self.weights == "uniform" else list(sample_weights)

    def _coefficients(self, pi, losses, lipschitz):
        try:
            return ops.qfedavg_coefficients(pi, losses, self.q, lipschitz)
        except ValueError as e:
            raise FedAvgError(str(e)) from e

    def _step(self, rows, a, b, g, out, idx, P):
        dev = rows.device
        a32 = torch.tensor(a, dtype=torch.float32, device=dev)
        b64 = torch.tensor(b, dtype=torch.float64, device=dev)
        _, sqdist, state = ops.qfedavg_rows(rows, a32, b64, g, out, ops.QFA_STEP, row_index=idx,
                                            P=P)
        if self.keep_stats:
            self.last_den = float(state[ops.QFA_DEN].item())
            self.last_sqdist = sqdist.tolist()
        return out

    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         losses: Sequence[float], global_flat: torch.Tensor, lipschitz: float,
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q-FedAvg of client rows already on the device ([clients, >= P] fp32) around
        global_flat (fp32 [P]): one STEP.  Rows are summed in the order of `row_index`
        (default: row order); `out` may be global_flat itself."""
        C = len(num_samples)
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        if len(losses) != C:
            raise FedAvgError(f"{len(losses)} losses for {C} clients")
        if row_index is not None and len(row_index) != C:
            raise FedAvgError("row_index and num_samples differ in length")
        if row_index is None and packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        pi = self._pi(self._calculate_sample_weights_n(list(num_samples)))
        a, b = self._coefficients(pi, losses, lipschitz)
        dev = packed.device
        idx = None if row_index is None else torch.tensor([int(i) for i in row_index],
                                                          dtype=torch.int32, device=dev)
        P = global_flat.numel()
        if out is None:
            out = torch.empty(P, dtype=torch.float32, device=dev)
        return self._step(packed, a, b, global_flat, out, idx, P)

    def aggregate_updates(self, updates: List[ModelUpdate], global_model: GlobalModel,
                          lipschitz: float,
                          losses: Union[Mapping[str, float], Sequence[float], None] = None,
                          weights: Optional[List[float]] = None) -> GlobalModel:
        """The reference-style entry point: the base class's filtering, truncation, weights,
        packing and history, then one q-FedAvg STEP around `global_model`.  `losses` maps
        client_id to the client's loss F_k, or lists the losses in the order of `updates`;
        by default each update's ``training_loss`` stands in.  `weights` replaces pi_k."""
        try:
            t0 = datetime.now()
            self._validate_aggregation_inputs(updates, weights)
            if losses is None:
                loss_of = {id(u): u.training_loss for u in updates}
            elif isinstance(losses, Mapping):
                missing = [u.client_id for u in updates if u.client_id not in losses]
                if missing:
                    raise FedAvgError(f"no loss for clients {missing}")
                loss_of = {id(u): losses[u.client_id] for u in updates}
            else:
                if len(losses) != len(updates):
                    raise FedAvgError("Number of losses must match number of updates")
                loss_of = {id(u): x for u, x in zip(updates, losses)}
            valid = self._filter_and_validate_updates(updates)
            if len(valid) < self.min_clients:
                raise FedAvgError(f"Insufficient valid updates: {len(valid)} < {self.min_clients}")
            if self.max_clients and len(valid) > self.max_clients:
                valid = sorted(valid, key=lambda u: u.num_samples, reverse=True)[:self.max_clients]
            sample_w = self._calculate_sample_weights(valid)
            pi = self._pi(sample_w) if weights is None \
                else self._normalize_weights(weights[:len(valid)])
            a, b = self._coefficients(pi, [loss_of[id(u)] for u in valid], lipschitz)
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
            self._step(rows, a, b, g, g, None, g.numel())
            total = sum(u.num_samples for u in valid)
            avg_loss = sum(u.training_loss * w for u, w in zip(valid, sample_w))
            gm = GlobalModel(round_number=valid[0].round_number,
                             model_weights=self._unpack_row(g, ref, names, offs, sizes),
                             accuracy_metrics={},
                             participating_clients=[u.client_id for u in valid],
                             convergence_score=0.0, created_at=datetime.now())
            self._record_aggregation_stats(valid, pi, total, avg_loss,
                                           (datetime.now() - t0).total_seconds())
            return gm
        except Exception as e:
            logger.error(f"q-FedAvg aggregation failed: {e}")
            raise FedAvgError(f"q-FedAvg aggregation failed: {e}") from e
