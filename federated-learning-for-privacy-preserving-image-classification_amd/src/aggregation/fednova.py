"""FedNova beside FedAvg: normalised averaging for uneven local step counts (Wang et al.,
"Tackling the Objective Inconsistency Problem in Heterogeneous Federated Optimization",
NeurIPS 2020); the sum runs on HIP.

FedAvg averages the trained models with sample-count weights p_k only.  When the clients run
different numbers of local steps a_k, that average converges to a stationary point of a
mismatched objective: the clients with many steps pull the global model toward their own
optima.  FedNova divides every client's delta by its step count and rescales the average:

    x_new = g + tau_eff * sum_k (p_k / a_k) * (x_k - g),        tau_eff = sum_k p_k * a_k

With all a_k equal this is FedAvg.  The coefficients are host bookkeeping
(fedhip.ops.fednova_coefficients); the exact fp32 arithmetic is fh_fednova_rows'
(include/fedhip.h).  The step counts come from the coordinator: the reference's
ModelUpdate record has no step field and keeps none here, so ``aggregate_updates`` takes them
beside the updates.  The a_k are the plain step counts (the paper's vanilla-SGD normaliser);
for momentum or Adam clients they are used as is.
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
class FedNovaConfig:
    """tau_eff: "weighted" (sum_k p_k * a_k, the paper's choice) or a finite positive number."""
    tau_eff: Union[str, float] = "weighted"


class FedNovaAggregator(FedAvgAggregator):
    def __init__(self, min_clients: int = 2, max_clients: Optional[int] = None,
                 validate_updates: bool = True, device: Optional[torch.device] = None,
                 tau_eff: Union[str, float] = "weighted"):
        super().__init__(min_clients, max_clients, validate_updates, device)
        ops.fednova_coefficients([1.0], [1], tau_eff)  # a bad tau_eff is refused here
        self.tau_eff = tau_eff

    def _coefficients(self, weights, local_steps):
        try:
            return ops.fednova_coefficients(weights, local_steps, self.tau_eff)
        except ValueError as e:
            raise FedAvgError(str(e)) from e

    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         local_steps: Sequence[int], global_flat: torch.Tensor,
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """FedNova of client rows already on the device ([clients, >= P] fp32) around
        global_flat (fp32 [P]): one launch.  Rows are summed in the order of `row_index`
        (default: row order); `out` may be global_flat itself."""
        C = len(num_samples)
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        if len(local_steps) != C:
            raise FedAvgError(f"{len(local_steps)} local step counts for {C} clients")
        if row_index is not None and len(row_index) != C:
            raise FedAvgError("row_index and num_samples differ in length")
        if row_index is None and packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        w = self._calculate_sample_weights_n(list(num_samples))
        coef, tau = self._coefficients(w, local_steps)
        dev = packed.device
        c32 = torch.tensor(coef, dtype=torch.float32, device=dev)
        idx = None if row_index is None else torch.tensor([int(i) for i in row_index],
                                                          dtype=torch.int32, device=dev)
        P = global_flat.numel()
        if out is None:
            out = torch.empty(P, dtype=torch.float32, device=dev)
        return ops.fednova_rows(packed, c32, global_flat, out, tau, ops.NOVA_STEP,
                                row_index=idx, P=P)

    def aggregate_updates(self, updates: List[ModelUpdate], global_model: GlobalModel,
                          local_steps: Union[Mapping[str, int], Sequence[int]],
                          weights: Optional[List[float]] = None) -> GlobalModel:
        """The reference-style entry point: the base class's filtering, truncation, weights,
        packing and history, then one FedNova launch around `global_model`.  `local_steps`
        maps client_id to the client's local step count, or lists the counts in the order
        of `updates`."""
        try:
            t0 = datetime.now()
            self._validate_aggregation_inputs(updates, weights)
            if isinstance(local_steps, Mapping):
                missing = [u.client_id for u in updates if u.client_id not in local_steps]
                if missing:
                    raise FedAvgError(f"no local step count for clients {missing}")
                steps_of = {id(u): local_steps[u.client_id] for u in updates}
            else:
                if len(local_steps) != len(updates):
                    raise FedAvgError("Number of local step counts must match number of "
                                      "updates")
                steps_of = {id(u): s for u, s in zip(updates, local_steps)}
            valid = self._filter_and_validate_updates(updates)
            if len(valid) < self.min_clients:
                raise FedAvgError(f"Insufficient valid updates: {len(valid)} < {self.min_clients}")
            if self.max_clients and len(valid) > self.max_clients:
                valid = sorted(valid, key=lambda u: u.num_samples, reverse=True)[:self.max_clients]
            agg_w = self._calculate_sample_weights(valid) if weights is None \
                else self._normalize_weights(weights[:len(valid)])
            coef, tau = self._coefficients(agg_w, [steps_of[id(u)] for u in valid])
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
            c32 = torch.tensor(coef, dtype=torch.float32, device=self.device)
            ops.fednova_rows(rows, c32, g, g, tau, ops.NOVA_STEP)
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
            logger.error(f"FedNova aggregation failed: {e}")
            raise FedAvgError(f"FedNova aggregation failed: {e}") from e
