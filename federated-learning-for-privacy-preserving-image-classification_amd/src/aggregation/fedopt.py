"""Adaptive server optimizers beside FedAvg: FedAvgM, FedAdagrad, FedAdam, FedYogi (Reddi et
al., "Adaptive Federated Optimization", ICLR 2021); the step runs on HIP.

The reference repository, and every aggregation rule here, assigns the aggregate to the global
model.  A ServerOptimizer instead treats  d = aggregate - global  as a pseudo-gradient and steps
the global model with first and second moments it keeps across rounds:

  FedAvgM     m' = b1*m + d                              g' = g + lr*m'
  FedAdagrad  m' = b1*m + (1-b1)*d   v' = v + d^2        g' = g + lr*m'/(sqrt(v') + tau)
  FedAdam     ...                    v' = b2*v + (1-b2)*d^2
  FedYogi     ...                    v' = v - (1-b2)*d^2*sign(v - d^2)

with no bias correction (the paper uses none) and the state m = 0, v = tau^2 before the first
round.  The exact fp32 arithmetic is fh_server_opt_step's (include/fedhip.h).

Whatever produced the aggregate is the `base` aggregator's business: the plain FedAvg (then
``step_packed`` is ONE launch that forms the weighted sum in registers and steps from it), a
robust rule of src.aggregation.robust (its ``aggregate_packed`` into a scratch vector, then a
single-row step), or nothing at all (``step_vector`` on an aggregate that already exists: an
all-reduce, secure.py's decode).  The client side is untouched.
"""
from __future__ import annotations

import logging
import math
from datetime import datetime
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from fedhip import ops

from ..shared.models import GlobalModel, ModelUpdate
from .fedavg import FedAvgAggregator, FedAvgError

logger = logging.getLogger(__name__)

RULES = {"fedavgm": ops.SOPT_MOMENTUM, "fedadagrad": ops.SOPT_ADAGRAD,
         "fedadam": ops.SOPT_ADAM, "fedyogi": ops.SOPT_YOGI}
_SCALARS = ("server_lr", "beta1", "beta2", "tau")


def _rule_id(rule) -> int:
    if isinstance(rule, str):
        if rule not in RULES:
            raise ValueError(f"unknown server optimizer: {rule!r}")
        return RULES[rule]
    if isinstance(rule, bool) or not isinstance(rule, (int, np.integer)) \
            or int(rule) not in RULES.values():
        raise ValueError(f"server optimizer rule must be one of {sorted(RULES)} or 0..3: "
                         f"{rule!r}")
    return int(rule)


def _fp32_scalars(server_lr, beta1, beta2, tau) -> Dict[str, float]:
    """The four scalars rounded to fp32 once (the kernel's arguments are fp32)."""
    out = {}
    for name, x in zip(_SCALARS, (server_lr, beta1, beta2, tau)):
        with np.errstate(over="ignore"):
            y = float(np.float32(x))
        if not math.isfinite(y):
            raise ValueError(f"{name} must be finite in fp32: {x!r}")
        out[name] = y
    if out["tau"] < 0:
        raise ValueError(f"tau must be >= 0: {tau!r}")
    return out


class ServerOptimizer:
    """One adaptive server optimizer and its state (m, v: fp32 [P] on the device, allocated
    for the first P seen)."""

    def __init__(self, rule, server_lr: float, beta1: float = 0.9, beta2: float = 0.99,
                 tau: float = 1e-3, base: Optional[FedAvgAggregator] = None,
                 device: Optional[torch.device] = None):
        self.rule = _rule_id(rule)
        for name, x in _fp32_scalars(server_lr, beta1, beta2, tau).items():
            setattr(self, name, x)
        if base is not None and not isinstance(base, FedAvgAggregator):
            raise ValueError(f"base must be a FedAvgAggregator: {type(base).__name__}")
        if base is None:
            base = FedAvgAggregator(device=device)
        self.base = base
        self.device = torch.device(device) if device is not None else base.device
        self.m: Optional[torch.Tensor] = None
        self.v: Optional[torch.Tensor] = None
        self._scratch: Optional[torch.Tensor] = None

    @property
    def plain_base(self) -> bool:
        """True when the base's packed aggregate is the plain weighted sum, which the step
        kernel forms itself (one launch)."""
        return type(self.base).aggregate_packed is FedAvgAggregator.aggregate_packed

    # ------------------------------------------------------------------ state
    def _state(self, P: int, device):
        if self.m is None:
            self.m = torch.zeros(P, dtype=torch.float32, device=device)
            if self.rule != ops.SOPT_MOMENTUM:
                tau32 = np.float32(self.tau)
                self.v = torch.full((P,), float(tau32 * tau32), dtype=torch.float32,
                                    device=device)
        if self.m.numel() != P:
            raise FedAvgError(f"server optimizer state holds {self.m.numel()} parameters, the "
                              f"model has {P}; reset() starts over")
        return self.m, self.v

    def reset(self):
        self.m = self.v = self._scratch = None

    def state_dict(self) -> Dict[str, Any]:
        d: Dict[str, Any] = {"rule": self.rule}
        d.update({name: getattr(self, name) for name in _SCALARS})
        d["m"] = None if self.m is None else self.m.detach().clone()
        d["v"] = None if self.v is None else self.v.detach().clone()
        return d

    def load_state_dict(self, state: Dict[str, Any]):
        missing = [k for k in ("rule", "m", "v") + _SCALARS if k not in state]
        if missing:
            raise FedAvgError(f"server optimizer state lacks {missing}")
        try:
            rule = _rule_id(state["rule"])
            scalars = _fp32_scalars(*(state[k] for k in _SCALARS))
        except (ValueError, TypeError) as e:
            raise FedAvgError(f"bad server optimizer state: {e}") from e
        m, v = state["m"], state["v"]
        need_v = rule != ops.SOPT_MOMENTUM
        if m is None:
            if v is not None:
                raise FedAvgError("server optimizer state has v but no m")
        else:
            if need_v and v is None:
                raise FedAvgError("server optimizer state has m but no v")
            for t, what in ((m, "m"), (v, "v")):
                if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 1
                                      or t.dtype != torch.float32 or t.shape != m.shape):
                    raise FedAvgError(f"server optimizer state: {what} must be a float32 "
                                      f"vector of m's length")
        self.rule = rule
        for name, x in scalars.items():
            setattr(self, name, x)
        self._scratch = None
        self.m = None if m is None else m.detach().to(self.device).clone().contiguous()
        self.v = None if (v is None or not need_v or m is None) \
            else v.detach().to(self.device).clone().contiguous()

    # ------------------------------------------------------------------ steps
    def _step(self, rows, global_flat, w32, idx):
        P = global_flat.numel()
        m, v = self._state(P, global_flat.device)
        return ops.server_opt_step(rows, global_flat, m, v, self.rule, self.server_lr, self.beta1,
                                   self.beta2, self.tau, weights_f32=w32, row_index=idx, P=P)

    def step_rows(self, packed: torch.Tensor, w32: torch.Tensor, global_flat: torch.Tensor,
                  row_index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fused launch on device-resident arguments: global_flat steps from the weighted
        sum of packed[row_index] with the fp32 weights w32 (row_index: device int32)."""
        return self._step(packed, global_flat, w32, row_index)

    def step_vector(self, aggregate: torch.Tensor, global_flat: torch.Tensor) -> torch.Tensor:
        """global_flat steps from an aggregate that already exists (fp32 [P])."""
        if aggregate.dim() != 1 or aggregate.numel() < global_flat.numel():
            raise FedAvgError(f"aggregate of shape {tuple(aggregate.shape)} for "
                              f"{global_flat.numel()} parameters")
        return self._step(aggregate.view(1, -1), global_flat, None, None)

    def step_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                    global_flat: torch.Tensor,
                    row_index: Optional[Sequence[int]] = None) -> torch.Tensor:
        """global_flat steps from the base's aggregate of the client rows packed[row_index]
        ([clients, >= P] fp32 on the device; default: every row, in order)."""
        C, P = len(num_samples), global_flat.numel()
        if C == 0:
            raise FedAvgError("No updates to aggregate")
        if row_index is not None and len(row_index) != C:
            raise FedAvgError("row_index and num_samples differ in length")
        if row_index is None and packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        if not self.plain_base:
            if self._scratch is None or self._scratch.numel() != P \
                    or self._scratch.device != packed.device:
                self._scratch = torch.empty(P, dtype=torch.float32, device=packed.device)
            extra = {"center": global_flat} if getattr(self.base, "uses_center", False) else {}
            self.base.aggregate_packed(packed[:, :P], num_samples, row_index=row_index,
                                       out=self._scratch, **extra)
            return self.step_vector(self._scratch, global_flat)
        w = self.base._calculate_sample_weights_n(list(num_samples))
        w32 = torch.tensor(w, dtype=torch.float32, device=packed.device)
        idx = None if row_index is None else torch.tensor([int(i) for i in row_index],
                                                          dtype=torch.int32, device=packed.device)
        return self.step_rows(packed, w32, global_flat, idx)

    def aggregate_updates(self, updates: List[ModelUpdate], round_number: int,
                          previous_model: GlobalModel) -> GlobalModel:
        """The reference-style entry point: the base aggregates the updates (its filtering,
        truncation, weights and history), the result is packed in the layer order of update 0
        and the previous global model steps toward it."""
        try:
            agg = self.base.aggregate_updates(updates)
            prev = previous_model.model_weights
            names = list(agg.model_weights)
            for n in names:
                if n not in prev or prev[n].shape != agg.model_weights[n].shape:
                    raise FedAvgError(f"previous model has no layer {n} of shape "
                                      f"{tuple(agg.model_weights[n].shape)}")
            dev = self.device

            def flat(weights):
                return torch.cat([weights[n].detach().to(device=dev, dtype=torch.float32)
                                  .reshape(-1) for n in names])
            aggregate, g = flat(agg.model_weights), flat(prev)
            self.step_vector(aggregate, g)
            out, o = {}, 0
            for n in names:
                s = prev[n].numel()
                out[n] = g[o:o + s].view(prev[n].shape).to(prev[n].device)
                o += s
            return GlobalModel(round_number=round_number, model_weights=out,
                               accuracy_metrics={},
                               participating_clients=agg.participating_clients,
                               convergence_score=0.0, created_at=datetime.now())
        except FedAvgError:
            raise
        except Exception as e:
            logger.error(f"Server optimizer step failed: {e}")
            raise FedAvgError(f"Server optimizer step failed: {e}") from e


def FedAvgM(server_lr: float, **kw) -> ServerOptimizer:
    return ServerOptimizer(ops.SOPT_MOMENTUM, server_lr, **kw)


def FedAdagrad(server_lr: float, **kw) -> ServerOptimizer:
    return ServerOptimizer(ops.SOPT_ADAGRAD, server_lr, **kw)


def FedAdam(server_lr: float, **kw) -> ServerOptimizer:
    return ServerOptimizer(ops.SOPT_ADAM, server_lr, **kw)


def FedYogi(server_lr: float, **kw) -> ServerOptimizer:
    return ServerOptimizer(ops.SOPT_YOGI, server_lr, **kw)


def create_server_optimizer(kind: str, **kwargs) -> ServerOptimizer:
    """"fedavgm" | "fedadagrad" | "fedadam" | "fedyogi"."""
    if kind not in RULES:
        raise ValueError(f"unknown server optimizer: {kind!r}")
    return ServerOptimizer(RULES[kind], **kwargs)
