"""Central, client-level differential privacy at the aggregation step: DP-FedAvg (McMahan et
al., "Learning Differentially Private Recurrent Language Models", ICLR 2018) with adaptive
quantile clipping (Andrew et al., "Differentially Private Learning with Adaptive Clipping",
NeurIPS 2021); every step runs on HIP.

The reference repository's DP is local: each client clips its own delta and adds its own noise
(fedhip.round.DPConfig, csrc/dp.hip).  Here the server clips every client's delta d_k = x_k - g
to an L2 norm C_t, averages the clipped deltas with UNIFORM weights 1/m (sample-count weights
would make the sensitivity depend on the data) and adds ONE Gaussian draw of standard deviation
z * C_t / m to the average, so the noise falls with the client count instead of being paid once
per client.  The clip norm follows the target quantile gamma of the clients' norms:

    b_k     = n_k <= C_t                      n_k = ||d_k||, whole row, fp64
    out     = g + ( sum_k fl32(min(1, C_t/n_k)) * fl32(1/m) * d_k  +  z_delta * C_t / m * N(0, I) )
    bbar    = (sum_k b_k + sigma_b * N(0, 1)) / m
    C_{t+1} = C_t * exp(-eta * (bbar - gamma))
    z_delta = (z^-2 - (2 sigma_b)^-2)^(-1/2)        eta = 0: z_delta = z, C_{t+1} = C_t

The exact arithmetic is that of fh_dpfa_* (include/fedhip.h).  The clip norm lives
on the device and is updated there: a round adds no host synchronisation.

What is protected is the PARAMETER aggregate.  BatchNorm running statistics are computed from
client data and are outside the guarantee; ``release_buffers=False`` keeps RankRound from
averaging them.
"""
from __future__ import annotations

import logging
import math
import secrets
from dataclasses import dataclass
from datetime import datetime
from typing import Any, Dict, List, Optional, Tuple

import torch

from fedhip import ops

from ..shared.models import GlobalModel, ModelUpdate
from .fedavg import FedAvgAggregator, FedAvgError

logger = logging.getLogger(__name__)

MASK64 = (1 << 64) - 1
_FIELDS = ("noise_multiplier", "clip_norm", "target_quantile", "clip_lr", "bit_noise",
           "release_buffers")


def round_key(dp_seed: int, seed: int, round_index: int) -> int:
    """The Philox key of one round: RankRound's DP round key."""
    return (int(dp_seed) * 6364136223846793005 + int(seed) * 1442695040888963407
            + int(round_index)) & MASK64


def delta_noise_multiplier(noise_multiplier: float, bit_noise: float) -> float:
    """z_delta = (z^-2 - (2 sigma_b)^-2)^(-1/2): the multiplier left for the deltas once the
    clipped-bit count has taken its share of the budget (Andrew et al., Thm. 1).  z = 0 stays 0;
    2 sigma_b <= z is refused (the count alone would exceed the budget)."""
    z, sb = float(noise_multiplier), float(bit_noise)
    if z == 0.0:
        return 0.0
    if 2.0 * sb <= z:
        raise ValueError(f"bit_noise={sb!r}: 2*bit_noise must exceed noise_multiplier={z!r}")
    return (z ** -2 - (2.0 * sb) ** -2) ** -0.5


def gaussian_epsilon(noise_multiplier: float, rounds: int, delta: float) -> float:
    """epsilon of `rounds` composed Gaussian mechanisms of noise multiplier z at `delta`, closed
    form.  The Renyi DP of the composition is T*alpha / (2 z^2) at every order alpha > 1; its
    conversion  eps(alpha) = T*alpha/(2 z^2) + ln(1/delta)/(alpha - 1)  is smallest at
    alpha = 1 + z*sqrt(2 ln(1/delta) / T), where it is

        eps = T / (2 z^2) + sqrt(2 T ln(1/delta)) / z.

    This is an UPPER BOUND, and it assumes every client takes part in every round (what
    RankRound does): there is no amplification by client sampling here."""
    z, T, d = float(noise_multiplier), int(rounds), float(delta)
    if not (z > 0 and math.isfinite(z)) or T < 1 or not 0.0 < d < 1.0:
        raise ValueError(f"gaussian_epsilon: need z > 0, rounds >= 1, 0 < delta < 1 "
                         f"(got {noise_multiplier!r}, {rounds!r}, {delta!r})")
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / d)) / z


@dataclass
class CentralDPConfig:
    """noise_multiplier z (0: clipping only), the initial clip_norm C_0, the target quantile
    gamma, the clip learning rate eta (0: a fixed clip norm) and the deviation sigma_b of the
    noise on the clipped-bit count (None: m/20 when eta > 0, the paper's default)."""
    noise_multiplier: float
    clip_norm: float
    target_quantile: float = 0.5
    clip_lr: float = 0.2
    bit_noise: Optional[float] = None
    release_buffers: bool = True

    def __post_init__(self):
        z, c = float(self.noise_multiplier), float(self.clip_norm)
        if not (math.isfinite(z) and z >= 0):
            raise ValueError(f"noise_multiplier must be finite and >= 0: {z!r}")
        if not (math.isfinite(c) and c > 0):
            raise ValueError(f"clip_norm must be finite and > 0: {c!r}")
        if not 0.0 <= float(self.target_quantile) <= 1.0:
            raise ValueError(f"target_quantile must lie in [0, 1]: {self.target_quantile!r}")
        if not (math.isfinite(float(self.clip_lr)) and self.clip_lr >= 0):
            raise ValueError(f"clip_lr must be finite and >= 0: {self.clip_lr!r}")
        if self.bit_noise is not None:
            if not (math.isfinite(float(self.bit_noise)) and self.bit_noise >= 0):
                raise ValueError(f"bit_noise must be finite and >= 0: {self.bit_noise!r}")
            if self.clip_lr > 0:
                delta_noise_multiplier(z, self.bit_noise)

    def resolve(self, m: int) -> Tuple[float, float]:
        """(z_delta, sigma_b) for a round of m clients."""
        if self.clip_lr == 0:
            return float(self.noise_multiplier), 0.0
        sb = m / 20.0 if self.bit_noise is None else float(self.bit_noise)
        return delta_noise_multiplier(self.noise_multiplier, sb), sb


class DPFedAvg:
    """The central-DP aggregate and its device-resident clip state (ops.DPFA_STATE_DOUBLES
    doubles, allocated once and carried across rounds)."""

    def __init__(self, config: CentralDPConfig, device: Optional[torch.device] = None,
                 dp_seed: Optional[int] = None, base: Optional[FedAvgAggregator] = None):
        if not isinstance(config, CentralDPConfig):
            raise ValueError(f"config must be a CentralDPConfig: {type(config).__name__}")
        self.config = config
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        # a public seed makes the noise recomputable, i.e. no privacy: secret unless fixed
        self.dp_seed = secrets.randbits(63) if dp_seed is None else int(dp_seed)
        self.base = base if base is not None else FedAvgAggregator(device=self.device)
        self.state = torch.zeros(ops.DPFA_STATE_DOUBLES, dtype=torch.float64, device=self.device)
        self.state[ops.DPFA_CLIP] = float(config.clip_norm)
        self.sigma = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._one = torch.ones(1, dtype=torch.float32, device=self.device)
        self._bufs: Dict[int, Dict[str, torch.Tensor]] = {}
        self.last: Dict[str, torch.Tensor] = {}
        self.rounds = 0

    # ------------------------------------------------------------------ state
    @property
    def clip_norm(self) -> float:
        """The clip norm the next round uses (reads the device back: synchronises)."""
        return float(self.state[ops.DPFA_CLIP].item())

    def state_dict(self) -> Dict[str, Any]:
        d: Dict[str, Any] = {name: getattr(self.config, name) for name in _FIELDS}
        d["state"] = self.state.detach().clone()
        d["rounds"] = self.rounds
        return d

    def load_state_dict(self, state: Dict[str, Any]):
        missing = [k for k in _FIELDS + ("state",) if k not in state]
        if missing:
            raise FedAvgError(f"central DP state lacks {missing}")
        try:
            config = CentralDPConfig(**{name: state[name] for name in _FIELDS})
        except (ValueError, TypeError) as e:
            raise FedAvgError(f"bad central DP state: {e}") from e
        t = state["state"]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 \
                or tuple(t.shape) != (ops.DPFA_STATE_DOUBLES,):
            raise FedAvgError(f"central DP state: the block must be {ops.DPFA_STATE_DOUBLES} "
                              f"float64 values")
        c = float(t[ops.DPFA_CLIP])
        if not (math.isfinite(c) and c > 0):
            raise FedAvgError(f"central DP state: clip norm {c!r}")
        self.config = config
        self.state.copy_(t.detach().to(self.device))
        self.rounds = int(state.get("rounds", 0))
        self.last = {}

    def _buf(self, C: int) -> Dict[str, torch.Tensor]:
        b = self._bufs.get(C)
        if b is None:
            dev = self.device
            b = self._bufs[C] = {
                "sqnorms": torch.empty(C, dtype=torch.float64, device=dev),
                "norms": torch.empty(C, dtype=torch.float64, device=dev),
                "scale": torch.empty(C, dtype=torch.float32, device=dev),
                "bits": torch.empty(C, dtype=torch.int32, device=dev)}
        return b

    # ------------------------------------------------------------------ steps
    def _coef(self, packed, global_flat, row_index, m):
        C = packed.shape[0] if row_index is None else row_index.numel()
        if C < 1 or m < C:
            raise FedAvgError(f"{C} client rows in a round of m={m} clients")
        z_delta, _ = self.config.resolve(m)
        b = self._buf(C)
        ops.dpfa_row_sqnorm(packed, global_flat, row_index=row_index, P=global_flat.numel(),
                            out=b["sqnorms"])
        ops.dpfa_clip_coef(b["sqnorms"], self.state, m, z_delta, scale=b["scale"],
                           bits=b["bits"], sigma=self.sigma)
        torch.sqrt(b["sqnorms"], out=b["norms"])
        self.last = b
        return b["scale"]

    def _noise_args(self, noise):
        if noise is not None:
            return {"noise": noise}
        return {"sigma": self.sigma} if self.config.noise_multiplier > 0 else {}

    def _update(self, m, seed, bit_sum=None):
        _, sigma_b = self.config.resolve(m)
        ops.dpfa_clip_update(self.state, m, self.config.target_quantile, self.config.clip_lr,
                             sigma_b, seed=seed, bit_sum=bit_sum)
        self.rounds += 1

    def step_rows(self, packed: torch.Tensor, global_flat: torch.Tensor,
                  row_index: Optional[torch.Tensor], m: int, seed: int,
                  out: Optional[torch.Tensor] = None,
                  noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One rank, every client's row at hand: norms -> coefficients -> clipped noisy sum ->
        clip update.  out (default, and possibly: global_flat) = the noisy aggregate of
        packed[row_index] (device int32; None: every row) around global_flat; m = the round's
        client count; seed = the round's Philox key; noise (fp32 [P]) replaces the draw."""
        scale = self._coef(packed, global_flat, row_index, m)
        out = global_flat if out is None else out
        ops.dpfa_clip_sum(packed, scale, out, global_=global_flat, row_index=row_index,
                          seed=seed, P=global_flat.numel(), **self._noise_args(noise))
        self._update(m, seed)
        return out

    def partial_rows(self, packed: torch.Tensor, global_flat: torch.Tensor,
                     row_index: Optional[torch.Tensor], m: int,
                     out: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Several ranks, this rank's part: (out = sum over ITS rows of s_k * d_k, without g
        and without noise; its clipped-bit count, a one-element float64 view of the state
        block).  Both are all-reduced (SUM) and handed to finish()."""
        scale = self._coef(packed, global_flat, row_index, m)
        ops.dpfa_clip_sum(packed, scale, out, global_=global_flat, row_index=row_index,
                          add_global=False, P=global_flat.numel())
        return out, self.state[ops.DPFA_BITSUM:ops.DPFA_BITSUM + 1]

    def finish(self, partial: torch.Tensor, bit_sum: torch.Tensor, global_flat: torch.Tensor,
               m: int, seed: int, out: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out = global_flat + (partial + noise) from the all-reduced partial sum, and the clip
        update from the all-reduced bit count.  Every rank runs it with the same key on the
        same values: the ranks stay bit-identical without a broadcast."""
        P = global_flat.numel()
        out = global_flat if out is None else out
        ops.dpfa_clip_sum(partial.view(1, -1), self._one, out, global_=global_flat, seed=seed,
                          rows_are_deltas=True, P=P, **self._noise_args(noise))
        self._update(m, seed, bit_sum=bit_sum)
        return out

    def aggregate_updates(self, updates: List[ModelUpdate], round_number: int,
                          previous_model: GlobalModel) -> GlobalModel:
        """The reference-style entry point: the updates are filtered as FedAvg's are, packed in
        the layer order of update 0 and aggregated around the previous global model."""
        try:
            base = self.base
            base._validate_aggregation_inputs(updates, None)
            valid = base._filter_and_validate_updates(updates)
            if len(valid) < base.min_clients:
                raise FedAvgError(f"Insufficient valid updates: {len(valid)} < "
                                  f"{base.min_clients}")
            rows, names, offs, sizes = base._pack_updates(valid)
            prev = previous_model.model_weights
            ref = valid[0].model_weights
            for n in names:
                if n not in prev or prev[n].shape != ref[n].shape:
                    raise FedAvgError(f"previous model has no layer {n} of shape "
                                      f"{tuple(ref[n].shape)}")
            g = torch.cat([prev[n].detach().to(device=self.device, dtype=torch.float32)
                           .reshape(-1) for n in names])
            self.step_rows(rows, g, None, len(valid),
                           round_key(self.dp_seed, 0, round_number))
            return GlobalModel(round_number=round_number,
                               model_weights=base._unpack_row(g, prev, names, offs, sizes),
                               accuracy_metrics={},
                               participating_clients=[u.client_id for u in valid],
                               convergence_score=0.0, created_at=datetime.now())
        except FedAvgError:
            raise
        except Exception as e:
            logger.error(f"DP-FedAvg aggregation failed: {e}")
            raise FedAvgError(f"DP-FedAvg aggregation failed: {e}") from e
