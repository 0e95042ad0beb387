"""One federated round on one GPU rank: local training -> update-level DP -> FedAvg.

Reference control flow replaced (per round):
  FederatedTrainer._perform_local_training  src/client/federated_trainer.py:390-426
  FederatedTrainer._apply_differential_privacy  :428-469
  FederatedLearningServicer._perform_aggregation  src/coordinator/grpc_server.py:465-506
    -> FedAvgAggregator.aggregate_updates  src/aggregation/fedavg.py:56-124

Multi-GPU (one process per GPU, torch.distributed over RCCL): clients are
LPT-assigned to ranks by sample count; each rank trains its clients as one
packed job, forms its partial FedAvg sum  S_r = sum_{k in r} fl32(w_k) x_k
(w_k = n_k / sum_all n, host double, client-list order inside the rank), and
one all_reduce(SUM) of the P-float vector over xGMI yields the new global
model on every rank (no broadcast needed).  With one rank the sum is the
reference's sequential loop, bit for bit.  With more ranks the association of
the all-reduce differs from that loop by a few ulp; ``exact=True`` instead
all-gathers every client's row and runs the sequential FedAvg kernel over all
clients in global client order on every rank (fedavg.py:278-285 bit for bit, at
C x P floats of gather traffic per rank instead of one P-float all-reduce).

``aggregator`` (a src.aggregation.robust rule: trimmed mean, median, Krum, geometric median,
centered clipping, FLTrust) replaces the FedAvg of the PARAMETER rows by the rule's ``aggregate_packed``
over the same rows: this rank's on one rank, the all-gathered rows of every client (global client
order) with ``exact=True`` on several.  A rule with ``uses_center`` (geometric median, centered
clipping) is also handed the previous global vector as ``center=``.  A robust rule is not a sum,
so it cannot be all-reduced: several ranks without
``exact`` are refused at construction.  The BN running statistics (``global_bufs``) keep the
plain FedAvg.  With ``aggregator=None`` nothing changes.

``aggregator=FLTrustAggregator(...)`` with ``trust_root=<global client id>`` (Cao et al., NDSS
2021): that client's shard is the server's clean root dataset.  It trains like every
other client (the step programs, lanes, ``dp``, ``compression`` and the BN-buffer FedAvg do not
know about it); its trained row is the reference direction and is left out of the sum.  Every
other client's delta is scored by its cosine with the root's delta, negative scores are clipped to
zero, the deltas are rescaled to the root delta's norm and averaged with the scores as weights,
in one ``fh_fltrust_rows`` call.  One rank: the rule runs over this rank's other rows, so the
root must be this rank's client.  ``exact=True`` on several ranks: over the all-gathered rows in
global client order, the root's row taken from the gather.  ``server_opt`` composes as with the
other robust rules.  Refused: the rule without ``trust_root`` and ``trust_root`` without the rule, a
root that is not a client of the round (on one rank: of this rank) or whose shard is empty, no
other client or more than 64 of them, and what every robust rule refuses (several ranks without
``exact``, ``fednova``, ``qfedavg``, ``central_dp``).  A round in which no client is trusted raises
FedAvgError and leaves the global vector as it was.  With ``trust_root=None`` nothing changes.

``server_opt`` (a src.aggregation.fedopt.ServerOptimizer: FedAvgM, FedAdagrad, FedAdam, FedYogi)
replaces the assignment of the aggregate to the global PARAMETER vector by one server-optimizer
step toward it.  One rank without ``aggregator``: one fused launch over the rank's rows (the
weighted sum never leaves registers).  Every other path forms its aggregate in ``partial`` as
before (the all-reduced sum, the exact-mode FedAvg, the robust rule) and a single-row step
follows; every rank holds the same state and runs the same deterministic kernel on the same
aggregate, so the ranks stay bit-identical without a broadcast.  A ``server_opt`` whose ``base``
is a robust rule uses that rule as ``aggregator``; given together with ``aggregator=`` it is
refused.  The BN running statistics keep the plain FedAvg.  With ``server_opt=None`` nothing
changes.

``central_dp`` (a src.aggregation.dpfedavg.CentralDPConfig) replaces the FedAvg of the PARAMETER
rows by the central DP-FedAvg aggregate: every client's delta clipped to the (adaptive) clip
norm, averaged with uniform weights 1/m over ALL clients of the round and one Gaussian draw
added to the average (src/aggregation/dpfedavg.py).  One rank, and ``exact=True`` on several
(the all-gathered rows in global client order): the fused path.  Several ranks otherwise: each
rank's clipped partial sum and clipped-bit count are all-reduced and every rank finishes with
the same round key, so the ranks stay bit-identical without a per-round broadcast (the ranks
adopt rank 0's ``dp_seed`` once, at construction: the one shared draw needs one secret).  The aggregate lands
where FedAvg's would, so ``server_opt`` composes unchanged.  Refused together with ``dp`` (two
mechanisms, no joint accounting) and with a robust ``aggregator`` (the sensitivity argument
needs a sum).  The BN running statistics are outside the guarantee: ``release_buffers=False``
leaves ``global_bufs`` as it was.  With ``central_dp=None`` nothing changes.

``compression`` (a fedhip.compress.CompressionConfig) compresses every client's update delta
before any aggregation sees the rows.  The order of a round is train -> ``dp`` -> compression ->
aggregation.  ``error_feedback=True`` makes the round own ``residual`` ([S, P], one row per slot,
zero at construction, kept across ``run()`` calls, cleared by ``reset_compression_state()``):
each client compresses its delta plus its residual and keeps what was not sent.  With ``dp`` the
residual therefore also carries what compression removed from the NOISED delta; compression and
the residual are post-processing of the mechanism's output, so the DP statement is untouched.
``stochastic=True`` draws the quantiser's rounding words from the round key under the clients'
global ids (``squant_words``, uint32 [S, P], replaces the draw for exact replay).  Compression
works on a rank's own rows, and the client-to-rank assignment is fixed for a RankRound, so it
composes unchanged with ``exact``, ``aggregator``, ``server_opt``, ``central_dp`` and several
ranks.  A client with an empty shard sends from its residual at FedAvg weight 0.  With the
default CompressionConfig options nothing changes.

``sparse=True`` (top-k only; fedhip/sparse.py) also packs every client's kept
coordinates into (index, value) payload rows, kept as ``last_sparse`` (one row per slot, rewritten
by every ``run()``; ``wire.sparse_to_payloads`` turns it into the reference's upload dicts).  The
plain FedAvg routes (no ``aggregator``, no ``central_dp``, not ``exact``) sum from the payload and
leave the trained rows as they are; with ``server_opt`` on one rank the sum lands in ``partial``
and ``step_vector`` follows.  The other routes rebuild the dense rows from the payload first.
The global model, ``global_bufs`` and ``residual`` are bit for bit those of ``sparse=False``.

``packed=True`` (deterministic quantisation with bits <= 8 only; fedhip/quantpack.py, DESIGN.md
D22) is the quantiser's counterpart: every client's codes are bit-packed into payload rows next to
their scale and zero point, kept as ``last_quant`` (one row per slot, rewritten by every
``run()``; ``wire.quant_to_payloads`` turns it into the reference's upload dicts).  The plain
FedAvg routes (no ``aggregator``, no ``central_dp``, not ``exact``; one or several ranks, with or
without ``server_opt``) sum the parameter aggregate from the payload with ``quant_fedavg`` and
leave the trained rows as they are; the other routes rebuild the dense rows first and proceed as
without it.  ``global_flat``, ``global_bufs`` and ``residual`` are bit for bit those of
``packed=False``.

``fednova`` (``True`` or a src.aggregation.fednova.FedNovaConfig) replaces the FedAvg of the
PARAMETER rows by FedNova's normalised average (Wang et al., NeurIPS 2020)
    x_new = g + tau_eff * sum_k (p_k / a_k) * (x_k - g),      tau_eff = sum_k p_k * a_k,
with a_k = epochs * ceil(n_k / batch) the local step count of client k.  The host knows every
client's step count on every rank, so the coefficients and tau_eff are computed over all clients
in global client order at construction and every rank holds the same tau_eff with no extra
collective.  One rank: one STEP launch.  Several ranks: each rank's PARTIAL sum over its rows,
the one all-reduce, then FINISH on every rank.  ``exact=True``: STEP over the all-gathered rows
in global client order.  The result lands where FedAvg's would, so ``server_opt`` composes
unchanged (a single-row step follows).  ``dp`` and ``compression`` stay allowed; the sums from the
sparse and packed payloads are FedAvg's, so under FedNova the dense rows are rebuilt.  Refused
with a robust ``aggregator`` (the rule is a weighted sum, the robust rules are not) and with
``central_dp`` (its sensitivity argument needs uniform weights, D19).  The BN running statistics
keep the plain FedAvg: they are not the product of gradient steps.  With ``fednova=None`` nothing
changes.

``qfedavg`` (``True`` or a src.aggregation.qfedavg.QFedAvgConfig) replaces the FedAvg of the
PARAMETER rows by q-FedAvg's fairness-aware step (Li et al., ICLR 2020, Algorithm 2; DESIGN.md
D25)
    x_new = g + (1/den) * sum_k a_k * (x_k - g),    den = sum_k (b_k * ||x_k - g||^2 + a_k),
    a_k = pi_k * F_k^q,    b_k = pi_k * q * L * F_k^(q-1),
with pi_k = 1/m over all clients of the round (``weights="samples"``: the FedAvg weights) and
L = ``lipschitz``, by default 1/lr of that ``run()`` call (the paper's estimate).  F_k is the
paper's loss of client k AT the global model it started from: ``run(..., client_losses=)`` takes
it from the caller (a mapping client id -> loss, or a sequence indexed by global client id).  By
default the round's own ``ClientMetrics.loss`` stands in, the mean training loss of the client's
last local epoch, which is already on the host; it is a proxy, not the paper's quantity.  A client
with an empty shard (loss NaN, FedAvg weight 0) or with a negative or non-finite loss is not live:
it is skipped.  The coefficients are host bookkeeping per ``run()``; den stays on the device.  One
rank: one STEP over this rank's rows.  Several ranks: each rank's PARTIAL sum and share of den,
one all-reduce of the [P] sum and one of the fp64 den, then FINISH on every rank.  ``exact=True``:
the ranks exchange their clients' losses and run one STEP over the all-gathered rows in global
client order.  The result lands where FedAvg's would, so ``server_opt`` composes unchanged (a
single-row step follows).  ``dp`` and ``compression`` stay allowed; the sums from the sparse and
packed payloads are FedAvg's, so under q-FedAvg the dense rows are rebuilt.  Refused with
``fednova`` (two different reweightings of the same deltas), with a robust ``aggregator`` (the rule
is a weighted sum, the robust rules are not) and with ``central_dp`` (its sensitivity argument
needs weights that do not depend on the clients' data, D19).  The BN running statistics keep the
plain FedAvg.  With ``qfedavg=None`` nothing changes.
"""
from __future__ import annotations

import math
import os
import secrets
import sys
import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from . import ops
from .lanes import HOST_TIMING as _HOST_TIMING  # diagnostics: per-round host split
from .lanes import LanedTrainer


@dataclass
class DPConfig:
    epsilon: float
    delta: float = 1e-5
    max_grad_norm: float = 1.0


class RankRound:
    def __init__(self, template_model, all_train_sizes: Sequence[int], my_clients: Sequence[int],
                 epochs: int = 1, batch: int = 32, device="cuda", dp: Optional[DPConfig] = None,
                 group=None, lanes=None, compression=None, transform=None, dp_seed=None,
                 shuffle_seed=None, exact=False, aggregator=None, server_opt=None,
                 central_dp=None, fednova=None, qfedavg=None, trust_root=None):
        self.device = torch.device(device)
        self._template = template_model
        self.B, self.epochs, self.dp, self.group = batch, epochs, dp, group
        self.all_sizes = list(all_train_sizes)
        # slots: this rank's clients ordered by descending step count (stable)
        self.clients = sorted(my_clients)
        self.slots = sorted(self.clients, key=lambda k: (-math.ceil(self.all_sizes[k] / batch), k))
        self.slot_of = {k: i for i, k in enumerate(self.slots)}
        steps = [epochs * math.ceil(self.all_sizes[k] / batch) for k in self.slots]
        self.distributed = group is not None or (dist.is_available() and dist.is_initialized())
        self.rank = dist.get_rank(group) if self.distributed else 0
        if server_opt is not None and not server_opt.plain_base:
            if aggregator is not None:
                raise ops.FedHipError("server_opt has a robust base and aggregator= is given "
                                      "too: ambiguous, pass the rule once")
            aggregator = server_opt.base
        self.aggregator, self.server_opt = aggregator, server_opt
        if aggregator is not None and not exact and self.distributed \
                and dist.get_world_size(group) > 1:
            raise ops.FedHipError("a robust aggregator over several ranks needs exact=True: "
                                  "the rule is not a sum and cannot be all-reduced")
        # FLTrust: the shard of client `trust_root` is the server's root dataset.  It trains
        # like every other client; its row is the reference direction and is left out of the sum
        uses_root = getattr(aggregator, "uses_root", False)
        if uses_root and trust_root is None:
            raise ops.FedHipError(f"{type(aggregator).__name__} scores the clients against the "
                                  f"server's root update: pass trust_root=<global client id>")
        if trust_root is not None:
            if not uses_root:
                raise ops.FedHipError("trust_root names the server's root shard for a rule that "
                                      "uses one: pass aggregator=FLTrustAggregator(...)")
            if isinstance(trust_root, bool) or not isinstance(trust_root, int) \
                    or not 0 <= trust_root < len(self.all_sizes):
                raise ops.FedHipError(f"trust_root={trust_root!r} is not a client of the round "
                                      f"(0..{len(self.all_sizes) - 1})")
            if self.all_sizes[trust_root] <= 0:
                raise ops.FedHipError(f"trust_root={trust_root}: the root shard is empty, the "
                                      f"server would have no update to score against")
            gathered = bool(exact) and self.distributed
            if not gathered and trust_root not in self.clients:
                raise ops.FedHipError(f"trust_root={trust_root} is not one of this rank's clients "
                                      f"{self.clients}: on one rank the root trains here")
            nmax = (len(self.all_sizes) if gathered else len(self.clients)) - 1
            if not 1 <= nmax <= ops.FLT_MAX_CLIENTS:
                raise ops.FedHipError(f"fltrust: {nmax} clients beside the root in one call, "
                                      f"fh_fltrust_rows takes 1..64")
        self.trust_root = trust_root
        if fednova is not None and fednova is not False:
            if fednova is True:
                from src.aggregation.fednova import FedNovaConfig
                fednova = FedNovaConfig()
            if aggregator is not None:
                raise ops.FedHipError("fednova is a weighted sum of normalised deltas and a "
                                      "robust aggregator is not a sum: they cannot be combined")
            if central_dp is not None:
                raise ops.FedHipError("fednova weighs the clients by p_k / a_k and central_dp's "
                                      "sensitivity argument needs uniform weights (D19): they "
                                      "cannot be combined")
        else:
            fednova = None
        self.fednova = fednova
        if qfedavg is not None and qfedavg is not False:
            if qfedavg is True:
                from src.aggregation.qfedavg import QFedAvgConfig
                qfedavg = QFedAvgConfig()
            if fednova is not None:
                raise ops.FedHipError("qfedavg and fednova both reweight the clients' deltas, by "
                                      "the loss and by the step count: pass one")
            if aggregator is not None:
                raise ops.FedHipError("qfedavg is a weighted sum of the clients' deltas and a "
                                      "robust aggregator is not a sum: they cannot be combined")
            if central_dp is not None:
                raise ops.FedHipError("qfedavg weighs the clients by their losses and central_dp's "
                                      "sensitivity argument needs weights that do not depend on "
                                      "the data (D19): they cannot be combined")
            nmax = len(self.all_sizes) if exact and self.distributed else len(self.clients)
            if nmax > 64:
                raise ops.FedHipError(f"qfedavg: {nmax} clients in one call, fh_qfedavg_rows "
                                      f"takes at most 64")
        else:
            qfedavg = None
        self.qfedavg = qfedavg
        self.central = None
        if central_dp is not None:
            if dp is not None:
                raise ops.FedHipError("central_dp and dp are two DP mechanisms with no joint "
                                      "accounting: pass one")
            if aggregator is not None:
                raise ops.FedHipError("central_dp needs a sum (its sensitivity argument does): "
                                      "a robust aggregator cannot be combined with it")
            if not self.clients:
                raise ops.FedHipError("central_dp: this rank holds no client")
            try:  # 2 * bit_noise <= noise_multiplier is refused here, not in round one
                central_dp.resolve(len(self.all_sizes))
            except ValueError as e:
                raise ops.FedHipError(f"central_dp: {e}") from e
        self.trainer = LanedTrainer(template_model, steps or [0], batch=batch, device=self.device,
                                    lanes=lanes, salt=self.rank)
        if self.slots:  # dropout / augmentation keyed by global client id (not rank / lane)
            self.trainer.set_client_ids(self.slots)
        self.transform = transform  # ops.DataTransform when the shards are raw uint8 images
        self.trainer.transform = transform
        L = self.trainer.layout
        self.P = L.P
        self.global_flat = torch.zeros(self.P, device=self.device)
        with torch.no_grad():
            for n, p in template_model.named_parameters():
                L.view(self.global_flat.view(1, -1), n)[0].copy_(p.detach().reshape(-1))
        # FedAvg weights: samples_processed = epochs * train size (federated_trainer.py:481),
        # w_k = n_k / sum(n) in Python double (fedavg.py:255), rounded to fp32 at the multiply.
        processed = [epochs * n for n in self.all_sizes]
        total = sum(processed)
        self.weights = [n / total for n in processed]
        self.w32 = torch.tensor([self.weights[k] for k in self.clients], dtype=torch.float32,
                                device=self.device)
        self.rows = torch.tensor([self.slot_of[k] for k in self.clients], dtype=torch.int32,
                                 device=self.device)
        # FedNova: c_k = p_k / a_k and tau_eff over ALL clients in global client order (host
        # double), the same on every rank; this rank's coefficients in client-list order
        self._nova_coef = self._nova_c32 = self._nova_tau = None
        if fednova is not None:
            local_steps = [epochs * math.ceil(n / batch) for n in self.all_sizes]
            try:
                self._nova_coef, self._nova_tau = ops.fednova_coefficients(
                    self.weights, local_steps, fednova.tau_eff)
            except ValueError as e:
                raise ops.FedHipError(f"fednova: {e}") from e
            self._nova_c32 = torch.tensor([self._nova_coef[k] for k in self.clients],
                                          dtype=torch.float32, device=self.device)
        # what a robust aggregator is handed on one rank: its clients' rows and sample counts
        # (without the trust root, whose row is handed over as root_row=)
        self._agg_rows = [self.slot_of[k] for k in self.clients if k != trust_root]
        self._agg_samples = [processed[k] for k in self.clients if k != trust_root]
        self._agg_root = self.slot_of.get(trust_root)
        # update-level DP noise: Philox keyed by (round key, global client id, element), so
        # no two clients — on any rank or lane — ever draw the same noise; the round key
        # comes from a secret base seed (os.urandom) unless the caller fixes one (tests /
        # reproducible benchmarks: a public seed makes the noise recomputable, i.e. no
        # privacy)
        self.slot_ids = torch.tensor(list(self.slots), dtype=torch.int64, device=self.device)
        self.dp_seed = secrets.randbits(63) if dp_seed is None else int(dp_seed)
        # data shuffling when run() gets no generator: every client draws its epochs'
        # permutations from its own generator keyed by (shuffle seed, round seed, client
        # id) — independent of the rank / lane / slot it lands on
        self.shuffle_seed = secrets.randbits(62) if shuffle_seed is None else int(shuffle_seed)
        self.partial = torch.zeros(self.P, device=self.device)
        # q-FedAvg: den and the live count stay on the device; last_qfedavg keeps the host side
        # of the last run() (losses, a, b, L of this rank's call; no device read)
        self._qfa_state = self._qfa_sqdist = None
        self.last_qfedavg = None
        if qfedavg is not None:
            self._qfa_state = torch.zeros(ops.QFA_STATE_DOUBLES, dtype=torch.float64,
                                          device=self.device)
        # central DP-FedAvg: its own draws come from the same round key as the update-level
        # DP's, under stream words no client id can equal.  central_noise (fp32 [P]) replaces
        # the draw (exact replay)
        self.central_noise = None
        if central_dp is not None:
            from src.aggregation.dpfedavg import DPFedAvg
            if self.distributed and dist.get_world_size(group) > 1:
                # the aggregate carries ONE draw that every rank must make alike: the ranks
                # agree on rank 0's secret once, here (no per-round broadcast).  The per-client
                # streams of dp= tolerate per-rank secrets; this one does not.
                box = [self.dp_seed]
                src = 0 if group is None else dist.get_global_rank(group, 0)
                dist.broadcast_object_list(box, src=src, group=group)
                self.dp_seed = int(box[0])
            self.central = DPFedAvg(central_dp, self.device, dp_seed=self.dp_seed)
        # global BN running statistics for evaluation (f-1; divergence D13): FedAvg of the
        # clients' buffers with the same weights.  Clients keep their own buffers (D4).
        self.Q = L.Q
        self.global_bufs = torch.zeros(max(self.Q, 1), device=self.device)
        with torch.no_grad():
            for n, b in template_model.named_buffers():
                if n in L.buf_names:
                    L.bview(self.global_bufs.view(1, -1), n)[0].copy_(b.detach().reshape(-1))
        self.round_index = 0
        self._evaluator = None
        # test / diagnostic hooks: on_trained(params, S) sees the trained rows before DP /
        # compression / FedAvg; dp_noise [S, P] replaces the Philox draw (exact replay)
        self.on_trained = None
        self.dp_noise = None
        self.last_plan = None
        # update compression before FedAvg (f-3; insertion point D14): delta vs the global
        self.compression = compression
        self._cplan = None
        # error feedback: one residual row per slot, kept across run() calls; squant_words
        # (uint32 [S, P]) replaces the stochastic quantiser's Philox words (exact replay)
        self.residual = None
        self.squant_words = None
        if compression is not None:
            from .compress import SegmentPlan
            self._cplan = SegmentPlan(L.seg_offsets(), self.device)
            if compression.error_feedback:
                # row stride padded to 64 floats: every row starts on a 16-byte boundary
                self.residual = torch.zeros(max(len(self.slots), 1), (self.P + 63) // 64 * 64,
                                            device=self.device)[:, :self.P]
        # sparse top-k (D21): the slots' (index, value) payload rows, rewritten every round;
        # last_sparse is the payload of the last run()
        self._sparse = None
        self.last_sparse = None
        if compression is not None and compression.sparse:
            from .sparse import SparsePlan
            self._sparse = SparsePlan(self._cplan, compression.sparsity_ratio).empty(
                len(self.slots))
        # packed quantised updates (D22): the slots' code rows, rewritten every round;
        # last_quant is the payload of the last run()
        self._quant = None
        self.last_quant = None
        if compression is not None and compression.packed:
            from .quantpack import QuantPlan
            self._quant = QuantPlan(self._cplan, compression.bits).empty(len(self.slots))
        self.exact = bool(exact) and self.distributed
        if self.exact:
            self._init_exact()

    def _init_exact(self):
        """Exact-mode FedAvg layout: every rank's client list (host, once), rows padded to
        the largest rank's count, and the gather position of each global client."""
        world = dist.get_world_size(self.group)
        lists = [None] * world
        dist.all_gather_object(lists, list(self.clients), group=self.group)
        maxS = max(1, max(len(c) for c in lists))
        pos = {}
        for r, cl in enumerate(lists):
            for i, k in enumerate(cl):
                if k in pos:  # the all-reduce path would count it twice, this one once
                    raise ops.FedHipError(f"exact FedAvg: client {k} is listed by more than "
                                          f"one rank")
                pos[k] = r * maxS + i
        order = sorted(pos)  # global client order: the reference's sequential loop
        if order != list(range(len(self.all_sizes))):
            raise ops.FedHipError(f"exact FedAvg: the ranks' client lists cover {len(order)} "
                                  f"of {len(self.all_sizes)} clients")
        self._x_world, self._x_maxS = world, maxS
        self._x_w32 = torch.tensor([self.weights[k] for k in order], dtype=torch.float32,
                                   device=self.device)
        self._x_idx = torch.tensor([pos[k] for k in order], dtype=torch.int32, device=self.device)
        if self._nova_coef is not None:
            self._x_c32 = torch.tensor([self._nova_coef[k] for k in order], dtype=torch.float32,
                                       device=self.device)
        # what a robust aggregator is handed: every client but the trust root, global order
        self._x_rows = [pos[k] for k in order if k != self.trust_root]
        self._x_order = order
        self._x_samples = [self.epochs * self.all_sizes[k] for k in order if k != self.trust_root]
        self._x_root = pos.get(self.trust_root)
        self._x_mine = torch.tensor([self.slot_of[k] for k in self.clients], dtype=torch.int64,
                                    device=self.device)
        self._x_buf = {}

    def _exact_gather(self, rows, n):
        """[world * maxS, n]: this rank's rows (client-list order, zero padded) all-gathered;
        global client k sits at row _x_rows[k].  The row stride is n rounded up to 4 floats, so
        every row starts on a 16-byte boundary and the kernels take their vector paths."""
        world, maxS = self._x_world, self._x_maxS
        buf = self._x_buf.get(n)
        if buf is None:
            npad = (n + 3) // 4 * 4
            buf = self._x_buf[n] = (torch.zeros(maxS, npad, device=self.device),
                                    torch.empty(world, maxS, npad, device=self.device))
        send, recv = buf
        S = len(self.clients)
        if S:
            send[:S, :n].copy_(rows[:, :n].index_select(0, self._x_mine))
        dist.all_gather(list(recv.unbind(0)), send, group=self.group)
        return recv.view(world * maxS, -1)[:, :n]

    def _exact_fedavg(self, rows, n, out):
        """out = sum over ALL clients, in global client order, of fl32(w_k) * row_k: the
        all-gathered rows, then fh_fedavg_weighted_sum."""
        ops.fedavg_weighted_sum(self._exact_gather(rows, n), self._x_w32, out,
                                row_index=self._x_idx, P=n)

    def client_shuffle_seed(self, seed: int, client: int) -> int:
        """Seed of the torch.Generator client `client` draws its round-`seed` batch
        permutations from (one torch.randperm per local epoch, fedhip/engine.plan_round)."""
        return (self.shuffle_seed * 0x9E3779B97F4A7C15 + seed * 0xBF58476D1CE4E5B9
                + client * 0x94D049BB133111EB) & 0x7FFFFFFFFFFFFFFF

    def set_global(self, flat: torch.Tensor):
        self.global_flat.copy_(flat)

    def _sparse_sum(self):
        """Whether this round's parameter aggregate is summed from the sparse payload: the plain
        FedAvg routes.  Exact mode, a robust rule, central DP, FedNova and q-FedAvg read dense
        rows."""
        return self._sparse is not None and self.aggregator is None and self.central is None \
            and not self.exact and self.fednova is None and self.qfedavg is None

    def _quant_sum(self):
        """The same for the packed quantised payload."""
        return self._quant is not None and self.aggregator is None and self.central is None \
            and not self.exact and self.fednova is None and self.qfedavg is None

    def _center_kw(self, root_row=None):
        """A rule that iterates around a centre (geometric median, centered clipping, FLTrust)
        gets the previous global model as that centre; FLTrust also the trust root's row."""
        kw = {}
        if getattr(self.aggregator, "uses_center", False):
            kw["center"] = self.global_flat
        if self.trust_root is not None:
            kw["root_row"] = root_row
        return kw

    def _qfa_losses(self, metrics, client_losses):
        """{client id: F_k} of this rank's clients (exact mode: of every client): the caller's
        ``client_losses`` or, by default, the round's last-epoch training losses."""
        if client_losses is None:
            loss_of = {k: metrics[self.slot_of[k]].loss for k in self.clients}
            if self.exact:  # every rank needs every client's loss: one host exchange
                boxes = [None] * self._x_world
                dist.all_gather_object(boxes, loss_of, group=self.group)
                loss_of = {k: v for box in boxes for k, v in box.items()}
            return loss_of
        need = self._x_order if self.exact else self.clients
        if hasattr(client_losses, "keys"):
            missing = [k for k in need if k not in client_losses]
            if missing:
                raise ops.FedHipError(f"qfedavg: client_losses has no loss for clients {missing}")
            return {k: float(client_losses[k]) for k in need}
        if len(client_losses) != len(self.all_sizes):
            raise ops.FedHipError(f"qfedavg: {len(client_losses)} client_losses for "
                                  f"{len(self.all_sizes)} clients (indexed by global client id)")
        return {k: float(client_losses[k]) for k in need}

    def _qfa_coef(self, clients, loss_of, lr, require_live):
        """(a fp32 [C], b fp64 [C]) on the device for `clients` in that order; pi_k is 1/m over
        ALL clients of the round, or the FedAvg weight."""
        cfg = self.qfedavg
        m = len(self.all_sizes)
        pi = [1.0 / m if cfg.weights == "uniform" else self.weights[k] for k in clients]
        losses = [loss_of[k] for k in clients]
        try:
            L = cfg.lipschitz if cfg.lipschitz is not None else 1.0 / lr
            a, b = ops.qfedavg_coefficients(pi, losses, cfg.q, L, require_live=require_live)
        except (ValueError, ZeroDivisionError) as e:
            raise ops.FedHipError(f"qfedavg: {e}") from e
        self.last_qfedavg = {"clients": list(clients), "losses": losses, "a": a, "b": b,
                             "lipschitz": L}
        return (torch.tensor(a, dtype=torch.float32, device=self.device),
                torch.tensor(b, dtype=torch.float64, device=self.device))

    def reset_compression_state(self):
        """Forget every client's error-feedback residual (a new training run, or a new
        client-to-slot assignment, on the same RankRound)."""
        if self.residual is not None:
            self.residual.zero_()

    def run(self, data, labels, slot_offsets: Sequence[int], optimizer_type="sgd", lr=0.01,
            seed=0, generator=None, serialize_lanes=False, client_losses=None):
        """One round. data/labels: this rank's train shards, slot k's at slot_offsets[k].
        client_losses (only with ``qfedavg``): every client's loss at the global model the round
        starts from, a mapping client id -> loss or a sequence indexed by global client id."""
        if client_losses is not None and self.qfedavg is None:
            raise ops.FedHipError("client_losses is q-FedAvg's input: pass qfedavg= to RankRound")
        tr = self.trainer
        S = len(self.slots)
        _t = [time.perf_counter()] if _HOST_TIMING else None
        tr.params[:S, :self.P].copy_(self.global_flat.expand(S, -1))  # all start from global
        sizes = [self.all_sizes[k] for k in self.slots]
        cseeds = None
        if generator is None:
            cseeds = [self.client_shuffle_seed(seed, k) for k in self.slots]
        plan = tr.make_plan(sizes, self.epochs, generator=generator, client_seeds=cseeds)
        self.last_plan = plan
        if _t:
            _t.append(time.perf_counter())
        metrics = tr.run_round(data, labels, slot_offsets, plan, optimizer_type=optimizer_type,
                               lr=lr, seed=seed, serialize=serialize_lanes)
        if _t:
            _t.append(time.perf_counter())
        if self.on_trained is not None:
            self.on_trained(tr.params, S)
        if self.dp is not None:
            self._apply_dp(S, seed)
        if self.compression is not None:
            from .compress import compress_rows
            extra = {}
            if self.compression.error_feedback:
                extra["resid"] = self.residual
            if self.compression.stochastic:
                extra.update(key=self._round_key(seed), row_ids=self.slot_ids[:S],
                             words=self.squant_words)
            if self._sparse is not None:
                # the plain FedAvg sums straight from the payload: the rows stay as trained
                extra.update(sparse_out=self._sparse, rewrite_rows=not self._sparse_sum())
                self.last_sparse = self._sparse
            if self._quant is not None:
                extra.update(quant_out=self._quant, rewrite_rows=not self._quant_sum())
                self.last_quant = self._quant
            compress_rows(self._cplan, self.compression, tr.params, S,
                          base=self.global_flat.view(1, -1).expand(S, -1), **extra)
        distributed = self.distributed
        sopt = self.server_opt
        # with a server optimizer the aggregate lands in `partial` and the global steps to it
        agg_out = self.global_flat if sopt is None else self.partial
        cdp = self.central
        m_all = len(self.all_sizes)
        keep_bufs = cdp is not None and not cdp.config.release_buffers
        if self.exact:  # bit-exact multi-rank FedAvg: all-gather + one sequential sum
            if cdp is not None:  # the fused path over every client's row, global client order
                cdp.step_rows(self._exact_gather(tr.params, self.P), self.global_flat,
                              self._x_idx, m_all, self._round_key(seed), out=agg_out,
                              noise=self.central_noise)
            elif self.fednova is not None:  # one STEP over every client's row, global order
                ops.fednova_rows(self._exact_gather(tr.params, self.P), self._x_c32,
                                 self.global_flat, agg_out, self._nova_tau, ops.NOVA_STEP,
                                 row_index=self._x_idx, P=self.P)
            elif self.qfedavg is not None:  # one STEP over every client's row, global order
                a32, b64 = self._qfa_coef(self._x_order, self._qfa_losses(metrics, client_losses),
                                          lr, True)
                ops.qfedavg_rows(self._exact_gather(tr.params, self.P), a32, b64,
                                 self.global_flat, agg_out, ops.QFA_STEP, row_index=self._x_idx,
                                 P=self.P, state=self._qfa_state)
            elif self.aggregator is None:
                self._exact_fedavg(tr.params, self.P, agg_out)
            else:  # the rule over every client's row, in global client order, on every rank
                self.aggregator.aggregate_packed(self._exact_gather(tr.params, self.P),
                                                 self._x_samples, row_index=self._x_rows,
                                                 out=agg_out, **self._center_kw(self._x_root))
            if sopt is not None:
                sopt.step_vector(self.partial, self.global_flat)
            if self.Q and not keep_bufs:
                self._exact_fedavg(tr.bufs, self.Q, self.global_bufs)
            self.round_index += 1
            self._host_timing(_t)
            return metrics
        # FedAvg: this rank's partial sum in client-list order, then RCCL all-reduce.
        if cdp is not None:
            key = self._round_key(seed)
            if not distributed:
                cdp.step_rows(tr.params, self.global_flat, self.rows, m_all, key, out=agg_out,
                              noise=self.central_noise)
            else:  # clipped partial sum and bit count, all-reduced; every rank finishes alike
                part, bit_sum = cdp.partial_rows(tr.params, self.global_flat, self.rows, m_all,
                                                 out=self.partial)
                dist.all_reduce(part, op=dist.ReduceOp.SUM, group=self.group)
                dist.all_reduce(bit_sum, op=dist.ReduceOp.SUM, group=self.group)
                cdp.finish(part, bit_sum, self.global_flat, m_all, key, out=agg_out,
                           noise=self.central_noise)
            if sopt is not None:
                sopt.step_vector(self.partial, self.global_flat)
        elif self.fednova is not None:
            if not distributed:  # one launch: the whole rule over this rank's rows
                ops.fednova_rows(tr.params, self._nova_c32, self.global_flat, agg_out,
                                 self._nova_tau, ops.NOVA_STEP, row_index=self.rows, P=self.P)
            else:  # this rank's share of the normalised sum, one all-reduce, every rank finishes
                if self.clients:
                    ops.fednova_rows(tr.params, self._nova_c32, self.global_flat, self.partial,
                                     self._nova_tau, ops.NOVA_PARTIAL, row_index=self.rows,
                                     P=self.P)
                else:
                    self.partial.zero_()
                dist.all_reduce(self.partial, op=dist.ReduceOp.SUM, group=self.group)
                ops.fednova_rows(self.partial.view(1, -1), None, self.global_flat, agg_out,
                                 self._nova_tau, ops.NOVA_FINISH, P=self.P)
            if sopt is not None:
                sopt.step_vector(self.partial, self.global_flat)
        elif self.qfedavg is not None:
            loss_of = self._qfa_losses(metrics, client_losses)
            if not distributed:  # one call: the whole rule over this rank's rows
                a32, b64 = self._qfa_coef(self.clients, loss_of, lr, True)
                ops.qfedavg_rows(tr.params, a32, b64, self.global_flat, agg_out, ops.QFA_STEP,
                                 row_index=self.rows, P=self.P, state=self._qfa_state)
            else:  # this rank's shares of the sum and of den, two all-reduces, every rank finishes
                if self.clients:  # a rank without a live client adds zeros to both
                    a32, b64 = self._qfa_coef(self.clients, loss_of, lr, False)
                    ops.qfedavg_rows(tr.params, a32, b64, self.global_flat, self.partial,
                                     ops.QFA_PARTIAL, row_index=self.rows, P=self.P,
                                     state=self._qfa_state)
                else:
                    self.partial.zero_()
                    self._qfa_state.zero_()
                dist.all_reduce(self.partial, op=dist.ReduceOp.SUM, group=self.group)
                dist.all_reduce(self._qfa_state, op=dist.ReduceOp.SUM, group=self.group)
                ops.qfedavg_rows(self.partial.view(1, -1), None, None, self.global_flat, agg_out,
                                 ops.QFA_FINISH, P=self.P, state=self._qfa_state)
            if sopt is not None:
                sopt.step_vector(self.partial, self.global_flat)
        elif self.aggregator is None:
            if sopt is not None and not distributed and self._sparse is None \
                    and self._quant is None:
                sopt.step_rows(tr.params, self.w32, self.global_flat, self.rows)  # one launch
            else:
                if self._sparse is not None:  # the same sum from the (index, value) payload
                    from .sparse import sparse_fedavg
                    sparse_fedavg(self._sparse, self.w32, self.global_flat, self.partial,
                                  row_index=self.rows)
                elif self._quant is not None:  # ... and from the packed codes
                    from .quantpack import quant_fedavg
                    quant_fedavg(self._quant, self.w32, self.global_flat, self.partial,
                                 row_index=self.rows)
                else:
                    ops.fedavg_weighted_sum(tr.params, self.w32, self.partial,
                                            row_index=self.rows, P=self.P)
                if distributed:
                    dist.all_reduce(self.partial, op=dist.ReduceOp.SUM, group=self.group)
                if sopt is None:
                    self.global_flat.copy_(self.partial)
                else:
                    sopt.step_vector(self.partial, self.global_flat)
        else:  # one rank (checked at construction): the rule over this rank's rows
            self.aggregator.aggregate_packed(tr.params[:, :self.P], self._agg_samples,
                                             row_index=self._agg_rows, out=agg_out,
                                             **self._center_kw(self._agg_root))
            if sopt is not None:
                sopt.step_vector(self.partial, self.global_flat)
        if self.Q and not keep_bufs:
            ops.fedavg_weighted_sum(tr.bufs, self.w32, self.global_bufs, row_index=self.rows,
                                    P=self.Q)
            if distributed:
                dist.all_reduce(self.global_bufs, op=dist.ReduceOp.SUM, group=self.group)
        self.round_index += 1
        self._host_timing(_t)
        return metrics

    def _host_timing(self, _t):
        if _t:
            torch.cuda.synchronize(self.device)
            _t.append(time.perf_counter())
            print("round host ms: plan %.1f, run_round %.1f, dp/fedavg+sync %.1f" % tuple(
                1e3 * (b - a) for a, b in zip(_t, _t[1:])), file=sys.stderr)

    def evaluate(self, data, labels, template_model=None):
        """Eval-mode metrics of the current global model on a device-resident test set
        (fedhip/evaluate.py; LocalTrainer.evaluate_model's keys + 'loss')."""
        if self._evaluator is None:
            from .evaluate import GlobalEvaluator
            self._evaluator = GlobalEvaluator(template_model or self._template, self.device)
        return self._evaluator.evaluate(self.global_flat, self.global_bufs, data, labels,
                                        transform=self.transform)

    def _round_key(self, seed):
        """The round's Philox key, from the (secret by default) dp_seed."""
        return (self.dp_seed * 6364136223846793005 + seed * 1442695040888963407
                + self.round_index) & ((1 << 64) - 1)

    def _apply_dp(self, S, seed):
        """federated_trainer.py:434-462 for every client at once (budget bookkeeping is the
        caller's: privacy.py's tracker is host state)."""
        tr, dp = self.trainer, self.dp
        sq = ops.dp_delta_sqnorm(tr.params, self.global_flat.view(1, -1).expand(S, -1),
                                 tr.seg_offsets, S)
        total, coef, clipped, sigma = ops.dp_clip_coef(sq, dp.max_grad_norm, dp.epsilon, dp.delta)
        g = self.global_flat.view(1, -1).expand(S, -1)
        key = self._round_key(seed)
        ops.dp_apply(tr.params, g, tr.params, coef, clipped, sigma, P=self.P, seed=key,
                     row_ids=self.slot_ids[:S], noise=self.dp_noise)
        self.last_dp = (total, clipped, sigma)
