"""Secure aggregation beside FedAvg: the server only ever sees masked rows and their sum.

The reference repository has only the plain weighted mean (src/aggregation/fedavg.py), which
reads every client's update in the clear.  SecureAggregator follows the pairwise-masking scheme
of Bonawitz et al. (CCS 2017): a client encodes fl32(w_k * x_k) in fixed point in the ring
Z/2^32, adds one pseudorandom mask per peer (the pair's other member subtracts the same mask)
and optionally a self mask; the sum of the masked rows is the sum of the encodings, because the
pair masks cancel.  When clients drop out after masking, the masks between a surviving and a
dropped client are left over and the server removes them.  Both stages run on HIP
(csrc/secagg.hip: fh_secagg_encode_mask_rows, fh_secagg_sum_decode); the arithmetic is defined
in include/fedhip.h and DESIGN.md §5.

This is a ONE-PROCESS SIMULATION of the protocol's arithmetic: every key is derived here from
`session_seed`, so the process that plays the server also holds every client's keys.  Key
agreement between clients and the secret sharing that lets the server rebuild a dropped
client's keys are host-side protocol and are not part of it.

Like the robust rules it replaces FedAvgAggregator's reduction and nothing else.
"""
from __future__ import annotations

import logging
import secrets
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from fedhip import ops

from ..shared.models import ModelUpdate, ModelWeights
from .fedavg import FedAvgAggregator, FedAvgError

logger = logging.getLogger(__name__)

MASK64 = 0xFFFFFFFFFFFFFFFF
MAX_TERMS = 64  # mask terms per row in one fh_secagg_encode_mask_rows launch


def philox4x32_10(seed: int, hi: int, lo: int) -> Tuple[int, int, int, int]:
    """One Philox4x32-10 block on the host (Salmon et al., SC'11), with the counter / key
    layout of Philox::gen in csrc/fh_common.h; plain Python integers."""
    m32 = 0xFFFFFFFF
    seed, hi, lo = seed & MASK64, hi & MASK64, lo & MASK64
    c0, c1, c2, c3 = lo & m32, lo >> 32, hi & m32, hi >> 32
    k0, k1 = seed & m32, seed >> 32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m32, (p0 >> 32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


class SecureAggregator(FedAvgAggregator):
    """FedAvg computed from pairwise-masked fixed-point rows.

    ``mask`` is the clients' side (all of them, simulated in one launch), ``unmask_sum`` the
    server's; ``aggregate_packed`` / ``aggregate_updates`` are one after the other with nobody
    dropped.  `frac_bits` fractional bits; a client's weighted coordinate saturates at
    qmax * 2^-frac_bits with qmax = (2^31 - 1) // C, so a sum of C saturated values cannot
    wrap; `last_clipped` (int32 per client) counts the coordinates that saturated or were NaN.
    `nonce` is the round counter the masks are drawn under: ``mask`` uses it and advances it.
    """

    def __init__(self, frac_bits: int = 16, session_seed: Optional[int] = None,
                 self_masks: bool = False, min_clients: int = 2,
                 max_clients: Optional[int] = None, validate_updates: bool = True,
                 device: Optional[torch.device] = None):
        if not 0 <= int(frac_bits) <= 30:
            raise ValueError(f"frac_bits must be in [0, 30]: {frac_bits}")
        super().__init__(min_clients, max_clients, validate_updates, device)
        self.frac_bits = int(frac_bits)
        self.session_seed = (secrets.randbits(64) if session_seed is None
                             else int(session_seed)) & MASK64
        self.self_masks = bool(self_masks)
        self.nonce = 0
        self.last_clipped: Optional[torch.Tensor] = None
        self._last = None  # what unmask_sum needs to know about the last mask call

    # ------------------------------------------------------------------ keys
    def pair_key(self, a: int, b: int) -> int:
        """The key clients a < b (global ids) share; stands in for a Diffie-Hellman agreed
        key.  uint64 r0 | r1 << 32 of Philox(seed = session_seed, hi = a, lo = b)."""
        a, b = int(a), int(b)
        if not 0 <= a < b <= MASK64:
            raise ValueError(f"pair_key needs 0 <= a < b < 2^64: {a}, {b}")
        r = philox4x32_10(self.session_seed, a, b)
        return r[0] | r[1] << 32

    def self_key(self, a: int) -> int:
        """Client a's own mask key: likewise from (hi = 2^64 - 1, lo = a)."""
        r = philox4x32_10(self.session_seed, MASK64, int(a))
        return r[0] | r[1] << 32

    @staticmethod
    def qmax(num_clients: int) -> int:
        return (2 ** 31 - 1) // int(num_clients)

    def client_terms(self, ids: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
        """(keys uint64 [C, T], signs int32 [C, T]) each client adds to its row: + the mask of
        pair (a, b) when a < b, - when a > b; with self_masks + its self mask.  T = C - 1
        (+ 1), at least 1."""
        C = len(ids)
        T = max(1, C - 1 + int(self.self_masks))
        keys = np.zeros((C, T), dtype=np.uint64)
        signs = np.zeros((C, T), dtype=np.int32)
        pk = {}
        for i, a in enumerate(ids):
            t = 0
            for b in ids:
                if b == a:
                    continue
                lo, hi = min(a, b), max(a, b)
                if (lo, hi) not in pk:
                    pk[(lo, hi)] = self.pair_key(lo, hi)
                keys[i, t], signs[i, t] = pk[(lo, hi)], 1 if a < b else -1
                t += 1
            if self.self_masks:
                keys[i, t], signs[i, t] = self.self_key(a), 1
        return keys, signs

    def server_terms(self, survivors: Sequence[int],
                     dropped: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
        """What is left in the survivors' sum: for survivor s and dropped d the mask of their
        pair with the sign s gave it, and the survivors' self masks."""
        keys, signs = [], []
        for s in survivors:
            for d in dropped:
                keys.append(self.pair_key(min(s, d), max(s, d)))
                signs.append(1 if s < d else -1)
            if self.self_masks:
                keys.append(self.self_key(s))
                signs.append(1)
        return np.array(keys, dtype=np.uint64), np.array(signs, dtype=np.int32)

    # ------------------------------------------------------------------ the two stages
    def mask(self, packed: torch.Tensor, num_samples: Sequence[int],
             client_ids: Optional[Sequence[int]] = None,
             row_index: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The clients' side.  Client k (global id client_ids[k], default k) holds row
        row_index[k] (default k) of `packed` and weighs it by FedAvg's fp32 n_k / N.
        Returns (masked int32 [C, P], clipped int32 [C]); row k of `masked` is what client k
        would send.  Uses the current `nonce` and advances it."""
        ns = [int(n) for n in num_samples]
        if not ns:
            raise FedAvgError("No updates to aggregate")
        return self._mask_rows(packed, self._calculate_sample_weights_n(ns), ns, client_ids,
                               row_index)

    def _mask_rows(self, packed, weights, samples, client_ids, row_index):
        C = len(weights)
        ids = list(range(C)) if client_ids is None else [int(i) for i in client_ids]
        if len(ids) != C or len(set(ids)) != C:
            raise FedAvgError(f"client_ids must be {C} distinct ids")
        if C - 1 + int(self.self_masks) > MAX_TERMS:
            raise FedAvgError(f"SecureAggregator masks at most {MAX_TERMS + 1 - self.self_masks}"
                              f" clients per call: {C}")
        dev = packed.device
        idx = None
        if row_index is not None:
            host = [int(i) for i in row_index]
            if len(host) != C:
                raise FedAvgError("row_index and num_samples differ in length")
            idx = torch.tensor(host, dtype=torch.int32, device=dev)
        elif packed.shape[0] != C:
            raise FedAvgError(f"{packed.shape[0]} rows for {C} clients and no row_index")
        keys, signs = self.client_terms(ids)
        P = packed.shape[1]
        masked = torch.empty(C, P, dtype=torch.int32, device=dev)
        clipped = torch.zeros(C, dtype=torch.int32, device=dev)
        nonce = self.nonce
        ops.secagg_encode_mask_rows(
            packed, masked, self.frac_bits, self.qmax(C),
            term_keys=torch.from_numpy(keys.view(np.int64)).to(dev),
            term_signs=torch.from_numpy(signs).to(dev), nonce=nonce,
            weights=torch.tensor(weights, dtype=torch.float32, device=dev), row_index=idx,
            clipped=clipped)
        self.nonce = (nonce + 1) & MASK64
        self._last = {"ids": ids, "samples": samples, "nonce": nonce}
        self.last_clipped = clipped
        counts = clipped.cpu().numpy()
        if counts.any():
            logger.warning("secure aggregation: %d coordinates of %d clients were NaN or beyond "
                           "+-%g and were clipped", int(counts.sum()),
                           int(np.count_nonzero(counts)), self.qmax(C) * 2.0 ** -self.frac_bits)
        return masked, clipped

    def unmask_sum(self, masked: torch.Tensor, survivors: Sequence[int],
                   dropped: Sequence[int] = (), out: Optional[torch.Tensor] = None
                   ) -> torch.Tensor:
        """The server's side, for the rows of the last ``mask`` call.  `survivors` / `dropped`
        are client ids of that call: the survivors' rows are summed, the masks their pairs with
        the dropped clients left behind (and their self masks) are removed and the sum is
        decoded to fp32.  With `dropped` non-empty the row is then multiplied once in fp32 by
        fl32(N / N_S) (N: every client's samples, N_S: the survivors'), which makes it the
        survivors' FedAvg."""
        if self._last is None:
            raise FedAvgError("unmask_sum needs a mask call before it")
        ids = self._last["ids"]
        pos = {c: i for i, c in enumerate(ids)}
        surv, drop = [int(s) for s in survivors], [int(d) for d in dropped]
        if not surv:
            raise FedAvgError("No surviving clients to aggregate")
        if sorted(surv + drop) != sorted(ids):
            raise FedAvgError("survivors and dropped must partition the masked clients")
        if masked.shape[0] != len(ids):
            raise FedAvgError(f"{masked.shape[0]} masked rows for {len(ids)} clients")
        dev = masked.device
        idx = None if not drop and surv == ids else \
            torch.tensor([pos[s] for s in surv], dtype=torch.int32, device=dev)
        keys, signs = self.server_terms(surv, drop)
        kt = st = None
        if len(keys):
            kt = torch.from_numpy(keys.view(np.int64)).to(dev)
            st = torch.from_numpy(signs).to(dev)
        P = masked.shape[1]
        if out is None:
            out = torch.empty(P, dtype=torch.float32, device=dev)
        if not drop:
            ops.secagg_sum_decode(masked, self.frac_bits, kt, st, self._last["nonce"],
                                  row_index=idx, out=out)
            return out
        samples = self._last["samples"]
        if samples is None:
            raise FedAvgError("recovery from dropped clients needs the sample counts of mask()")
        n_all = sum(samples)
        n_s = sum(samples[pos[s]] for s in surv)
        if n_s <= 0:
            raise FedAvgError("the surviving clients hold no samples")
        row = torch.empty(1, P, dtype=torch.float32, device=dev)
        ops.secagg_sum_decode(masked, self.frac_bits, kt, st, self._last["nonce"], row_index=idx,
                              out=row)
        # one rounded fp32 multiply per coordinate, by the FedAvg kernel over the single row
        scale = torch.tensor([n_all / n_s], dtype=torch.float32, device=dev)
        return ops.fedavg_weighted_sum(row, scale, out, P=P)

    # ------------------------------------------------------------------ FedAvgAggregator's hooks
    def aggregate_packed(self, packed: torch.Tensor, num_samples: Sequence[int],
                         row_index: Optional[Sequence[int]] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """FedAvg of client rows already on the device ([clients, P] fp32), through the masked
        rows: ``mask``, then ``unmask_sum`` with every client surviving."""
        masked, _ = self.mask(packed, num_samples, row_index=row_index)
        return self.unmask_sum(masked, self._last["ids"], out=out)

    def _weighted_average(self, updates: List[ModelUpdate], weights: List[float]) -> ModelWeights:
        rows, names, offs, sizes = self._pack_updates(updates)
        masked, _ = self._mask_rows(rows, list(weights), None, None, None)
        out = self.unmask_sum(masked, self._last["ids"])
        return self._unpack_row(out, updates[0].model_weights, names, offs, sizes)


def create_secure_aggregator(**kwargs) -> SecureAggregator:
    return SecureAggregator(**kwargs)
