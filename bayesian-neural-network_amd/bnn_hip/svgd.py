"""F23: Stein variational gradient descent (Liu & Wang 2016) and the weight-space repulsive ensemble kde-WGD (D'Angelo & Fortuin
2021; neither is in the reference) on the members of a DeepEnsemble (csrc/svgd.hip; include/bnn_hip.h F23).

`SteinTransform` sits between the last bnn_ens_bwd and the optimiser's launch of ensemble.EnsembleTrainStep and rewrites the
gradient bucket in place into the direction the optimiser subtracts,

    d = A g + B theta      per parameter column, A and B two M x M matrices formed from the members' pairwise distances,

in three launches: bnn_svgd_dist (per-chunk sums of squared differences of every pair), bnn_svgd_coef (one fp64 block: D2, its
median, the bandwidth, the kernel matrix, [A | B]) and bnn_svgd_direction ([A | B] . [g ; theta] on the fp32 matrix core).
Everything stays on the device; `read()` copies the small fp64 record back for watching a collapse.

The prior enters through `prior_precision` (B carries tau' = prior_precision / temperature): build the optimiser with
weight_decay = 0, or the prior is counted twice.  The optimiser is the unchanged FusedSGD / FusedAdam(capturable=True); Adam on
the Stein direction is what the SVGD paper's code does with AdaGrad."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops import BnnHipError

METHODS = {"svgd": L.SVGD_SVGD, "wgd": L.SVGD_WGD}


class SteinRecord(NamedTuple):
    """bnn_svgd_coef's record of the last enqueue: D2 [M, M] (squared distances), their median, the bandwidth h used and the
    kernel's row sums r [M] (r_i -> M as member i collapses onto the others, -> 1 as it drifts away)."""
    D2: np.ndarray
    median: float
    h: float
    r: np.ndarray


class SteinTransform:
    def __init__(self, ens, *, dataset_size, batch_size, prior_precision: float = 1.0, temperature: float = 1.0,
                 method: str = "svgd", bandwidth: Optional[float] = None):
        """`ens`: the DeepEnsemble whose members are the particles.  grad U_j = s g_j + tau' theta_j with s = dataset_size /
        (batch_size temperature), tau' = prior_precision / temperature and g_j the gradient of the step's SUM loss.
        `method`: "svgd" or "wgd" (kde-WGD: the repulsion normalised per member, the gradients not mixed).  `bandwidth`: the
        RBF kernel's h in k = exp(-D2 / h); None: the median heuristic h = median(D2) / log(M + 1), re-formed every step."""
        M = int(ens.members)
        if M > L.SVGD_MAX_MEMBERS:
            raise BnnHipError(f"SteinTransform: at most {L.SVGD_MAX_MEMBERS} members, got {M}")
        if method not in METHODS:
            raise BnnHipError(f"SteinTransform: method must be one of {tuple(METHODS)}, got {method!r}")
        if int(dataset_size) < 1 or int(batch_size) < 1:
            raise BnnHipError("SteinTransform: dataset_size and batch_size must be >= 1")
        if not (float(prior_precision) >= 0.0 and math.isfinite(float(prior_precision))):
            raise BnnHipError(f"SteinTransform: prior_precision must be >= 0, got {prior_precision!r}")
        if not (float(temperature) > 0.0 and math.isfinite(float(temperature))):
            raise BnnHipError(f"SteinTransform: temperature must be > 0, got {temperature!r}")
        if bandwidth is not None and not (float(bandwidth) > 0.0 and math.isfinite(float(bandwidth))):
            raise BnnHipError(f"SteinTransform: bandwidth must be > 0 (None: the median heuristic), got {bandwidth!r}")
        bank = ens.bank
        ops.require_device(bank.buffer)
        self.ens, self.members, self.method = ens, M, method
        self.grad_scale = float(dataset_size) / (float(batch_size) * float(temperature))
        self.tau = float(prior_precision) / float(temperature)
        self.bandwidth = None if bandwidth is None else float(bandwidth)
        self.stride = int(bank.stride)
        self.chunks = ops.svgd_chunks(self.stride)
        dev = bank.buffer.device
        self.partials = torch.zeros((self.chunks, max(1, M * (M - 1) // 2)), dtype=torch.float32, device=dev)
        self.coef = torch.zeros((M, 2 * M), dtype=torch.float32, device=dev)
        self.record = torch.zeros((L.svgd_record_doubles(M),), dtype=torch.float64, device=dev)
        self.launches = 3

    def _check(self, bank, bucket):
        M = self.members
        buf = bank.buffer if hasattr(bank, "buffer") else bank
        ops.require_device(buf, bucket)
        if buf.dim() != 2 or buf.shape[0] < M:
            raise BnnHipError(f"SteinTransform: the bank holds {buf.shape[0] if buf.dim() == 2 else 0} members, {M} are needed")
        if buf.shape[1] != self.stride or tuple(bucket.shape) != (M, self.stride):
            raise BnnHipError(f"SteinTransform: the bank and the bucket must be [{M}, {self.stride}] in the bank's layout")
        return buf

    def enqueue(self, bank, bucket: torch.Tensor):
        """The three launches on the current stream: `bucket` ([M, stride], the members' gradients in the bank's layout) becomes
        A g + B theta in place; `bank` (a WeightBank or its buffer) is only read."""
        buf = self._check(bank, bucket)
        M = self.members
        ops.svgd_dist(buf, self.partials, members=M)
        ops.svgd_coef(self.partials, self.coef, self.record, members=M, chunks=self.chunks, grad_scale=self.grad_scale,
                      tau=self.tau, method=METHODS[self.method], bandwidth=0.0 if self.bandwidth is None else self.bandwidth)
        ops.svgd_direction(self.coef, buf, bucket, members=M)
        return bucket

    def read(self) -> SteinRecord:
        """The record of the last enqueue (or replay of a captured step), one device-to-host copy."""
        M = self.members
        rec = self.record.cpu().numpy()
        n = M * M
        return SteinRecord(rec[:n].reshape(M, M).copy(), float(rec[n]), float(rec[n + 1]), rec[n + 2:n + 2 + M].copy())
