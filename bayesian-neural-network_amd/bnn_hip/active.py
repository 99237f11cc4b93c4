"""F10: pool-based active learning on the device -- what predictive's mutual_information ("epistemic, BALD") exists for.

A round is: train on the labelled subset, score the whole pool, take the k candidates the model is least sure about, grow
the subset.  The data set stays where it is (`epoch.DeviceDataset`): the subset is a list of row indices on the device
(`ActivePool.labelled`), its epoch order is bnn_epoch_permutation over its positions composed with that list
(bnn_acquire_compose), and bnn_epoch_stage gathers through the result -- no row is copied, and the graphed training step
is the one a full-data epoch replays.  Scoring runs the stacked predictive over the pool in identity order and writes one
number per row; the selection (bnn_acquire_topk) is one C entry that also updates the mask, the list and its count word.
The host keeps a mirror of the count (k and the initial rows are host values), so a round reads nothing back.
Semantics: include/bnn_hip.h F10.  Warm start only: the network is not re-initialised between rounds.

F15 (BatchBALD): instead of the k best per-row scores, ActivePool.joint_probs evaluates the pool once under weight draws
shared by every row and ActivePool.acquire_batchbald builds the batch greedily by its JOINT mutual information
(bnn_batchbald_joint, the same bnn_acquire_topk with k = 1, bnn_batchbald_extend); acquisition="batchbald" in ActiveLearner.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .capture import word32
from .epoch import DeviceDataset, DeviceLoader, EpochRunner, fill_rows
from .ops import BnnHipError
from .runtime import state, take_samples

ACQUISITIONS = ("bald", "entropy", "variance", "random")
BATCH_ACQUISITIONS = ("batchbald",)       # scored jointly over the batch (F15): joint_probs + acquire_batchbald, not score + acquire
_FIELD = {"bald": "mutual_information", "entropy": "predictive_entropy", "variance": "variance"}


def check_acquisition(net, acquisition: str):
    """Host-side refusals: an unknown name, an uncertainty score on a plain MLP (it has no predictive distribution), an
    entropy score on a regression network, a variance score on a classifier."""
    import networks
    if acquisition in BATCH_ACQUISITIONS:
        return check_joint(net)
    if acquisition not in ACQUISITIONS:
        raise BnnHipError(f"acquisition must be one of {ACQUISITIONS + BATCH_ACQUISITIONS}, got {acquisition!r}")
    if acquisition == "random":
        return
    if not isinstance(net, (networks.BayesianNetwork, networks.MLP_Dropout)):
        raise BnnHipError(f"acquisition {acquisition!r} needs a predictive distribution (BayesianNetwork or MLP_Dropout); "
                          f"{type(net).__name__} accepts only 'random'")
    want = "regression" if acquisition == "variance" else "classification"
    if net.mode != want:
        raise BnnHipError(f"acquisition {acquisition!r} is a {want} score; the network's mode is {net.mode!r}")


def check_joint(net):
    """Host-side refusals of the joint (BatchBALD) acquisition: it needs the SAME weight draw s for every row of the pool,
    which only weight-space noise gives -- a BayesianNetwork with local_reparam=False, classification, all samples here."""
    import networks
    from .flipout import FlipoutNetwork
    if isinstance(net, FlipoutNetwork):
        raise BnnHipError("batchbald: a Flipout network (FlipoutNetwork) draws its noise per row, not one weight draw shared "
                          "across rows; use the BayesianNetwork it views (local_reparam=False) or 'bald'")
    if isinstance(net, networks.MLP_Dropout):
        raise BnnHipError("batchbald: MLP_Dropout draws its masks per row, not one weight draw shared across rows; use 'bald'")
    if not isinstance(net, networks.BayesianNetwork):
        raise BnnHipError(f"batchbald needs a predictive distribution over shared weight draws (BayesianNetwork); "
                          f"{type(net).__name__} accepts only 'random'")
    if net.local_reparam:
        raise BnnHipError("batchbald: a local-reparameterisation network (BayesianLinearLR) draws its noise per row, not one "
                          "weight draw shared across rows; use local_reparam=False or 'bald'")
    if net.mode != "classification":
        raise BnnHipError(f"batchbald is a classification score; the network's mode is {net.mode!r}")
    if state.shard_samples:
        raise BnnHipError("batchbald: sample sharding splits the weight draws over ranks; every rank needs all of them")
    if state.host_eps or any(sp.m._eps_stubbed() for sp in net._specs()):
        raise BnnHipError("batchbald: host-drawn or injected epsilon is drawn afresh by every forward_mc call, so rows of "
                          "different calls would not share their weight draws; use the on-chip generator")


class JointProbs:
    """ActivePool.joint_probs' result: probs float32 [S, N, C] (draw s is the SAME weights for every row), cond and marg
    float64 [N] (the expected entropy and the entropy of the mean), first_sample (the global index of draw 0)."""

    def __init__(self, probs, cond, marg, first_sample):
        self.probs, self.cond, self.marg, self.first_sample = probs, cond, marg, first_sample


class BatchBaldResult:
    """ActivePool.acquire_batchbald's result, on the device: selected int32 [k] in the order chosen, batch_scores float64
    [k] (entry n - 1: the joint mutual information of the first n rows)."""

    def __init__(self, selected, batch_scores):
        self.selected, self.batch_scores = selected, batch_scores


class SubsetLoader(DeviceLoader):
    """DeviceLoader over the labelled subset of an ActivePool: the same protocol (iteration, begin_epoch / end_epoch /
    stage_args / example / batch_index / epoch), so an unchanged EpochRunner and tasks.*.train_step drive it.  len() is
    n_labelled // batch_size (drop_last) at the pool's CURRENT size; an epoch is one bnn_epoch_permutation over the
    n_labelled positions (the seed and epoch word of a DeviceLoader over the copied rows give the same minibatches), one
    bnn_acquire_compose, then the usual stage launches over the full data set.  A runner holds M and its beta table, so it
    is rebuilt after an acquisition; the graphed step is not."""

    def __init__(self, pool: "ActivePool", batch_size: int, shuffle: bool = True, seed: Optional[int] = None):
        self.pool, self.dataset, self.batch_size = pool, pool.dataset, int(batch_size)
        self.shuffle, self.drop_last = bool(shuffle), True
        if not 1 <= self.batch_size <= pool.n_labelled:
            raise BnnHipError(f"SubsetLoader: batch_size must lie in [1, {pool.n_labelled}] (the labelled rows)")
        self.seed = (state.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self._words = self._order = self._perm = None
        self._perm_args = (0, None)
        self._mid_epoch = False
        self._ahead = None              # ActiveLearner.prepare: the minibatch count of a coming round

    @property
    def num_batches(self):
        return self._ahead if self._ahead is not None else self.pool.n_labelled // self.batch_size

    def _state(self):
        if self._words is None:
            ops.require_device(self.dataset.x)
            dev, N = self.dataset.device, len(self.dataset)
            self._words = torch.zeros(4, dtype=torch.int32, device=dev)        # minibatch j, epoch e, ticket, (unused)
            self._order = torch.zeros(N, dtype=torch.int32, device=dev)
            self._perm = torch.zeros(N, dtype=torch.int32, device=dev)
        return self._words

    def begin_epoch(self, order=None):
        """As DeviceLoader.begin_epoch; `order` is a permutation of the subset's POSITIONS 0 .. n_labelled-1.  Always
        returns the int32 device order (rows of the full data set): an unshuffled pass walks the list as it grew."""
        w, n = self._state(), self.pool.n_labelled
        if self._mid_epoch:
            w[0:1].zero_()
            w[1:2].add_(1)
        self._mid_epoch = True
        if order is not None:
            order = torch.as_tensor(order)
            if order.numel() != n:
                raise BnnHipError("SubsetLoader: order must hold one entry per labelled row")
            self._perm[:n].copy_(order.reshape(-1), non_blocking=True)
        elif self.shuffle:
            if self._perm_args[0] != n:
                self._perm_args = (n, ops.epoch_perm_args(n_rows=n, seed=self.seed, epoch=w[1:2], order=self._perm[:n]))
            ops.epoch_permutation(self._perm_args[1])
        else:
            self._order[:n].copy_(self.pool.labelled)
            return self._order
        ops.acquire_compose(self.pool._labelled, self._perm, self._order, n)
        return self._order

    def stage_args(self, x_out, targets_out, shuffled: bool = True, **kw) -> L.EpochStageArgs:
        return super().stage_args(x_out, targets_out, True, **kw)      # the subset is always gathered through its order


class ActivePool:
    """The unlabelled pool of a DeviceDataset and the labelled subset grown from it: a uint8 candidate mask [N], the
    int32 list of labelled rows in the order they were added, its count as a device word and as a host mirror (the
    mirror never needs the device word: k and `initial` are host values and a short pool is refused on the host).
    len(pool) is the number of candidates left."""

    def __init__(self, dataset: DeviceDataset, initial):
        N = len(dataset)
        idx = np.asarray(torch.as_tensor(initial).cpu().numpy(), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= N):
            raise BnnHipError(f"ActivePool: initial rows must lie in [0, {N})")
        if np.unique(idx).size != idx.size:
            raise BnnHipError("ActivePool: initial rows must be distinct")
        self.dataset, self.device = dataset, dataset.device
        cand, lab = np.ones(N, np.uint8), np.zeros(N, np.int32)
        cand[idx] = 0
        lab[:idx.size] = idx
        self.candidate = torch.from_numpy(cand).to(self.device)
        self._labelled = torch.from_numpy(lab).to(self.device)
        self._words = torch.tensor([idx.size, 0], dtype=torch.int32, device=self.device)   # n_labelled, the last launch's winners
        self.n_labelled = int(idx.size)
        self.round = 0                  # acquisitions so far: word 1 of the random scores' counter
        self._workspace = self._xb = self._bb = None
        self._evals = {}

    def __len__(self):
        return len(self.dataset) - self.n_labelled

    @property
    def labelled(self) -> torch.Tensor:
        return self._labelled[:self.n_labelled]

    @property
    def n_labelled_word(self) -> torch.Tensor:
        return self._words[0:1]

    @property
    def n_selected_word(self) -> torch.Tensor:
        return self._words[1:2]

    def loader(self, batch_size: int, shuffle: bool = True, seed: Optional[int] = None) -> SubsetLoader:
        return SubsetLoader(self, batch_size, shuffle=shuffle, seed=seed)

    # ---- scoring
    def _fill(self, dst: torch.Tensor, a: int, b: int):
        """Rows a .. b-1 of the data set as fp32 into dst (epoch.fill_rows)."""
        fill_rows(self.dataset, dst, a, b)

    def _evaluator(self, net, G: int, B: int, samples: int):
        from .engine import GraphedPredictive
        key = (id(net), G, B, samples, state.math, state.form)
        ev = self._evals.get(key)
        if ev is None:
            x = torch.zeros((G, B, self.dataset.x.shape[1]), dtype=torch.float32, device=self.device)
            with torch.no_grad():
                ev = self._evals[key] = GraphedPredictive(net, x, samples, capture=False, stacked=True)
        return ev

    def score(self, net, samples, acquisition: str, chunk: int = 16) -> torch.Tensor:
        """float32 [N] on the device: one score per row of the data set (the mask is applied at selection).  "bald":
        mutual_information, "entropy": predictive_entropy, "variance": the per-row sum of the regression variance over the
        outputs, "random": bnn_acquire_random's uniforms for this pool's round.  Rows are scored in identity order in
        minibatches of the network's batch size -- BayesianNetwork: `chunk` minibatches per launch group of the stacked
        predictive; MLP_Dropout: its predictive per minibatch -- and minibatch g draws the MC-sample indices the g-th
        call of a per-minibatch `predictive` loop would.  A last minibatch short of rows is padded with zero rows whose
        scores are discarded."""
        import networks
        if acquisition in BATCH_ACQUISITIONS:
            raise BnnHipError(f"score: {acquisition!r} scores a batch jointly; use joint_probs and acquire_batchbald")
        check_acquisition(net, acquisition)
        N, d = self.dataset.x.shape
        ops.require_device(self.dataset.x)
        scores = torch.empty(N, dtype=torch.float32, device=self.device)
        if acquisition == "random":
            return ops.acquire_random(scores, state.seed, self.round)
        samples, B, field = int(samples), int(net.batch_size), _FIELD[acquisition]
        if samples < 1:
            raise BnnHipError("score: samples must be >= 1")
        nb = (N + B - 1) // B

        def take(p, a, b):
            v = getattr(p, field)
            if acquisition == "variance":
                v = v.sum(-1)
            scores[a:b].copy_(v.reshape(-1)[:b - a])

        with torch.no_grad():
            if isinstance(net, networks.BayesianNetwork):
                for g0 in range(0, nb, int(chunk)):
                    G = min(int(chunk), nb - g0)
                    a, b = g0 * B, min(N, (g0 + G) * B)
                    ev = self._evaluator(net, G, B, samples)
                    self._fill(ev.x.view(G * B, d), a, b)
                    ev.counter.fill_(word32(state.counter))             # where a predictive call made now would start
                    ev.replay()
                    take(ev._pred, a, b)
            else:
                if self._xb is None or self._xb.shape[0] != B:
                    self._xb = torch.empty((B, d), dtype=torch.float32, device=self.device)
                xin = self._xb.view(B, 1, 1, d) if net.mode == "classification" else self._xb
                for g in range(nb):
                    a, b = g * B, min(N, (g + 1) * B)
                    self._fill(self._xb, a, b)
                    take(net.predictive(xin, samples), a, b)
        return scores

    # ---- selection
    def acquire(self, scores: torch.Tensor, k: int) -> torch.Tensor:
        """One bnn_acquire_topk launch: the k candidates with the highest scores (ties to the lower row, NaN last) leave
        the pool and join the labelled list.  Returns the device int32 [k] of their rows, best first."""
        k = int(k)
        if not 1 <= k <= L.ACQUIRE_MAX_K:
            raise BnnHipError(f"acquire: k must lie in [1, {L.ACQUIRE_MAX_K}] (BNN_ACQUIRE_MAX_K)")
        if k > len(self):
            raise BnnHipError(f"acquire: k = {k} but only {len(self)} candidates are left in the pool")
        if scores.numel() != len(self.dataset):
            raise BnnHipError("acquire: one score per row of the data set")
        if self._workspace is None:
            self._workspace = ops.acquire_topk_workspace(self.device)
        selected = torch.empty(k, dtype=torch.int32, device=self.device)
        ops.acquire_topk(ops.acquire_topk_args(scores=scores, candidate=self.candidate, k=k, selected=selected,
                                               labelled=self._labelled, n_labelled=self._words[0:1],
                                               n_selected=self._words[1:2], workspace=self._workspace))
        self.n_labelled += k
        self.round += 1
        return selected

    # ---- BatchBALD (F15)
    def joint_probs(self, net, samples, rows_per_call: int = 4096) -> JointProbs:
        """The pool's class probabilities under `samples` weight draws SHARED by every row: the rows are evaluated in identity
        order, `rows_per_call` per forward_mc, and the sample counter is rewound to the same first index before every call
        (weight-space epsilon does not depend on x), left at first + samples after the last.  bnn_batchbald_probs turns each
        call's logits into its rows of probs and the two per-row entropies."""
        check_joint(net)
        S, R = int(samples), int(rows_per_call)
        if not 1 <= S <= L.BATCHBALD_MAX_SAMPLES:
            raise BnnHipError(f"joint_probs: samples must lie in [1, {L.BATCHBALD_MAX_SAMPLES}] (BNN_BATCHBALD_MAX_SAMPLES)")
        if R < 1:
            raise BnnHipError("joint_probs: rows_per_call must be >= 1")
        Cc = int(net.classes)
        if not 2 <= Cc <= L.BATCHBALD_MAX_CLASSES:
            raise BnnHipError(f"joint_probs: classes must lie in [2, {L.BATCHBALD_MAX_CLASSES}] (BNN_BATCHBALD_MAX_CLASSES)")
        N, d = self.dataset.x.shape
        ops.require_device(self.dataset.x)
        probs = torch.empty((S, N, Cc), dtype=torch.float32, device=self.device)
        cond = torch.empty(N, dtype=torch.float64, device=self.device)
        marg = torch.empty(N, dtype=torch.float64, device=self.device)
        xb = torch.empty((min(R, N), d), dtype=torch.float32, device=self.device)
        first = take_samples(S)
        with torch.no_grad():
            for a in range(0, N, R):
                b = min(N, a + R)
                self._fill(xb[:b - a], a, b)
                state.counter = first
                logits = net.forward_mc(xb[:b - a], S)
                ops.batchbald_probs(logits.contiguous(), probs, cond, marg, a)
        return JointProbs(probs, cond, marg, first)

    def acquire_batchbald(self, joint: JointProbs, k: int, max_configs: int = 8192, seed: Optional[int] = None) -> BatchBaldResult:
        """A batch of k candidates by greedy BatchBALD: bnn_batchbald_begin, then k times bnn_batchbald_joint (every row scored
        together with the rows chosen so far), bnn_acquire_topk with k = 1 (the mask, the list and the count word as in
        acquire) and bnn_batchbald_extend (the k-th one only books base and batch_scores).  Every label configuration of the chosen rows is enumerated while there are at
        most `max_configs` of them, then `max_configs` importance-sampled ones stand in (`seed`: their Philox key, default
        the runtime's seed; the pool's round is in the counter).  Nothing is read back."""
        k, mc = int(k), int(max_configs)
        if not 1 <= k <= L.BATCHBALD_MAX_K:
            raise BnnHipError(f"acquire_batchbald: k must lie in [1, {L.BATCHBALD_MAX_K}] (BNN_BATCHBALD_MAX_K)")
        if not 1 <= mc <= L.BATCHBALD_MAX_CONFIGS:
            raise BnnHipError(f"acquire_batchbald: max_configs must lie in [1, {L.BATCHBALD_MAX_CONFIGS}] (BNN_BATCHBALD_MAX_CONFIGS)")
        if k > len(self):
            raise BnnHipError(f"acquire_batchbald: k = {k} but only {len(self)} candidates are left in the pool")
        S, N, Cc = joint.probs.shape
        if N != len(self.dataset):
            raise BnnHipError("acquire_batchbald: one row of probabilities per row of the data set")
        ops.require_device(joint.probs)
        seed = state.seed if seed is None else int(seed)
        dev, cap = self.device, ops.batchbald_configs(Cc, k - 1, mc)          # the last extend writes no state
        key = (S, N, Cc, cap)
        if self._bb is None or self._bb[0] != key:
            f64 = dict(dtype=torch.float64, device=dev)
            self._bb = (key, dict(
                phat=[torch.empty((cap, S), dtype=torch.float32, device=dev) for _ in range(2)],
                expo=[torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2)],
                weight=torch.empty(cap, **f64), offset=torch.empty(cap, **f64), base=torch.empty(1, **f64),
                scores=torch.empty(N, dtype=torch.float32, device=dev), scores64=torch.empty(N, **f64),
                workspace=ops.batchbald_joint_workspace(N, Cc, cap, dev)))
        b = self._bb[1]
        if self._workspace is None:
            self._workspace = ops.acquire_topk_workspace(dev)
        selected = torch.empty(k, dtype=torch.int32, device=dev)
        batch_scores = torch.empty(k, dtype=torch.float64, device=dev)

        def st(n):                        # the state of n chosen rows lives in half n & 1
            return ops.batchbald_state_args(
                probs=joint.probs, cond=joint.cond, labelled=self._labelled, n_labelled=self._words[0:1],
                phat_in=b["phat"][(n + 1) & 1], expo_in=b["expo"][(n + 1) & 1], phat_out=b["phat"][n & 1], expo_out=b["expo"][n & 1],
                weight=b["weight"], offset=b["offset"], base=b["base"], max_configs=mc, n_chosen=n, round=self.round, seed=seed,
                scores64=b["scores64"], batch_scores=batch_scores if n else None, last=n == k)

        ops.batchbald_begin(st(0))
        for n in range(1, k + 1):
            ops.batchbald_joint(ops.batchbald_joint_args(
                probs=joint.probs, phat=b["phat"][(n - 1) & 1], weight=b["weight"], offset=b["offset"], cond=joint.cond,
                base=b["base"], scores=b["scores"], scores64=b["scores64"], n_configs=ops.batchbald_configs(Cc, n - 1, mc),
                workspace=b["workspace"]))
            ops.acquire_topk(ops.acquire_topk_args(scores=b["scores"], candidate=self.candidate, k=1, selected=selected[n - 1:n],
                                                   labelled=self._labelled, n_labelled=self._words[0:1],
                                                   n_selected=self._words[1:2], workspace=self._workspace))
            ops.batchbald_extend(st(n))
        self.n_labelled += k
        self.round += 1
        return BatchBaldResult(selected, batch_scores)


class ActiveLearner:
    """Rounds of pool-based active learning on one of the six bnn_hip.tasks wrappers: round() = `epochs_per_round` x
    task.train_step(pool's loader), pool.score, pool.acquire -- with acquisition="batchbald" (BATCH_ACQUISITIONS)
    pool.joint_probs and pool.acquire_batchbald(k, max_configs) in their place.  `samples` defaults to the task's
    test_samples; the plain MLP wrappers accept only acquisition="random".

    A round enqueues work and does not synchronise (classification tasks; the regression wrappers read their epoch loss
    once per train_step).  What a new subset size needs from the host -- an EpochRunner with its beta table, 4 M bytes
    uploaded -- is built by prepare(rounds) ahead of the rounds that use it; run() calls it, and round() falls back to it."""

    def __init__(self, task, pool: ActivePool, k: int, acquisition: str = "bald", samples: Optional[int] = None,
                 epochs_per_round: int = 1, batch_size: Optional[int] = None, chunk: int = 16, seed: Optional[int] = None,
                 max_configs: int = 8192):
        check_acquisition(task.net, acquisition)
        self.task, self.pool, self.k, self.acquisition = task, pool, int(k), acquisition
        self.max_configs = int(max_configs)
        if not 1 <= self.k <= L.ACQUIRE_MAX_K:
            raise BnnHipError(f"ActiveLearner: k must lie in [1, {L.ACQUIRE_MAX_K}] (BNN_ACQUIRE_MAX_K)")
        self.samples = int(samples if samples is not None else getattr(task, "test_samples", 0) or 0)
        if acquisition != "random" and self.samples < 1:
            raise BnnHipError("ActiveLearner: samples (or the task's test_samples) must be >= 1")
        if acquisition in BATCH_ACQUISITIONS and (self.k > L.BATCHBALD_MAX_K or self.samples > L.BATCHBALD_MAX_SAMPLES):
            raise BnnHipError(f"ActiveLearner: {acquisition!r} takes k in [1, {L.BATCHBALD_MAX_K}] (BNN_BATCHBALD_MAX_K) and samples "
                              f"in [1, {L.BATCHBALD_MAX_SAMPLES}] (BNN_BATCHBALD_MAX_SAMPLES)")
        self.epochs_per_round, self.chunk = int(epochs_per_round), int(chunk)
        self.loader = pool.loader(int(batch_size if batch_size is not None else task.batch_size), seed=seed)
        self._runners = {}
        self.accuracy: List[float] = []

    def prepare(self, rounds: int = 1):
        """The runners of the next `rounds` rounds' subset sizes (one per distinct minibatch count)."""
        ld = self.loader
        step = self.task._step_for(*ld.example())
        for r in range(int(rounds)):
            M = (self.pool.n_labelled + r * self.k) // ld.batch_size
            if M not in self._runners:
                ld._ahead = M
                try:
                    self._runners[M] = EpochRunner(step, ld)
                finally:
                    ld._ahead = None

    def round(self) -> torch.Tensor:
        self.prepare(1)
        self.task._runners[id(self.loader)] = self._runners[len(self.loader)]
        for _ in range(self.epochs_per_round):
            self.task.train_step(self.loader)
        if self.acquisition in BATCH_ACQUISITIONS:
            joint = self.pool.joint_probs(self.task.net, self.samples)
            return self.pool.acquire_batchbald(joint, self.k, self.max_configs).selected
        scores = self.pool.score(self.task.net, self.samples, self.acquisition, self.chunk)
        return self.pool.acquire(scores, self.k)

    def run(self, rounds: int, test_loader=None) -> List[torch.Tensor]:
        """`rounds` rounds; returns their `selected` tensors.  With a test loader the task's accuracy after each round is
        appended to `.accuracy` (epoch.evaluate: one read per round)."""
        self.prepare(rounds)
        out = []
        for _ in range(int(rounds)):
            out.append(self.round())
            if test_loader is not None:
                self.task.evaluate(test_loader)
                self.accuracy.append(self.task.acc)
        return out
