"""F8: the supervised tasks' epoch loop (classification/class_task.py:67-79, regression/reg_task.py:60-74) with the data
loader on the device.

The reference walks a CPU DataLoader(shuffle=True, drop_last=True): per step a host shuffle and collate, a host-to-device
copy, a host-computed beta.  Here the data set lives on the device (`DeviceDataset`), the epoch's permutation is drawn
there (bnn_epoch_permutation) and one launch per minibatch (bnn_epoch_stage) gathers its rows into the training step's
own static buffers -- x, its bf16 copy, the targets -- looks beta up in a device table and files the previous step's
loss words; the step's graph replay follows.  The minibatch and epoch numbers are device words, so `run_epoch` reads
nothing back and never synchronises.  Semantics: include/bnn_hip.h F8; the permutation comes from its own Philox stream
(counter words (.., 2, 1)), which shares no counter with epsilon or with the bandit's streams.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .capture import word32
from .ops import BnnHipError
from .runtime import state


def beta_table(num_batches: int) -> np.ndarray:
    """float32 [M]: beta_j = 2^(M-(j+1)) / (2^M - 1) (class_task.py:70, reg_task.py:63) in exact Python integers and true
    division, rounded once to fp32 -- the value GraphedTrainStep.step hands its device word."""
    M = int(num_batches)
    return np.asarray([2 ** (M - (j + 1)) / (2 ** M - 1) for j in range(M)], dtype=np.float64).astype(np.float32)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class DeviceDataset:
    """(x, y) held on the device.  x: uint8 (converted as u / 255 when staged: torchvision's ToTensor) or float32, [N, ...]
    -- image shapes are flattened to [N, d] as flat_input / BayesianNetwork.forward flatten them, and minibatches are
    handed out in the original item shape; y: int64 labels [N] or float32 targets [N, ...] (flattened to [N, k])."""

    def __init__(self, x, y, device=None):
        x, y = torch.as_tensor(x), torch.as_tensor(y)
        if x.dtype not in (torch.uint8, torch.float32):
            raise BnnHipError(f"DeviceDataset: x must be uint8 or float32, got {x.dtype}")
        if x.dim() < 2 or x.shape[0] < 1 or x.shape[0] != y.shape[0]:
            raise BnnHipError("DeviceDataset: x must be [N, ...] and y must have N entries")
        if x.shape[0] > L.EPOCH_MAX_ROWS:
            raise BnnHipError(f"DeviceDataset: at most {L.EPOCH_MAX_ROWS} rows (BNN_EPOCH_MAX_ROWS)")
        if y.dtype == torch.int64:
            if y.dim() != 1:
                raise BnnHipError("DeviceDataset: int64 labels must be [N]")
        elif y.dtype != torch.float32 or y.dim() < 2:
            raise BnnHipError("DeviceDataset: y must be int64 labels [N] or float32 targets [N, ...]")
        dev = torch.device(device) if device is not None else (x.device if x.is_cuda else _default_device())
        N = x.shape[0]
        self.item_shape, self.target_shape = tuple(x.shape[1:]), tuple(y.shape[1:])
        self.x = x.to(dev).reshape(N, -1).contiguous()
        self.y = (y.to(dev) if y.dtype == torch.int64 else y.to(dev).reshape(N, -1)).contiguous()
        self.device = dev

    def __len__(self):
        return self.x.shape[0]


class DeviceLoader:
    """The reference's DataLoader over a DeviceDataset.  len() is the number of minibatches M; iterating yields device
    (x, y) minibatches of the reference's shapes (x float32 [B, *item_shape]) in the loader's order, a fresh order per
    pass when shuffle=True (epoch e of a loader with `seed`: include/bnn_hip.h F8).  N % batch_size != 0 needs
    drop_last=True: a short last minibatch would need a second step object (as the bandit's buffer_size % batch_size)."""

    def __init__(self, dataset: DeviceDataset, batch_size: int, shuffle: bool = True, drop_last: bool = True,
                 seed: Optional[int] = None):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        N = len(dataset)
        if not 1 <= self.batch_size <= N:
            raise BnnHipError(f"DeviceLoader: batch_size must lie in [1, {N}]")
        if N % self.batch_size and not self.drop_last:
            raise BnnHipError("DeviceLoader: the data set's rows must be a multiple of batch_size, or drop_last=True "
                              "(a short last minibatch needs a second step object)")
        self.num_batches = N // self.batch_size
        self.seed = (state.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self._words = self._order = self._perm = None
        self._mid_epoch = False

    def __len__(self):
        return self.num_batches

    # ---- device state
    def _state(self):
        if self._words is None:
            ops.require_device(self.dataset.x)
            dev = self.dataset.device
            self._words = torch.zeros(4, dtype=torch.int32, device=dev)        # minibatch j, epoch e, ticket, (unused)
            self._order = torch.zeros(len(self.dataset), dtype=torch.int32, device=dev)
            self._perm = ops.epoch_perm_args(n_rows=len(self.dataset), seed=self.seed, epoch=self._words[1:2], order=self._order)
        return self._words

    @property
    def batch_index(self):
        return self._state()[0:1]

    @property
    def epoch(self):
        return self._state()[1:2]

    def begin_epoch(self, order=None):
        """Start a pass: rewinds a pass that was abandoned half-way, then settles the order -- `order` (a permutation of
        the rows, e.g. torch.randperm drawn with the reference loader's generator) copied to the device, else a drawn
        permutation (shuffle=True), else None (the identity).  Returns the int32 device order or None."""
        w = self._state()
        if self._mid_epoch:
            w[0:1].zero_()
            w[1:2].add_(1)
        self._mid_epoch = True
        if order is not None:
            order = torch.as_tensor(order)
            if order.numel() != len(self.dataset):
                raise BnnHipError("DeviceLoader: order must hold one entry per row")
            self._order.copy_(order.reshape(-1), non_blocking=True)
            return self._order
        if self.shuffle:
            ops.epoch_permutation(self._perm)
            return self._order
        return None

    def end_epoch(self):
        self._mid_epoch = False

    def stage_args(self, x_out, targets_out, shuffled: bool, **kw) -> L.EpochStageArgs:
        """bnn_epoch_stage's argument block for these destinations, on this loader's words and order."""
        w, ds = self._state(), self.dataset
        return ops.epoch_stage_args(x=ds.x, targets=ds.y, batch_size=self.batch_size, num_batches=self.num_batches,
                                    batch_index=w[0:1], epoch=w[1:2], ticket=w[2:3], x_out=x_out, targets_out=targets_out,
                                    order=self._order if shuffled else None, **kw)

    def example(self):
        """A zero minibatch of the loader's shapes and dtypes (what a graphed step is built on)."""
        ds, B = self.dataset, self.batch_size
        return (torch.zeros((B,) + ds.item_shape, dtype=torch.float32, device=ds.device),
                torch.zeros((B,) + ds.target_shape, dtype=ds.y.dtype, device=ds.device))

    def __iter__(self):
        order = self.begin_epoch()
        for _ in range(self.num_batches):
            x, y = self.example()
            ops.epoch_stage(self.stage_args(x, y, order is not None))
            yield x, y
        self.end_epoch()


class EvalLoader:
    """An evaluation pass over a DeviceDataset in identity order, for epoch.score: no step object is built on its
    minibatches, so with drop_last=False a short last minibatch is allowed (it is padded to batch_size and the padding
    rows are excluded from the scores)."""
    shuffle = False

    def __init__(self, dataset: DeviceDataset, batch_size: int, drop_last: bool = False):
        self.dataset, self.batch_size, self.drop_last = dataset, int(batch_size), bool(drop_last)
        N = len(dataset)
        if not 1 <= self.batch_size <= N:
            raise BnnHipError(f"EvalLoader: batch_size must lie in [1, {N}]")
        self.num_batches = N // self.batch_size if self.drop_last else (N + self.batch_size - 1) // self.batch_size

    def __len__(self):
        return self.num_batches


def fill_rows(dataset: DeviceDataset, dst: torch.Tensor, a: int, b: int):
    """Rows a .. b-1 of the data set as fp32 into dst [rows >= b - a, d] (uint8 as u / 255, IEEE division: the staging
    kernel's conversion), zero rows behind them."""
    x = dataset.x
    dst[:b - a].copy_(x[a:b])
    if x.dtype == torch.uint8:
        d255 = getattr(dataset, "_d255", None)
        if d255 is None:
            d255 = dataset._d255 = torch.full((1,), 255.0, dtype=torch.float32, device=dataset.device)
        dst[:b - a].div_(d255)                  # a device divisor: torch divides (a host scalar would multiply by 1 / 255)
    if dst.shape[0] > b - a:
        dst[b - a:].zero_()


class EpochRunner:
    """One epoch of the reference's train_step on a train.GraphedTrainStep, a dense_train.GraphedDenseTrainStep or an
    ensemble.EnsembleTrainStep built on a shared minibatch:
    run_epoch() = one bnn_epoch_permutation, then M x (bnn_epoch_stage into the step's own x, x16, y and beta, the step's
    replay()).  The step keeps its bookkeeping (learning-rate words, MC-sample counter and its host mirror, data-parallel
    all-reduces) exactly as step() does, so evaluations between epochs draw past the indices used.  An ensemble's losses
    (one per member: more than bnn_epoch_stage's loss words) are filed by one device copy after each replay instead."""

    def __init__(self, step, loader: DeviceLoader):
        from .dense_train import GraphedDenseTrainStep
        from .ensemble import EnsembleTrainStep
        self.step, self.loader = step, loader
        self.ensemble = isinstance(step, EnsembleTrainStep)
        if self.ensemble and step.per_member:
            raise BnnHipError("EpochRunner: an EnsembleTrainStep must be built on a shared minibatch ([batch, ...])")
        self.dense = isinstance(step, GraphedDenseTrainStep) or self.ensemble
        ds, B = loader.dataset, loader.batch_size
        d = ds.x.shape[1]
        if not step.x.is_contiguous() or step.x.numel() != B * d or step.x.dtype != torch.float32:
            raise BnnHipError(f"EpochRunner: the step was built on another minibatch shape than [{B}, {d}]")
        if step.y.dtype != ds.y.dtype or not step.y.is_contiguous() or step.y.numel() != B * (ds.y.shape[1] if ds.y.dim() == 2 else 1):
            raise BnnHipError("EpochRunner: the step's targets do not match the data set's")
        if self.ensemble:
            self._out = ()                                              # step.loss [members], copied row by row
            self._beta = None
        elif self.dense:
            self._out = (step.loss,)
            self._beta = None
        else:
            self._out = tuple(step.out)
            self._beta = torch.from_numpy(beta_table(len(loader))).to(ds.device)
        self._loss_src = [o.reshape(1) for o in self._out]              # views of the step's static outputs
        self.loss_cols = step.members if self.ensemble else len(self._out)
        self._args = {}

    def _stage_args(self, shuffled: bool, history: torch.Tensor) -> L.EpochStageArgs:
        a = self._args.get(shuffled)
        if a is None:
            kw = dict(x_bf16_out=getattr(self.step, "x16", None))
            if not self.ensemble:
                kw.update(loss_src=self._loss_src, loss_history=history)
            if self._beta is not None:
                kw.update(beta_table=self._beta, beta=self.step.beta.reshape(1))
            a = self._args[shuffled] = self.loader.stage_args(self.step.x, self.step.y, shuffled, **kw)
        if not self.ensemble:
            a.loss_history = history.data_ptr()                         # a fresh [M, k] per epoch, the block re-used
        return a

    def run_epoch(self, order=None) -> torch.Tensor:
        """Returns the per-minibatch loss tuples as one device tensor [M, k] (k = 4 BBB, 3 local reparameterisation, 1
        MLP, the members of an ensemble): row M-1 is the reference's loss_info, its first entry the epoch_loss.  No host
        synchronisation."""
        ld, M = self.loader, len(self.loader)
        perm = ld.begin_epoch(order)
        hist = torch.empty((M, self.loss_cols), dtype=torch.float32, device=ld.dataset.device)
        a = self._stage_args(perm is not None, hist)
        step = self.step
        for j in range(M):
            ops.epoch_stage(a)                   # files minibatch j-1's loss words, stages minibatch j
            step.replay()
            if self.ensemble:
                hist[j].copy_(step.loss)
        if not self.ensemble:
            hist[M - 1].copy_(torch.cat(self._loss_src))
        ld.end_epoch()
        return hist


def evaluate(net, loader: DeviceLoader, samples: int, chunk: int = 16) -> int:
    """The reference's evaluate (class_task.py:89-103): the number of correct predictions over all minibatches of
    `loader`, counted on the device and read once.  Bayesian networks: the stacked predictive of up to `chunk` minibatches
    per launch group (minibatch g of a call draws the sample indices the per-minibatch loop would); MLP_Dropout:
    predict_mc per minibatch; MLP (and MLP_Dropout with samples = 0, the reference's MLP_Classification with dropout):
    the plain forward's argmax."""
    import networks
    correct = torch.zeros((), dtype=torch.int64, device=loader.dataset.device)
    bayes = isinstance(net, networks.BayesianNetwork)
    xs, ys = [], []

    def flush():
        if xs:
            preds = net.predictive(torch.stack(xs), int(samples), stacked=True).preds
            correct.add_((preds == torch.stack(ys)).sum())
            xs.clear()
            ys.clear()
    with torch.no_grad():
        for x, y in loader:
            if bayes:
                xs.append(x)
                ys.append(y)
                if len(xs) == chunk:
                    flush()
            elif isinstance(net, networks.MLP_Dropout) and samples:
                correct.add_((net.predict_mc(x, int(samples))[0] == y).sum())
            else:
                correct.add_((torch.argmax(net(x), dim=1) == y).sum())
        flush()
    return int(correct.item())


def score(net, loader, samples: int, *, sigma: float = 1.0, bins: int = 10, chunk: int = 16):
    """F12 over a whole data set: the held-out scores (an ops.Scores; `.read()` is the one copy) of every row the loader
    covers -- a DeviceLoader or an EvalLoader, walked in identity order (the scores do not depend on the order).  With
    drop_last=False a short last minibatch is padded with zero rows that bnn_mc_score's n_valid excludes; with
    drop_last=True the rows behind the last full minibatch are left out, as `evaluate` leaves them out.
    Bayesian networks run the stacked evaluation ActivePool.score runs: `chunk` minibatches per launch group, minibatch g
    drawing the MC-sample indices the g-th call of a per-minibatch loop would.  MLP_Dropout: mc_forward per minibatch; MLP:
    the plain forward as one sample.  No host synchronisation before read()."""
    import networks
    from . import mcdropout
    ds, B, samples = loader.dataset, int(loader.batch_size), int(samples)
    ops.require_device(ds.x)
    N, d = ds.x.shape
    rows = (N // B) * B if loader.drop_last else N
    nb = (rows + B - 1) // B
    scores = ops.Scores(net.mode, bins, ds.device)
    cls = net.mode == "classification"
    k = 1 if cls else ds.y.shape[1]
    with torch.no_grad():
        if isinstance(net, networks.BayesianNetwork):
            if samples < 1:
                raise BnnHipError("score: samples must be >= 1")
            from .engine import GraphedScore
            cache = loader.__dict__.setdefault("_score_evals", {})
            for g0 in range(0, nb, int(chunk)):
                G = min(int(chunk), nb - g0)
                a, b = g0 * B, min(rows, (g0 + G) * B)
                key = (id(net), G, B, samples, state.math, state.form)
                ev = cache.get(key)
                if ev is None:
                    x0 = torch.zeros((G, B, d), dtype=torch.float32, device=ds.device)
                    y0 = torch.zeros((G, B) if cls else (G, B, k), dtype=ds.y.dtype, device=ds.device)
                    ev = cache[key] = GraphedScore(net, x0, y0, samples, sigma=sigma, capture=False, stacked=True, scores=scores)
                ev.scores, ev.score_sigma, ev.n_valid = scores, float(sigma), b - a
                fill_rows(ds, ev.x.view(G * B, d), a, b)
                yv = ev.y.view(G * B) if cls else ev.y.view(G * B, k)
                yv[:b - a].copy_(ds.y[a:b])
                if G * B > b - a:
                    yv[b - a:].zero_()                  # padding: a valid label for the chain's own NLL; never scored
                ev.counter.fill_(word32(state.counter))     # where a per-minibatch loop started now would draw
                ev.replay()
        else:
            dropout = isinstance(net, networks.MLP_Dropout) and samples > 0
            xb = torch.empty((B, d), dtype=torch.float32, device=ds.device)
            yb = torch.zeros((B,) if cls else (B, k), dtype=ds.y.dtype, device=ds.device)
            xin = xb.view(B, 1, 1, d) if cls else xb
            for g in range(nb):
                a, b = g * B, min(rows, (g + 1) * B)
                fill_rows(ds, xb, a, b)
                yb[:b - a].copy_(ds.y[a:b])
                if dropout:
                    mcdropout.score(net, xin, yb, samples, sigma=sigma, record=scores, n_valid=b - a)
                else:
                    mcdropout.score_plain(net, xin, yb, sigma=sigma, record=scores, n_valid=b - a)
    return scores
