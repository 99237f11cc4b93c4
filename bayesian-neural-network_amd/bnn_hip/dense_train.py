"""K6: one training step of MLP / MLP_Dropout (the reference's train_step, classification/class_task.py:150-157,
regression/reg_task.py:176-183: zero_grad -> forward -> cross_entropy / mse_loss (sum) -> backward -> optimiser step)
as a fixed chain of HIP launches, captured once as a hipGraph:

  bnn_dense_fwd per layer (one sample, fp32 outputs, the kind-3 dropout mask of the step's global sample index; the
  output layer's launch advances the device sample counter)  ->  bnn_dense_loss (loss + logits gradient)  ->
  bnn_dense_bwd per layer, top down (weight and bias gradients; the input gradient, already multiplied by the layer
  below's mask read off its saved output, except at layer 0)  ->  bnn_sgd_step / bnn_adam_step.

Three layers: 3 + 1 + 3 + 1 = 8 launches.  The step always trains in train-mode semantics (dropout on), as the
reference's train_step does after net.train().

With ivon.FusedIVON the chain runs once per MC sample s = 0 .. S - 1 behind the optimiser's draw launch (opt.perturb(s):
theta = m + sigma eps into the parameters) and ends in its step launch: 8 S + 1 launches, the sample counter advancing by S.
The loss returned is then the LAST sample's sum loss at the drawn weights, not the loss at the mean."""
from __future__ import annotations

import torch

from . import _lib as L
from . import ops
from .capture import SampleCounter, grad_bucket, snapshot, warm_up
from .mcdropout import _math, flat_input, layers_of
from .ops import BnnHipError
from .optim import FusedAdam, FusedSGD, _sgd_supported
from .runtime import state
from .ivon import FusedIVON, default_loss_scale, require_plain_mlp
from .sgmcmc import FusedSGMCMC
from .swag import FusedSWAG

LOSSES = ("cross_entropy", "mse")


class GraphedDenseTrainStep:
    def __init__(self, mlp, optimizer, x: torch.Tensor, y: torch.Tensor, loss=None, capture: bool = True):
        """`x`, `y`: an example minibatch (the shape and dtype of every later one): classification x [B, 1, h, w] with
        int64 labels [B], regression x [B, in] with float32 targets of B * out elements.  `optimizer`: FusedSGD,
        FusedAdam, sgmcmc.FusedSGMCMC (the sampler in the optimiser's place), swag.FusedSWAG (SGD that also collects SWAG's
        moments) or ivon.FusedIVON (variational online Newton: its loss_scale, when None, becomes
        ivon.default_loss_scale(loss, B, optimizer.sigma)) with capturable=True over the network's parameters.
        `loss`: 'cross_entropy' or 'mse' (sum reduction),
        by default the reference's for mlp.mode.  `capture=False`: the same launches, run eagerly on every step.

        Building the step runs one real warm-up step and then restores the parameters, the optimiser state and the
        sample counter, so the model and the optimiser are left as they were."""
        if not isinstance(optimizer, (FusedSGD, FusedAdam, FusedSGMCMC, FusedSWAG, FusedIVON)):
            raise BnnHipError("GraphedDenseTrainStep needs FusedSGD, FusedAdam, FusedSGMCMC, FusedSWAG or FusedIVON "
                              "(capturable=True)")
        if not all(g.get("capturable") for g in optimizer.param_groups):
            raise BnnHipError("GraphedDenseTrainStep needs a capturable optimiser (capturable=True)")
        if isinstance(optimizer, FusedSGD):
            for g in optimizer.param_groups:
                _sgd_supported(g)
        if isinstance(optimizer, FusedIVON):
            require_plain_mlp(mlp, "GraphedDenseTrainStep")
        if state.shard_samples:
            raise BnnHipError("GraphedDenseTrainStep: MC-sample sharding is not supported; switch it off")
        if loss is None:
            loss = "cross_entropy" if mlp.mode == "classification" else "mse"
        if loss not in LOSSES:
            raise BnnHipError(f"GraphedDenseTrainStep: loss must be one of {LOSSES}, got {loss!r}")
        self.layers = layers_of(mlp)
        for d in self.layers[:-1]:
            if d.p and not d.relu:
                raise BnnHipError("GraphedDenseTrainStep: a Dropout needs a ReLU before it (the backward reads the mask "
                                  "off the layer's saved output)")
        self.loss_mode = "classification" if loss == "cross_entropy" else "regression"
        self.mlp, self.opt = mlp, optimizer
        self.x = flat_input(mlp, x).clone().contiguous()
        ops.require_device(y)
        B, dev = self.x.shape[0], self.x.device
        C_out = self.layers[-1].linear.out_features
        if self.loss_mode == "classification":
            if y.dtype != torch.int64 or y.numel() != B:
                raise BnnHipError("GraphedDenseTrainStep: cross-entropy targets must be int64 labels, one per row")
        elif y.dtype != torch.float32 or y.numel() != B * C_out:
            raise BnnHipError(f"GraphedDenseTrainStep: mse targets must be float32 with {B * C_out} elements")
        self.y = y.clone().contiguous()
        self.math = _math()[0]
        # MC samples per step: the draws of a FusedIVON; every other optimiser steps on one forward / backward pass
        self.ivon = isinstance(optimizer, FusedIVON)
        self.samples = optimizer.param_groups[0]["samples"] if self.ivon else 1
        if self.ivon:
            if optimizer._drawn:
                raise BnnHipError("GraphedDenseTrainStep: the FusedIVON has a step under way; call its step() first")
            self.loss_scale = optimizer.loss_scale if optimizer.loss_scale is not None else \
                default_loss_scale(loss, B, optimizer.sigma)

        # the parameters, in layer order, and one flat gradient bucket (each slice 256-byte aligned); p.grad are views
        self.params = [t for d in self.layers for t in (d.linear.weight, d.linear.bias) if t is not None]
        in_opt = {id(p) for g in optimizer.param_groups for p in g["params"]}
        if any(id(p) not in in_opt for p in self.params):
            raise BnnHipError("GraphedDenseTrainStep: the optimiser must hold every parameter of the network")
        self.bucket, offs = grad_bucket(self.params, dev)
        self.grad_views = [self.bucket[o:o + p.numel()].view(p.shape) for o, p in zip(offs, self.params)]
        self._grad_of = dict(zip(map(id, self.params), self.grad_views))

        # activations (fp32 for every layer: the backward reads them), the logits' gradient, the input gradients
        self.acts = [torch.empty((1, B, d.linear.out_features), dtype=torch.float32, device=dev) for d in self.layers]
        self.g_logits = torch.empty((B, C_out), dtype=torch.float32, device=dev)
        self.g_hidden = [torch.empty((B, d.linear.out_features), dtype=torch.float32, device=dev) for d in self.layers[:-1]]
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.scales = [ops.dropout_params(d.p)[1] for d in self.layers]

        # the optimiser's shared device sample counter (capture.SampleCounter): a step draws global sample index
        # base + counter, the output layer's forward advances it, and the host's counter is kept in step, so later
        # evaluations draw past it
        sh = self._shared = SampleCounter.of(optimizer, dev)
        self.counter, self.base = sh["counter"], sh["base"]
        sh.sync()

        self.graph = None
        if capture:
            # one real step on a side stream (allocator pools, the optimiser's lazily created state and device words), then
            # its effects undone: parameters, optimiser state, device step / learning-rate words, sample counter
            restore, mirror = snapshot(optimizer), sh["mirror"]
            warm_up(self._enqueue, sync_first=True)
            restore()
            sh.set(mirror)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._enqueue()

    # ---- the chain
    def _enqueue(self):
        if self.ivon:
            self._attach_grads()                 # perturb(s >= 1) folds the previous sample's gradients
            for s in range(self.samples):
                self.opt.perturb(s)
                self._enqueue_pass()
            self.opt.step(loss_scale=self.loss_scale)
            return
        self._enqueue_pass()
        self._attach_grads()
        if isinstance(self.opt, FusedAdam):
            self.opt._bump = None                # the sample counter advances in the forward, not in Adam's launch
        self.opt.step()

    def _enqueue_pass(self):
        """One forward / loss / backward pass at the parameters' current values (a launch per layer each way and the loss
        launch); the gradients are left in the bucket."""
        with torch.no_grad():
            last = len(self.layers) - 1
            h = self.x
            for i, d in enumerate(self.layers):
                lin = d.linear
                ops.dense_fwd(h, lin.weight.detach(), None if lin.bias is None else lin.bias.detach(), n_samples=1,
                              math_mode=self.math, relu=d.relu, drop_p=d.p, layer_id=d.layer_id, seed=state.seed,
                              sample_offset=self.base, sample_counter=self.counter, sample_counter_inc=1 if i == last else 0,
                              y_dtype=torch.float32, out=self.acts[i])
                h = self.acts[i][0]
            ops.dense_loss(self.acts[-1][0], self.y, self.loss_mode, loss=self.loss, g_logits=self.g_logits)
            for i in range(last, -1, -1):
                d = self.layers[i]
                lin = d.linear
                below = self.layers[i - 1] if i > 0 else None
                ops.dense_bwd(self.x if i == 0 else self.acts[i - 1][0], self.g_logits if i == last else self.g_hidden[i],
                              lin.weight.detach(), g_w=self._grad_of[id(lin.weight)],
                              g_b=None if lin.bias is None else self._grad_of[id(lin.bias)],
                              g_x=self.g_hidden[i - 1] if i > 0 else None, gx_mask=below is not None and below.relu,
                              gx_scale=self.scales[i - 1] if i > 0 else 1.0, math_mode=self.math)

    def _attach_grads(self):
        for p, g in zip(self.params, self.grad_views):
            p.grad = g

    # ---- the public step
    def step(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """One optimiser step on minibatch (x, y); returns the static 0-dim loss tensor (the reference's loss_info: read
        it before the next call; with a FusedIVON the last sample's sum loss at the drawn weights)."""
        xf = flat_input(self.mlp, x)
        ops.require_device(y)
        if xf.numel() != self.x.numel() or y.numel() != self.y.numel() or y.dtype != self.y.dtype:
            raise BnnHipError("GraphedDenseTrainStep.step: the minibatch must have the example's shape and dtype")
        if xf.is_contiguous() and y.is_contiguous():
            ops.stage_inputs(xf, self.x, y, self.y)                       # one launch instead of two
        else:
            self.x.copy_(xf.reshape(self.x.shape), non_blocking=True)
            self.y.copy_(y.reshape(self.y.shape), non_blocking=True)
        return self.replay()

    def replay(self) -> torch.Tensor:
        """The step on whatever the static buffers (x, y) hold -- step() after its staging; a caller that stages them on
        the device itself (epoch.EpochRunner) calls this.  Same bookkeeping, same return value."""
        self.opt.sync_lr()
        self._shared.sync()
        if self.graph is not None:
            self._attach_grads()
            self.graph.replay()
        else:
            self._enqueue()
        self._shared.advance(self.samples)
        return self.loss
