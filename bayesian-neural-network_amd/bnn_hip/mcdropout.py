"""MC dropout of MLP_Dropout on the device (K5, csrc/mlp_dropout.hip): the reference keeps the network in train mode at
test time and runs S full forward passes one after the other (main.py:42, :138; regression/reg_task.py:186-195,
classification/class_task.py:230-236).  Here the S passes are one launch per Linear layer: the first layer's product is
shared by the samples (nothing is random before the first dropout), the later layers run S * batch rows against the
shared weights, and each layer's dropout is the kind-3 Philox mask of include/bnn_hip.h in the epilogue.  The outputs
feed the same summaries as the Bayesian networks' (bnn_mc_predictive)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from . import _lib as L
from . import ops
from .capture import capture_on_side_stream
from .engine import _first_minibatch, dist_info
from .ops import BnnHipError, Predictive
from .runtime import state, take_samples


class DenseLayer:
    """One Linear -> [ReLU] -> [Dropout] group of an nn.Sequential."""

    def __init__(self, linear: nn.Linear, layer_id: int, relu: bool, p: float):
        self.linear, self.layer_id, self.relu, self.p = linear, layer_id, relu, p


def layers_of(mlp) -> List[DenseLayer]:
    """mlp.net as groups Linear -> [ReLU] -> [Dropout] ending in a bare Linear; BnnHipError for anything else, for
    parameters that are not fp32 device tensors and for a dropout probability outside [0, 1)."""
    mods = list(mlp.net)
    out, i = [], 0
    while i < len(mods):
        lin = mods[i]
        if type(lin) is not nn.Linear:
            raise BnnHipError(f"MC dropout: expected nn.Linear at position {i} of the network, got {type(lin).__name__}")
        i += 1
        relu = i < len(mods) and type(mods[i]) is nn.ReLU
        i += relu
        p = 0.0
        if i < len(mods) and type(mods[i]) is nn.Dropout:
            p = float(mods[i].p)
            ops.dropout_params(p)
            i += 1
        out.append(DenseLayer(lin, len(out), relu, p))
    if not out or out[-1].relu or out[-1].p:
        raise BnnHipError("MC dropout: the network must end in a bare nn.Linear")
    for d in out:
        for t in (d.linear.weight, d.linear.bias):
            if t is None:
                continue
            ops.require_device(t)
            if t.dtype != torch.float32:
                raise BnnHipError(f"MC dropout: parameters must be float32, got {t.dtype}")
    return out


def flat_input(mlp, x: torch.Tensor) -> torch.Tensor:
    """The input as the reference's forward takes it (networks.py:271-276): classification [B, 1, 28, 28] -> [B, in]."""
    if mlp.mode == 'classification':
        if x.dim() != 4:
            raise BnnHipError(f"MC dropout: classification input must be [batch, 1, h, w], got {tuple(x.shape)}")
        x = x.reshape(-1, mlp.input_shape)
    elif x.dim() != 2:
        raise BnnHipError(f"MC dropout: regression input must be [batch, in], got {tuple(x.shape)}")
    ops.require_device(x)
    if x.dtype != torch.float32:
        raise BnnHipError(f"MC dropout: input must be float32, got {x.dtype}")
    return x


def _math() -> Tuple[int, torch.dtype]:
    """(math mode of the launches, dtype of the hidden activations): bf16 math carries bf16 activations; f32 and bf16x3
    run the exact fp32 MFMA on fp32 activations."""
    if state.math == L.MATH_BF16:
        return L.MATH_BF16, torch.bfloat16
    return L.MATH_F32, torch.float32


def _no_sharding():
    if dist_info()[1] > 1:
        raise BnnHipError("MC dropout: sample sharding over several ranks is not supported")


def run_chain(layers: List[DenseLayer], x: torch.Tensor, samples: int, *, sample_offset: int, counter=None,
              bufs: Optional[List[torch.Tensor]] = None) -> torch.Tensor:
    """One launch per layer; returns the fp32 outputs [samples, B, out].  With `counter` (a device word) the last layer
    advances it by `samples`, so a captured chain draws fresh masks on every replay."""
    math_mode, hidden = _math()
    h = x
    last = len(layers) - 1
    for i, d in enumerate(layers):
        lin = d.linear
        h = ops.dense_fwd(h, lin.weight.detach(), None if lin.bias is None else lin.bias.detach(), n_samples=samples,
                          math_mode=math_mode, relu=d.relu, drop_p=d.p, layer_id=d.layer_id, seed=state.seed,
                          sample_offset=sample_offset, sample_counter=counter,
                          sample_counter_inc=samples if (i == last and counter is not None) else 0,
                          y_dtype=torch.float32 if i == last else hidden, out=None if bufs is None else bufs[i])
    return h


def mc_forward(mlp, x: torch.Tensor, samples: int) -> torch.Tensor:
    """[samples, B, out] fp32: `samples` MC-dropout passes, the masks at the next `samples` global sample indices."""
    samples = int(samples)
    if samples < 1:
        raise BnnHipError("MC dropout: samples must be >= 1")
    layers = layers_of(mlp)
    xf = flat_input(mlp, x)
    _no_sharding()
    first = take_samples(samples)
    with torch.no_grad():
        return run_chain(layers, xf, samples, sample_offset=first)


def predict_mc(mlp, x: torch.Tensor, samples: int):
    """(preds [B], probs [B, C]): probs = mean_s softmax of the MC-dropout outputs (class_task.py:230-236)."""
    logits = mc_forward(mlp, x, samples)
    probs, preds = ops.mc_softmax_mean(logits, 1.0 / int(samples))
    return preds, probs


def _summary_args(mode: str, quantiles):
    if mode not in ("classification", "regression"):
        raise Exception("Training mode must be either 'regression' or 'classification'")
    if mode == "classification" and quantiles:
        raise BnnHipError("predictive: quantiles are a regression summary")
    return ops.quantile_levels(quantiles)


def predictive(mlp, x: torch.Tensor, samples: int, quantiles=None, sigma: float = 1.0) -> Predictive:
    """bnn_mc_predictive over mc_forward's outputs: the same summaries as BayesianNetwork.predictive."""
    q = _summary_args(mlp.mode, quantiles)
    logits = mc_forward(mlp, x, samples)
    return _first_minibatch(ops.mc_predictive(logits, mlp.mode, sigma=float(sigma), quantiles=q))


def score(mlp, x: torch.Tensor, y: torch.Tensor, samples: int, sigma: float = 1.0, bins: int = 10, record=None,
          n_valid: Optional[int] = None) -> "ops.Scores":
    """F12: bnn_mc_score over mc_forward's outputs against the targets: the same scores as BayesianNetwork.score."""
    if mlp.mode not in ("classification", "regression"):
        raise Exception("Training mode must be either 'regression' or 'classification'")
    return ops.mc_score(mc_forward(mlp, x, samples), y, mlp.mode, sigma=float(sigma), bins=int(bins), record=record,
                        n_valid=n_valid)


def score_plain(mlp, x: torch.Tensor, y: torch.Tensor, sigma: float = 1.0, bins: int = 10, record=None,
                n_valid: Optional[int] = None) -> "ops.Scores":
    """F12 for a deterministic network: its forward as the single sample of bnn_mc_score."""
    if mlp.mode not in ("classification", "regression"):
        raise Exception("Training mode must be either 'regression' or 'classification'")
    ops.require_device(x)
    with torch.no_grad():
        out = mlp(x).float().contiguous()
    return ops.mc_score(out.unsqueeze(0), y, mlp.mode, sigma=float(sigma), bins=int(bins), record=record, n_valid=n_valid)


class GraphedDropoutPredictive:
    """predictive() for one input shape as a replayable evaluation: static input `.x` ([B, in], the flattened input),
    static outputs, one launch per layer plus the summary launch, all on one stream, captured once as a hipGraph
    (`capture=False`: the same chain launched eagerly on every replay).  The sample counter lives on the device and the
    output layer's launch advances it, so every replay draws fresh masks: replay k of an evaluation built at counter c
    uses the global sample indices c + (k + 1) S ... (the capture's warm-up run takes c .. c + S - 1), and the host
    counter is kept in step.  `replay()` returns the static Predictive."""

    def __init__(self, mlp, x: torch.Tensor, samples: int, quantiles=None, sigma: float = 1.0, capture: bool = True):
        self.mlp, self.samples, self.sigma = mlp, int(samples), float(sigma)
        if self.samples < 1:
            raise BnnHipError("MC dropout: samples must be >= 1")
        self.mode = mlp.mode
        self.q = _summary_args(self.mode, quantiles)
        self.layers = layers_of(mlp)
        _no_sharding()
        self.x = flat_input(mlp, x).clone().contiguous()
        dev = self.x.device
        B, S = self.x.shape[0], self.samples
        _, hidden = _math()
        last = len(self.layers) - 1
        self.bufs = [torch.empty((S, B, d.linear.out_features), dtype=torch.float32 if i == last else hidden, device=dev)
                     for i, d in enumerate(self.layers)]
        self.counter = torch.tensor([take_samples(0)], dtype=torch.int32, device=dev)
        self._pred = ops.predictive_buffers(self.mode, 1, B, self.layers[-1].linear.out_features, dev, self.q)
        self.result = _first_minibatch(self._pred)
        self.graph = None
        if capture:
            with torch.no_grad():
                self._enqueue()                  # warm-up (also validates the arguments eagerly)
            take_samples(S)
            torch.cuda.synchronize()
            with torch.no_grad():
                self.graph = capture_on_side_stream(self._enqueue)

    def _enqueue(self):
        logits = run_chain(self.layers, self.x, self.samples, sample_offset=0, counter=self.counter, bufs=self.bufs)
        ops.mc_predictive(logits, self.mode, sigma=self.sigma, quantiles=self.q, out=self._pred)

    def replay(self) -> Predictive:
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._enqueue()
        take_samples(self.samples)               # keep the host-side counter in step
        return self.result

    @property
    def logits(self) -> torch.Tensor:
        return self.bufs[-1]
