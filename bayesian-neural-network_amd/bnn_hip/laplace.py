"""F17: a diagonal Laplace posterior for MLP / MLP_Dropout (csrc/laplace.hip) -- the post-hoc route to a posterior for a
network that was trained as a point estimate.  The Gaussian N(w, (diag(F) + tau)^-1) is centred on the trained weights; F is
the diagonal of the generalised Gauss-Newton matrix (or of the empirical Fisher) of the data term summed over the data set,
tau one prior precision chosen by the Laplace estimate of the marginal likelihood.  Being mean-field it IS a BayesianNetwork
(mu = w, rho = softplus^-1 of the standard deviations): network() returns one, and every tool written for the Bayes-by-backprop
networks (predict_mc, predictive, score, PruneSweep, compress, BatchBALD, the bandits) runs on it unchanged.

One minibatch is a fixed chain of launches: bnn_dense_fwd per layer (one sample, fp32 activations, no dropout) ->
bnn_laplace_seed (the output deltas of the C virtual rows of every data row, and the log-likelihood record) ->
bnn_laplace_layer per layer, top down (the layer's curvature diagonal, accumulated in place, and the deltas of the layer
below).  Three layers: 3 + 1 + 3 = 7 launches, no parallel branches; accumulate_graph captures them once.

F18: the predictive that belongs to this curvature is the linearised (GLM) one -- the GGN is the exact Hessian of the network
linearised at the trained weights (Immer et al. 2021), and sampling weights through the non-linear network (network().predict_mc)
underfits against it.  glm_moments / glm_predictive / glm_predictive_graph / glm_score: 3 bnn_dense_fwd + 1 seed +
3 bnn_laplace_glm_layer + 1 bnn_laplace_glm_finish (+ 1 bnn_laplace_glm_sample + 1 bnn_mc_predictive) launches."""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops
from .capture import warm_up, word32
from .mcdropout import _math, flat_input, layers_of
from .engine import _first_minibatch
from .ops import BnnHipError, Predictive
from .runtime import state, take_samples

DEFAULT_PRECISIONS = np.logspace(-4, 4, 33)


class _Chain:
    """The static buffers of one minibatch shape and the launches over them."""

    def __init__(self, la: "LaplaceBase", B: int):
        self.la, self.B = la, B
        dev, layers = la.device, la.layers
        C_out = layers[-1].linear.out_features
        self.R = ops.laplace_rows(B, C_out, la.curvature)
        self.x = torch.zeros((B, layers[0].linear.in_features), dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.int64, device=dev) if la.mode == "classification" else \
            torch.zeros((B, C_out), dtype=torch.float32, device=dev)
        self.acts = [torch.empty((1, B, d.linear.out_features), dtype=torch.float32, device=dev) for d in layers]
        self.gy = torch.empty((self.R, C_out), dtype=torch.float32, device=dev)
        self.g_hidden = [torch.empty((self.R, d.linear.out_features), dtype=torch.float32, device=dev) for d in layers[:-1]]
        self.graph = None

    def stage(self, x: torch.Tensor, y: torch.Tensor):
        la = self.la
        xf = flat_input(la.mlp, x)
        ops.require_device(y)
        if xf.numel() != self.x.numel() or y.numel() != self.y.numel() or y.dtype != self.y.dtype:
            raise BnnHipError(f"{_who(la)}: a minibatch of {self.B} rows needs x of {self.x.numel()} float32 elements and "
                              f"y of {self.y.numel()} {self.y.dtype} elements")
        if xf.is_contiguous() and y.is_contiguous():
            ops.stage_inputs(xf, self.x, y, self.y)                           # one launch instead of two
        else:
            self.x.copy_(xf.reshape(self.x.shape), non_blocking=True)
            self.y.copy_(y.reshape(self.y.shape), non_blocking=True)

    def enqueue(self):
        la = self.la
        layers, math_mode = la.layers, _math()[0]
        last = len(layers) - 1
        with torch.no_grad():
            h = self.x
            for i, d in enumerate(layers):
                lin = d.linear
                ops.dense_fwd(h, lin.weight.detach(), lin.bias.detach(), n_samples=1, math_mode=math_mode, relu=d.relu,
                              drop_p=0.0, layer_id=d.layer_id, seed=state.seed, y_dtype=torch.float32, out=self.acts[i])
                h = self.acts[i][0]
            ops.laplace_seed(self.acts[-1][0], self.y, la.mode, curvature=la.curvature, sigma=la.sigma, gy=self.gy,
                             record=la.record)
            for i in range(last, -1, -1):
                d = layers[i]
                below = layers[i - 1] if i > 0 else None
                la._curvature_launch(i, self.x if i == 0 else self.acts[i - 1][0], self.gy if i == last else self.g_hidden[i],
                                     g_x=self.g_hidden[i - 1] if i > 0 else None,
                                     y=self.acts[i][0] if d.relu else None, gx_mask=below is not None and below.relu,
                                     math_mode=math_mode)

    def capture(self):
        """One warm-up run on a side stream (allocator pools), its accumulation undone, then the capture."""
        la = self.la
        saved = [t.clone() for t in la._accumulated()]
        warm_up(self.enqueue, sync_first=True)
        for t, s in zip(la._accumulated(), saved):
            t.copy_(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.enqueue()
        for t, s in zip(la._accumulated(), saved):                            # (capturing launches nothing; kept for safety)
            t.copy_(s)

    def run(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.enqueue()


class LaplaceStep:
    """What accumulate_graph returns: step(x, y) adds one minibatch of the captured shape by one hipGraph replay."""

    def __init__(self, chain: _Chain):
        self._chain = chain
        self.x, self.y = chain.x, chain.y

    def step(self, x: torch.Tensor, y: torch.Tensor):
        self._chain.stage(x, y)
        self.replay()

    def replay(self):
        """The accumulation of whatever the static buffers (x, y) hold."""
        self._chain.la._check_math()
        self._chain.run()
        self._chain.la._invalidate()


GLM_LINKS = ("probit", "mc")


class _GlmChain:
    """F18: the static buffers of the linearised predictive for one batch size and the launches over them -- bnn_dense_fwd
    per layer, bnn_laplace_seed (regression mode, GGN, sigma 1, no target: gy[c B + n, k] = delta_kc; its row count goes into
    a scratch record, never into la.record), bnn_laplace_glm_layer per layer top down, bnn_laplace_glm_finish, and for
    link 'mc' bnn_laplace_glm_sample (+ bnn_mc_predictive).  No parallel branches."""

    def __init__(self, la: "LaplaceBase", B: int):
        self.la, self.B = la, B
        dev, layers = la.device, la.layers
        C_out = layers[-1].linear.out_features
        P = ops.glm_pairs(C_out)                                              # (refuses more than 16 outputs)
        self.C, self.R = C_out, B * C_out
        f32 = dict(dtype=torch.float32, device=dev)
        self.x = torch.zeros((B, layers[0].linear.in_features), **f32)
        self.acts = [torch.empty((1, B, d.linear.out_features), **f32) for d in layers]
        self.gy = torch.empty((self.R, C_out), **f32)
        self.g_hidden = [torch.empty((self.R, d.linear.out_features), **f32) for d in layers[:-1]]
        self.parts = [torch.empty((ops.glm_tiles(d.linear.out_features), B, P), **f32) for d in layers]
        la._glm_buffers(self)
        self.scratch = torch.zeros(L.LAPLACE_RECORD_DOUBLES, dtype=torch.float64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)

    def stage(self, x: torch.Tensor):
        xf = flat_input(self.la.mlp, x)
        if xf.numel() != self.x.numel():
            raise BnnHipError(f"{_who(self.la)}: a batch of {self.B} rows needs x of {self.x.numel()} float32 elements")
        self.x.copy_(xf.reshape(self.x.shape), non_blocking=True)

    @property
    def mean(self) -> torch.Tensor:
        return self.acts[-1][0]

    def moments(self, tau, tau_dev, *, quantiles=(), sigma: float = 1.0, out=None, n_samples: int = 0) -> "ops.GlmMoments":
        """Forward, seed, the posterior's variance launches per layer, finish (which advances the counter by n_samples)."""
        la = self.la
        layers, math_mode = la.layers, _math()[0]
        last = len(layers) - 1
        with torch.no_grad():
            h = self.x
            for i, d in enumerate(layers):
                lin = d.linear
                ops.dense_fwd(h, lin.weight.detach(), lin.bias.detach(), n_samples=1, math_mode=math_mode, relu=d.relu,
                              drop_p=0.0, layer_id=d.layer_id, seed=state.seed, y_dtype=torch.float32, out=self.acts[i])
                h = self.acts[i][0]
            ops.laplace_seed(self.mean, None, "regression", curvature="ggn", sigma=1.0, gy=self.gy, record=self.scratch)
            for i in range(last, -1, -1):
                d = layers[i]
                below = layers[i - 1] if i > 0 else None
                la._glm_launch(self, i, self.x if i == 0 else self.acts[i - 1][0], self.gy if i == last else self.g_hidden[i],
                               g_x=self.g_hidden[i - 1] if i > 0 else None,
                               y=self.acts[i][0] if d.relu else None, gx_mask=below is not None and below.relu,
                               precision=tau, precision_device=tau_dev, math_mode=math_mode)
            return ops.laplace_glm_finish(self.parts, self.mean, la.mode, sigma=sigma, quantiles=quantiles, out=out,
                                          sample_counter=self.counter if n_samples else None, n_samples=n_samples)

    def sample(self, m: "ops.GlmMoments", samples: int, out=None) -> torch.Tensor:
        """logits [S, B, C] at the global sample indices counter - S ... counter - 1 (the finish launch advanced the counter)."""
        with torch.no_grad():
            return ops.laplace_glm_sample(self.mean, m.chol, samples, seed=state.seed, sample_counter=self.counter, out=out)


class GlmPredictiveGraph:
    """What glm_predictive_graph returns: the static input `.x` ([B, in], the flattened input) and `replay()`, which returns
    the static Predictive of whatever `.x` holds.  With link 'mc' the sample counter `.counter` lives on the device and the
    finish launch advances it, so replay k of a graph built at counter c draws the global samples c + (k + 1) S ... (the
    capture's warm-up run takes c ... c + S - 1), and the host counter is kept in step."""

    def __init__(self, la: "LaplaceBase", x, samples: int, link: str, quantiles, sigma, prior_precision, capture: bool = True):
        la._check_math()
        la._glm_ready()
        self.la, self.link, self.samples = la, link, int(samples)
        self.q, self.sigma = la._glm_args(self.samples, link, quantiles), la.sigma if sigma is None else float(sigma)
        self.tau, self.tau_dev = la._tau(prior_precision, "glm_predictive_graph")
        B = flat_input(la.mlp, x).shape[0]
        ch = self._chain = _GlmChain(la, B)
        ch.stage(x)
        self.x, self.counter = ch.x, ch.counter
        self.mc = link == "mc" and la.mode == "classification"
        self._m = ops.glm_buffers(la.mode, B, ch.C, la.device, len(self.q))
        self.logits = torch.empty((self.samples, B, ch.C), dtype=torch.float32, device=la.device) if self.mc else None
        self._pred = ops.predictive_buffers(la.mode, 1, B, ch.C, la.device) if self.mc else None
        self.result = _first_minibatch(self._pred) if self.mc else la._closed_form(ch.mean, self._m)
        self.counter.fill_(word32(take_samples(0)))
        self.graph = None
        if capture:
            warm_up(self._enqueue, sync_first=True)                           # (also validates the arguments eagerly)
            if self.mc:
                take_samples(self.samples)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._enqueue()

    def _enqueue(self):
        ch = self._chain
        m = ch.moments(self.tau, self.tau_dev, quantiles=self.q, sigma=self.sigma, out=self._m, n_samples=self.samples if self.mc else 0)
        if self.mc:
            ch.sample(m, self.samples, out=self.logits)
            ops.mc_predictive(self.logits, "classification", out=self._pred)

    @property
    def moments(self) -> "ops.GlmMoments":
        """The static cov / var / chol (and closed-form summaries) of the last replay."""
        return self._m

    def replay(self) -> Predictive:
        self.la._check_math()
        self.la._glm_ready()
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue()
        if self.mc:
            take_samples(self.samples)                                        # keep the host-side counter in step
        return self.result


def _who(obj) -> str:
    """The posterior's class name for a message (a bare stand-in object in a test has its own)."""
    return type(obj).__name__


class LaplaceBase:
    """What every Laplace posterior of an MLP here shares: the refusals, the accumulation chain (forward, seed, one curvature
    launch per layer top down; eager or captured), the record, the prior precision chosen by the evidence and the linearised
    (GLM) predictive's interface.  A structure (DiagLaplace; kfac.KronLaplace) supplies its accumulated tensors
    (_allocate, _accumulated), its layer launches (_curvature_launch, _glm_launch, _glm_buffers) and its evidence (_evidence)."""

    def __init__(self, mlp, curvature: str = "ggn", sigma: float = 1.0):
        """`mlp`: a trained networks.MLP, or MLP_Dropout with its dropout switched off (mlp.eval()), on the device.
        `curvature`: 'ggn' (the exact generalised Gauss-Newton / Fisher of the likelihood: C back-propagations per row) or
        'empirical' (squared gradients of the observed labels' log-likelihood: one).  `sigma`: the scale of the Gaussian
        likelihood (regression)."""
        name = _who(self)
        if curvature not in ops.LAPLACE_CURVATURES:
            raise BnnHipError(f"{name}: curvature must be one of {tuple(ops.LAPLACE_CURVATURES)}, got {curvature!r}")
        if not 0.0 < float(sigma) < float("inf"):
            raise BnnHipError(f"{name}: sigma must be positive and finite, got {sigma!r}")
        if mlp.mode not in ("classification", "regression"):
            raise BnnHipError(f"{name}: unknown mode {mlp.mode!r}")
        for m in mlp.modules():
            if isinstance(m, nn.Dropout) and m.p > 0 and m.training:
                raise BnnHipError(f"{name}: the network's dropout is on; the Laplace approximation is taken at the "
                                  "deterministic trained network -- call mlp.eval() first")
        self.layers = layers_of(mlp)
        if any(d.linear.bias is None for d in self.layers):
            raise BnnHipError(f"{name}: every Linear needs a bias (BayesianLinear has one)")
        if state.shard_samples:
            raise BnnHipError(f"{name}: MC-sample sharding is not supported; switch it off")
        self.mlp, self.mode, self.curvature, self.sigma = mlp, mlp.mode, curvature, float(sigma)
        self.params = [t.detach() for d in self.layers for t in (d.linear.weight, d.linear.bias)]
        if len(self.params) > L.LAPLACE_MAX_TENSORS:
            raise BnnHipError(f"{name}: at most {L.LAPLACE_MAX_TENSORS // 2} layers")
        self.device = self.params[0].device
        self._allocate()
        self.record = torch.zeros(L.LAPLACE_RECORD_DOUBLES, dtype=torch.float64, device=self.device)
        self.math = _math()[0]
        self._eager: Dict[int, _Chain] = {}
        self._graphed: Dict[int, _Chain] = {}
        self._glm: Dict[int, _GlmChain] = {}
        self._best_index = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._best = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._fitted = False

    def _check_math(self):
        if _math()[0] != self.math:
            raise BnnHipError(f"{_who(self)}: the math mode changed since this object was built (a captured chain bakes it in)")

    def _invalidate(self):
        """Called after every accumulation and reset: whatever a structure derives from the accumulated tensors is stale."""

    def _glm_ready(self):
        """Called before the GLM launches, eager or replayed: bring what they read up to date with the accumulated tensors."""

    def _glm_buffers(self, chain: "_GlmChain"):
        """Per-chain buffers of the structure's GLM launches (none by default)."""

    # ---- accumulation
    def reset(self):
        """Zero the curvature and the record (and forget a chosen prior precision)."""
        for t in self._accumulated():
            t.zero_()
        self._fitted = False
        self._invalidate()

    def accumulate(self, x: torch.Tensor, y: torch.Tensor):
        """Add one minibatch: forward, seed, one curvature launch per layer (eager launches)."""
        self._check_math()
        B = flat_input(self.mlp, x).shape[0]
        ch = self._eager.get(B)
        if ch is None:
            ch = self._eager[B] = _Chain(self, B)
        ch.stage(x, y)
        ch.enqueue()
        self._fitted = False
        self._invalidate()

    def accumulate_graph(self, x: torch.Tensor, y: torch.Tensor) -> LaplaceStep:
        """The chain for minibatches shaped like (x, y), captured once as a hipGraph: `s = la.accumulate_graph(x, y)`, then
        `s.step(x, y)` per minibatch -- the same launches as accumulate, so the same bits.  Building it accumulates nothing."""
        self._check_math()
        B = flat_input(self.mlp, x).shape[0]
        ch = self._graphed.get(B)
        if ch is None:
            ch = _Chain(self, B)
            ch.stage(x, y)                                                     # (checks the shapes and dtypes)
            ch.capture()
            self._graphed[B] = ch
        return LaplaceStep(ch)

    def fit(self, loader: Iterable):
        """reset(), then every (x, y) minibatch of `loader` (an epoch.DeviceLoader or any iterable of device tensors)
        through the captured chain of its batch size.  Returns self."""
        self.reset()
        for x, y in loader:
            self.accumulate_graph(x, y).step(x, y)
        return self

    @property
    def n_rows(self) -> int:
        """Data rows accumulated so far (one device read)."""
        return int(self.record[1].item())

    # ---- the prior precision
    def log_evidence(self, precisions: Sequence[float]) -> torch.Tensor:
        """The Laplace log marginal likelihood at every candidate prior precision: float64 device tensor [G]."""
        out, _, _ = self._evidence(precisions, torch.zeros(1, dtype=torch.int32, device=self.device),
                                   torch.zeros(2, dtype=torch.float64, device=self.device))
        return out

    def fit_prior_precision(self, precisions: Sequence[float] = DEFAULT_PRECISIONS) -> torch.Tensor:
        """Choose the candidate of the largest evidence (the lowest index on ties).  The choice stays on the device
        (network() takes it from there); `.prior_precision` reads it.  Returns the log evidences [G] (device)."""
        out, _, _ = self._evidence(precisions, self._best_index, self._best)
        self._fitted = True
        return out

    @property
    def prior_precision(self) -> float:
        """The precision fit_prior_precision chose (one device read)."""
        if not self._fitted:
            raise BnnHipError(f"{_who(self)}: no prior precision chosen yet; call fit_prior_precision()")
        return float(self._best[1].item())

    # ---- F18: the linearised (GLM) predictive
    def _tau(self, prior_precision, what: str):
        """(host tau, device word or None): by default the word fit_prior_precision chose (run with its defaults if it has
        not been), as network() does."""
        if prior_precision is None:
            if not self._fitted:
                self.fit_prior_precision()
            return None, self._best[1:2]
        tau = float(prior_precision)
        if not 0.0 < tau < float("inf"):
            raise BnnHipError(f"{_who(self)}.{what}: the prior precision must be positive and finite, got {prior_precision!r}")
        return tau, None

    def _glm_args(self, samples: int, link: str, quantiles) -> tuple:
        """The checked quantile levels; every refusal of the GLM interface that needs no device."""
        if link not in GLM_LINKS:
            raise BnnHipError(f"{_who(self)}: link must be one of {GLM_LINKS}, got {link!r}")
        if link == "mc" and int(samples) < 1:
            raise BnnHipError(f"{_who(self)}: link 'mc' needs samples >= 1, got {samples}")
        C_out = self.layers[-1].linear.out_features
        if C_out > L.LAPLACE_GLM_MAX_CLASSES:
            raise BnnHipError(f"{_who(self)}: the linearised predictive handles at most {L.LAPLACE_GLM_MAX_CLASSES} outputs "
                              f"(BNN_LAPLACE_GLM_MAX_CLASSES); this network has {C_out}")
        if self.mode == "classification" and quantiles:
            raise BnnHipError(f"{_who(self)}: quantiles are a regression summary")
        return ops.quantile_levels(quantiles)

    def _glm_chain(self, x) -> _GlmChain:
        self._check_math()
        self._glm_ready()
        B = flat_input(self.mlp, x).shape[0]
        ch = self._glm.get(B)
        if ch is None:
            ch = self._glm[B] = _GlmChain(self, B)
        ch.stage(x)
        return ch

    def _closed_form(self, mean, m) -> Predictive:
        if self.mode == "classification":
            return Predictive(probs=m.probs, preds=m.preds, predictive_entropy=m.entropy)
        return Predictive(mean=mean, variance=m.var, predictive_variance=m.predictive_variance, quantiles=m.quantiles)

    def glm_moments(self, x: torch.Tensor, prior_precision: Optional[float] = None):
        """(mean [B, C], cov [B, C, C]) of the Gaussian over the outputs of the network linearised at the trained weights,
        f(x, w) + J(x)(theta - w) with theta ~ N(w, (diag(F) + tau)^-1): mean = the network's output, cov = J diag(s^2) J^T
        (KronLaplace: theta ~ N(w, (H + tau)^-1) with its Kronecker-factored H, cov = J (H + tau)^-1 J^T).
        Defined for any such curvature, so an empirical-Fisher object is accepted too (the GGN is the one the linearisation
        is the exact Hessian of)."""
        self._glm_args(0, "probit", None)
        tau, tau_dev = self._tau(prior_precision, "glm_moments")
        ch = self._glm_chain(x)
        m = ch.moments(tau, tau_dev, sigma=self.sigma)
        return ch.mean.clone(), m.cov

    def glm_predictive(self, x: torch.Tensor, samples: int = 0, *, link: str = "probit", quantiles=None, sigma: Optional[float] = None,
                       prior_precision: Optional[float] = None, sample_offset: Optional[int] = None) -> Predictive:
        """The linearised predictive as an ops.Predictive.  Classification, link 'probit': probs = softmax(mean / sqrt(1 +
        pi / 8 var)) (MacKay), preds and predictive_entropy; expected_entropy and mutual_information are None (no closed
        form).  Classification, link 'mc': `samples` logit draws mean + chol . eps through bnn_mc_predictive, all five fields.
        Regression, either link: mean, variance, predictive_variance = variance + sigma^2 and closed-form quantiles; nothing is
        sampled.  `sigma` defaults to the object's, tau to the word fit_prior_precision chose.  `sample_offset`: the first
        global sample index of an 'mc' call (by default the next `samples` of the process-wide counter).  An empirical-Fisher
        object is accepted (see glm_moments)."""
        q = self._glm_args(samples, link, quantiles)
        sg = self.sigma if sigma is None else float(sigma)
        tau, tau_dev = self._tau(prior_precision, "glm_predictive")
        ch = self._glm_chain(x)
        mc = link == "mc" and self.mode == "classification"
        if mc:
            ch.counter.fill_(word32(take_samples(samples) if sample_offset is None else sample_offset))
        m = ch.moments(tau, tau_dev, quantiles=q, sigma=sg, n_samples=int(samples) if mc else 0)
        if not mc:
            return self._closed_form(ch.mean.clone(), m)
        return _first_minibatch(ops.mc_predictive(ch.sample(m, int(samples)), "classification"))

    def glm_predictive_graph(self, x: torch.Tensor, samples: int = 0, *, link: str = "probit", quantiles=None,
                             sigma: Optional[float] = None, prior_precision: Optional[float] = None,
                             capture: bool = True) -> GlmPredictiveGraph:
        """glm_predictive for inputs shaped like x, captured once as a hipGraph: `g = la.glm_predictive_graph(x, ...)`, write
        `g.x`, `g.replay()` -- the same launches as the eager call, so the same bits at the same counter value.  With link
        'mc' every replay draws fresh samples through the device counter `g.counter`."""
        return GlmPredictiveGraph(self, x, samples, link, quantiles, sigma, prior_precision, capture=capture)

    def glm_sample(self, x: torch.Tensor, samples: int, *, prior_precision: Optional[float] = None,
                   sample_offset: Optional[int] = None) -> torch.Tensor:
        """[samples, B, C] draws of the linearised network's outputs, mean + chol . eps (what link 'mc' and glm_score consume)."""
        self._glm_args(samples, "mc", None)
        tau, tau_dev = self._tau(prior_precision, "glm_sample")
        ch = self._glm_chain(x)
        ch.counter.fill_(word32(take_samples(samples) if sample_offset is None else sample_offset))
        m = ch.moments(tau, tau_dev, sigma=self.sigma, n_samples=int(samples))
        return ch.sample(m, int(samples))

    def glm_score(self, x: torch.Tensor, y: torch.Tensor, samples: int, *, sigma: Optional[float] = None, bins: int = 10,
                  record=None, prior_precision: Optional[float] = None, sample_offset: Optional[int] = None) -> "ops.Scores":
        """F12's held-out scores (bnn_mc_score, unchanged) of `samples` draws of the linearised network's outputs, in both
        modes."""
        logits = self.glm_sample(x, samples, prior_precision=prior_precision, sample_offset=sample_offset)
        return ops.mc_score(logits, y, self.mode, sigma=self.sigma if sigma is None else float(sigma), bins=int(bins), record=record)


class DiagLaplace(LaplaceBase):
    """The diagonal structure: curv[2 l], curv[2 l + 1] the curvature diagonals of layer l's weight and bias."""

    def _allocate(self):
        self.curv = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]

    def _accumulated(self):
        return self.curv + [self.record]

    def _curvature_launch(self, i, x, gy, *, g_x, y, gx_mask, math_mode):
        ops.laplace_layer(x, gy, self.layers[i].linear.weight.detach(), f_w=self.curv[2 * i], f_b=self.curv[2 * i + 1], g_x=g_x,
                          y=y, gx_mask=gx_mask, math_mode=math_mode)

    def _evidence(self, precisions, best_index, best):
        taus = [float(t) for t in np.asarray(precisions, dtype=np.float64).reshape(-1)]
        return ops.laplace_evidence(self.params, self.curv, taus, record=self.record, best_index=best_index, best=best)

    def _glm_launch(self, chain, i, x, gy, *, g_x, y, gx_mask, precision, precision_device, math_mode):
        ops.laplace_glm_layer(x, gy, self.layers[i].linear.weight.detach(), f_w=self.curv[2 * i], f_b=self.curv[2 * i + 1],
                              cov_part=chain.parts[i], g_x=g_x, y=y, gx_mask=gx_mask, precision=precision,
                              precision_device=precision_device, math_mode=math_mode)

    # ---- the posterior as a network
    def network(self, prior_precision: Optional[float] = None):
        """A networks.BayesianNetwork on the device holding this posterior: mu = the MLP's weights (the bits), rho =
        softplus^-1((F + tau)^-1/2), Gaussian prior N(0, tau^-1/2), weight sampling (local_reparam=False).
        `prior_precision`: tau; by default the one fit_prior_precision chose (run with its defaults if it has not been)."""
        import networks
        if [(d.relu, d.linear.in_features, d.linear.out_features) for d in self.layers] != \
                [(True, self.mlp.input_shape, self.mlp.hidden_units), (True, self.mlp.hidden_units, self.mlp.hidden_units),
                 (False, self.mlp.hidden_units, self.mlp.classes)]:
            raise BnnHipError("DiagLaplace.network: BayesianNetwork has three layers in -> hidden -> hidden -> classes with "
                              "ReLUs between them; this network has another architecture")
        if prior_precision is None:
            if not self._fitted:
                self.fit_prior_precision()
            tau, tau_dev = self.prior_precision, self._best[1:2]
        else:
            tau, tau_dev = float(prior_precision), None
            if not 0.0 < tau < float("inf"):
                raise BnnHipError(f"DiagLaplace.network: the prior precision must be positive and finite, got {prior_precision!r}")
        mp = dict(input_shape=self.mlp.input_shape, classes=self.mlp.classes, batch_size=self.mlp.batch_size,
                  hidden_units=self.mlp.hidden_units, mode=self.mode, mu_init=[-0.2, 0.2], rho_init=[-5.0, -4.0],
                  prior_init=[tau ** -0.5], mixture_prior=False, local_reparam=False)
        with torch.device(self.device):
            net = networks.BayesianNetwork(mp)
        net.to(self.device)
        lays = (net.l1, net.l2, net.l3)
        mus = [t.data for l in lays for t in (l.weight_mu, l.bias_mu)]
        rhos = [t.data for l in lays for t in (l.weight_rho, l.bias_rho)]
        with torch.no_grad():
            ops.laplace_posterior(self.params, self.curv, mus, rhos, precision=None if tau_dev is not None else tau,
                                  precision_device=tau_dev)
        return net
