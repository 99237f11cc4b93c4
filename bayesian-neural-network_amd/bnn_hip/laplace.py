"""F17: a diagonal Laplace posterior for MLP / MLP_Dropout (csrc/laplace.hip) -- the post-hoc route to a posterior for a
network that was trained as a point estimate.  The Gaussian N(w, (diag(F) + tau)^-1) is centred on the trained weights; F is
the diagonal of the generalised Gauss-Newton matrix (or of the empirical Fisher) of the data term summed over the data set,
tau one prior precision chosen by the Laplace estimate of the marginal likelihood.  Being mean-field it IS a BayesianNetwork
(mu = w, rho = softplus^-1 of the standard deviations): network() returns one, and every tool written for the Bayes-by-backprop
networks (predict_mc, predictive, score, PruneSweep, compress, BatchBALD, the bandits) runs on it unchanged.

One minibatch is a fixed chain of launches: bnn_dense_fwd per layer (one sample, fp32 activations, no dropout) ->
bnn_laplace_seed (the output deltas of the C virtual rows of every data row, and the log-likelihood record) ->
bnn_laplace_layer per layer, top down (the layer's curvature diagonal, accumulated in place, and the deltas of the layer
below).  Three layers: 3 + 1 + 3 = 7 launches, no parallel branches; accumulate_graph captures them once."""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops
from .mcdropout import _math, flat_input, layers_of
from .ops import BnnHipError
from .runtime import state

DEFAULT_PRECISIONS = np.logspace(-4, 4, 33)


class _Chain:
    """The static buffers of one minibatch shape and the launches over them."""

    def __init__(self, la: "DiagLaplace", B: int):
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
            raise BnnHipError(f"DiagLaplace: a minibatch of {self.B} rows needs x of {self.x.numel()} float32 elements and "
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
                ops.laplace_layer(self.x if i == 0 else self.acts[i - 1][0], self.gy if i == last else self.g_hidden[i],
                                  d.linear.weight.detach(), f_w=la.curv[2 * i], f_b=la.curv[2 * i + 1],
                                  g_x=self.g_hidden[i - 1] if i > 0 else None,
                                  y=self.acts[i][0] if d.relu else None, gx_mask=below is not None and below.relu,
                                  math_mode=math_mode)

    def capture(self):
        """One warm-up run on a side stream (allocator pools), its accumulation undone, then the capture."""
        la = self.la
        saved = [t.clone() for t in la.curv] + [la.record.clone()]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.enqueue()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for t, s in zip(la.curv + [la.record], saved):
            t.copy_(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.enqueue()
        for t, s in zip(la.curv + [la.record], saved):                        # (capturing launches nothing; kept for safety)
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


class DiagLaplace:
    def __init__(self, mlp, curvature: str = "ggn", sigma: float = 1.0):
        """`mlp`: a trained networks.MLP, or MLP_Dropout with its dropout switched off (mlp.eval()), on the device.
        `curvature`: 'ggn' (the exact generalised Gauss-Newton / Fisher of the likelihood: C back-propagations per row) or
        'empirical' (squared gradients of the observed labels' log-likelihood: one).  `sigma`: the scale of the Gaussian
        likelihood (regression)."""
        if curvature not in ops.LAPLACE_CURVATURES:
            raise BnnHipError(f"DiagLaplace: curvature must be one of {tuple(ops.LAPLACE_CURVATURES)}, got {curvature!r}")
        if not 0.0 < float(sigma) < float("inf"):
            raise BnnHipError(f"DiagLaplace: sigma must be positive and finite, got {sigma!r}")
        if mlp.mode not in ("classification", "regression"):
            raise BnnHipError(f"DiagLaplace: unknown mode {mlp.mode!r}")
        for m in mlp.modules():
            if isinstance(m, nn.Dropout) and m.p > 0 and m.training:
                raise BnnHipError("DiagLaplace: the network's dropout is on; the Laplace approximation is taken at the "
                                  "deterministic trained network -- call mlp.eval() first")
        self.layers = layers_of(mlp)
        if any(d.linear.bias is None for d in self.layers):
            raise BnnHipError("DiagLaplace: every Linear needs a bias (BayesianLinear has one)")
        if state.shard_samples:
            raise BnnHipError("DiagLaplace: MC-sample sharding is not supported; switch it off")
        self.mlp, self.mode, self.curvature, self.sigma = mlp, mlp.mode, curvature, float(sigma)
        self.params = [t.detach() for d in self.layers for t in (d.linear.weight, d.linear.bias)]
        if len(self.params) > L.LAPLACE_MAX_TENSORS:
            raise BnnHipError(f"DiagLaplace: at most {L.LAPLACE_MAX_TENSORS // 2} layers")
        self.device = self.params[0].device
        self.curv = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.record = torch.zeros(L.LAPLACE_RECORD_DOUBLES, dtype=torch.float64, device=self.device)
        self.math = _math()[0]
        self._eager: Dict[int, _Chain] = {}
        self._graphed: Dict[int, _Chain] = {}
        self._best_index = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._best = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._fitted = False

    def _check_math(self):
        if _math()[0] != self.math:
            raise BnnHipError("DiagLaplace: the math mode changed since this object was built (a captured chain bakes it in)")

    # ---- accumulation
    def reset(self):
        """Zero the curvature and the record (and forget a chosen prior precision)."""
        for t in self.curv:
            t.zero_()
        self.record.zero_()
        self._fitted = False

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

    def _evidence(self, precisions, best_index, best):
        taus = [float(t) for t in np.asarray(precisions, dtype=np.float64).reshape(-1)]
        return ops.laplace_evidence(self.params, self.curv, taus, record=self.record, best_index=best_index, best=best)

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
            raise BnnHipError("DiagLaplace: no prior precision chosen yet; call fit_prior_precision()")
        return float(self._best[1].item())

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
