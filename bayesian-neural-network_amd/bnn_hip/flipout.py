"""F16: the Flipout estimator (Wen et al., ICLR 2018) for the factorised Gaussian posterior of BayesianLinear, on the kernels of
csrc/flipout.hip (include/bnn_hip.h F16).

One base draw Delta = sigma o eps per layer is shared by the minibatch; every batch row sees it through its own rank-one sign
pattern, so each row has its own, marginally exact, weight sample -- and `samples` MC samples of a minibatch cost
`base_draws` <= samples passes of the epsilon generator plus shared-weight products over the stacked rows.  The scale-mixture
prior and the sampled log q - log p work as for BayesianLinear, evaluated at the base draw.

FlipoutLinear has BayesianLinear's parameters (names, shapes, initialisation), so state dicts interchange;
BayesianNetwork.flipout() returns a FlipoutNetwork over the SAME Parameters, so pruning, compression, posterior statistics and
BatchBALD keep working on the BBB view of a Flipout-trained network.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from . import _lib as L
from . import ops
from .functional import NLLFn, _need_f32
from .ops import BnnHipError, PriorSpec
from .runtime import state, take_samples
from .train import GraphedTrainStep


class _StandardNormal:
    """Default of the `.normal` seam (as in networks.py): while a node holds it, epsilon is generated on chip."""

    def sample(self, size):
        return torch.randn(tuple(size))


class _Node:
    """The (mu, rho) pair of a layer with BayesianLinear's `.normal` seam."""

    def __init__(self, mu, rho):
        self.mu, self.rho = mu, rho
        self.normal = _StandardNormal()

    @property
    def sigma(self):
        return torch.log1p(torch.exp(self.rho))


def _stubbed(node) -> bool:
    return type(node.normal).__name__ != "_StandardNormal"


@dataclass(frozen=True)
class FlipoutCall:
    """Static (non-tensor) description of one Flipout layer launch."""
    n_samples: int
    n_draws: int
    prior: PriorSpec
    math_mode: int
    relu: bool
    eps_mode: int
    seed: int
    layer_id: int
    sample_offset: int
    want_stats: bool
    sample_counter: Optional[torch.Tensor] = None
    row_offset: int = 0


class FlipoutLinearFn(torch.autograd.Function):
    """(x [B, K] | [S, B, K], w_mu, w_rho, b_mu, b_rho, eps_w [D, N, K] | None, eps_b [D, N] | None) ->
    (y [S, B, N], log_prior [D], log_q [D]).  Backward: bnn_flipout_bwd on the epsilon the forward's prepare launch kept."""

    @staticmethod
    def forward(ctx, x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, call: FlipoutCall):
        S, D = call.n_samples, call.n_draws
        common = dict(seed=call.seed, layer_id=call.layer_id, sample_offset=call.sample_offset, sample_counter=call.sample_counter)
        prep = ops.flipout_prepare(w_mu, w_rho, b_mu, b_rho, n_samples=S, n_draws=D, prior=call.prior, math_mode=call.math_mode,
                                   eps_mode=call.eps_mode, eps_w=eps_w, eps_b=eps_b, want_stats=call.want_stats, want_eps=True, **common)
        y = ops.flipout_fwd(x, prep, w_mu, b_mu, n_samples=S, n_draws=D, math_mode=call.math_mode, relu=call.relu,
                            eps_mode=call.eps_mode, y_dtype=torch.float32, row_offset=call.row_offset, **common)
        ctx.call = call
        ctx.save_for_backward(x, w_mu, w_rho, b_mu, b_rho, prep["eps_w"], prep["eps_b"], y if call.relu else None)
        if call.want_stats:
            return y, prep["log_prior"], prep["log_q"]
        z1 = torch.zeros(D, dtype=torch.float32, device=y.device)
        z2 = torch.zeros(D, dtype=torch.float32, device=y.device)
        ctx.mark_non_differentiable(z1, z2)
        return y, z1, z2

    @staticmethod
    def backward(ctx, gy, glp, glq):
        call: FlipoutCall = ctx.call
        x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, y = ctx.saved_tensors
        _need_f32("FlipoutLinearFn.backward", x, y)
        g_wmu, g_wrho, g_bmu, g_brho, gx = ops.flipout_bwd(
            x, gy.float(), y, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, n_samples=call.n_samples, n_draws=call.n_draws,
            prior=call.prior, relu=call.relu, seed=call.seed, layer_id=call.layer_id, sample_offset=call.sample_offset,
            sample_counter=call.sample_counter, row_offset=call.row_offset,
            g_log_prior=glp if call.want_stats else None, g_log_q=glq if call.want_stats else None,
            want_gx=ctx.needs_input_grad[0])
        if gx is not None and x.dim() == 2:
            gx = gx.sum(0)
        return gx, g_wmu, g_wrho, g_bmu, g_brho, None, None, None


def _uniform_param(lo_hi, *shape):
    return nn.Parameter(torch.empty(*shape).uniform_(*lo_hi))


class FlipoutLinear(nn.Module):
    """Flipout Bayesian FC layer: BayesianLinear's parameters ([out, in] weights) and side-effect attributes."""

    def __init__(self, in_features, out_features, mu_init, rho_init, prior_init, mixture_prior=True):
        super().__init__()
        self.weight_mu = _uniform_param(mu_init, out_features, in_features)
        self.weight_rho = _uniform_param(rho_init, out_features, in_features)
        self.bias_mu = _uniform_param(mu_init, out_features)
        self.bias_rho = _uniform_param(rho_init, out_features)
        self.weight = _Node(self.weight_mu, self.weight_rho)
        self.bias = _Node(self.bias_mu, self.bias_rho)
        self._prior_spec = PriorSpec.from_init(prior_init, bool(mixture_prior))
        self.log_prior = 0
        self.log_variational_posterior = 0
        self._layer_id = 0

    @classmethod
    def view_of(cls, layer):
        """A FlipoutLinear over the SAME Parameters (and `.normal` seam) as a BayesianLinear: no copy."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.weight_mu, self.weight_rho, self.bias_mu, self.bias_rho = layer.weight_mu, layer.weight_rho, layer.bias_mu, layer.bias_rho
        self.weight, self.bias = layer.weight, layer.bias
        self._prior_spec = layer._prior_spec
        self.log_prior = 0
        self.log_variational_posterior = 0
        self._layer_id = layer._layer_id
        return self

    def _eps_stubbed(self):
        return _stubbed(self.weight) or _stubbed(self.bias)

    def forward(self, input, sample=False, calculate_log_probs=False):
        do_sample = self.training or sample
        want = self.training or calculate_log_probs
        injected = _collect_injected([self], 1, input.device) if do_sample else None
        eps_mode = L.EPS_ZERO if not do_sample else (L.EPS_MEMORY if injected is not None else L.EPS_PHILOX)
        call = FlipoutCall(n_samples=1, n_draws=1, prior=self._prior_spec, math_mode=state.math, relu=False, eps_mode=eps_mode,
                           seed=state.seed, layer_id=self._layer_id,
                           sample_offset=take_samples(1) if eps_mode == L.EPS_PHILOX else 0, want_stats=want)
        e_w, e_b = injected[0] if injected is not None else (None, None)
        y, lp, lq = FlipoutLinearFn.apply(input, self.weight_mu, self.weight_rho, self.bias_mu, self.bias_rho, e_w, e_b, call)
        self.log_prior, self.log_variational_posterior = (lp[0], lq[0]) if want else (0, 0)
        return y[0]


def _collect_injected(layers, n_draws: int, device):
    """The identical-eps seam for D base draws: per draw, per layer, weight-shaped then bias-shaped (the reference's order).
    None while every node holds the default `.normal` and BNN_HIP_EPS is not host."""
    if not state.host_eps and not any(l._eps_stubbed() for l in layers):
        return None
    per = [[(l.weight.normal.sample(torch.Size(l.weight_mu.shape)), l.bias.normal.sample(torch.Size(l.bias_mu.shape)))
            for l in layers] for _ in range(n_draws)]
    return [(torch.stack([per[d][i][0].float() for d in range(n_draws)]).to(device).contiguous(),
             torch.stack([per[d][i][1].float() for d in range(n_draws)]).to(device).contiguous()) for i in range(len(layers))]


def _check_math():
    ops._flipout_math(state.math)


class FlipoutNetwork(nn.Module):
    """Three Flipout layers + ReLU and the ELBO assembly: BayesianNetwork's surface (forward, forward_mc, predict_mc, predictive,
    score, sample_elbo, graphed_train_step) with per-row weight noise.  `base_draws` D: how many base draws Delta_d the S MC
    samples of a call share (D | S; D = S gives every sample its own draw -- the epsilon BayesianLinear draws for it)."""

    def __init__(self, model_params, base_draws=1, _view_of=None):
        super().__init__()
        if model_params.get('local_reparam'):
            raise BnnHipError("FlipoutNetwork: Flipout perturbs sampled weights; a local_reparam=True network already draws its "
                              "noise per row -- use BayesianNetwork with local_reparam=True, or set local_reparam=False")
        self.input_shape = model_params['input_shape']
        self.classes = model_params['classes']
        self.batch_size = model_params['batch_size']
        self.hidden_units = model_params['hidden_units']
        self.mode = model_params['mode']
        self.mu_init = model_params['mu_init']
        self.rho_init = model_params['rho_init']
        self.prior_init = model_params['prior_init']
        self.mixture_prior = model_params['mixture_prior']
        self.local_reparam = False
        self.base_draws = int(base_draws)
        if self.base_draws < 1:
            raise BnnHipError("FlipoutNetwork: base_draws must be >= 1")
        if _view_of is not None:
            built = [FlipoutLinear.view_of(l) for l in (_view_of.l1, _view_of.l2, _view_of.l3)]
        else:
            dims = [(self.input_shape, self.hidden_units), (self.hidden_units, self.hidden_units), (self.hidden_units, self.classes)]
            built = [FlipoutLinear(i, o, self.mu_init, self.rho_init, self.prior_init, self.mixture_prior) for i, o in dims]
            for idx, l in enumerate(built):
                l._layer_id = idx
        self.l1 = built[0]
        self.l1_act = nn.ReLU()
        self.l2 = built[1]
        self.l2_act = nn.ReLU()
        self.l3 = built[2]

    @classmethod
    def view_of(cls, net, base_draws=1):
        """BayesianNetwork.flipout(): a FlipoutNetwork on the same Parameters, no copy."""
        if net.local_reparam:
            raise BnnHipError("flipout(): a local_reparam=True network keeps [in, out] weights and a closed-form KL; Flipout "
                              "needs the weight-sampling layers -- build the network with local_reparam=False")
        mp = dict(input_shape=net.input_shape, classes=net.classes, batch_size=net.batch_size, hidden_units=net.hidden_units,
                  mode=net.mode, mu_init=net.mu_init, rho_init=net.rho_init, prior_init=net.prior_init,
                  mixture_prior=net.mixture_prior, local_reparam=False)
        self = cls(mp, base_draws=base_draws, _view_of=net)
        self.train(net.training)
        return self

    # ---- what train.GraphedTrainStep / epoch.EpochRunner read of a network
    def _specs(self):
        from .engine import LayerSpec
        return [LayerSpec(self.l1, self.l1._layer_id, False, True), LayerSpec(self.l2, self.l2._layer_id, False, True),
                LayerSpec(self.l3, self.l3._layer_id, False, False)]

    def _layers(self):
        return [(self.l1, True), (self.l2, True), (self.l3, False)]

    def _flat(self, x):
        if self.mode == 'classification':
            x = x.view(-1, self.input_shape)
        return x

    def _draws(self, samples: int, base_draws=None) -> int:
        D = self.base_draws if base_draws is None else int(base_draws)
        if D < 1 or samples < 1 or samples % D:
            raise BnnHipError(f"Flipout: base_draws ({D}) must divide samples ({samples}); use base_draws=1 or base_draws=samples")
        return D

    def _run(self, x, S: int, D: int, first: int, *, sample: bool, want_stats: bool, injected, differentiable: bool):
        """`S` samples from `D` base draws through the stack: (logits [S, B, C] fp32, [(log_prior [D], log_q [D]) per layer])."""
        _check_math()
        if state.shard_samples:
            raise BnnHipError("Flipout: MC-sample sharding is not supported (a base draw is shared by the samples of its block); "
                              "call bnn_hip.shard_samples(False), or shard minibatches instead")
        if L._recording is not None:
            raise BnnHipError("Flipout: recorded launch lists (capture='calls') are not supported; use graphed_train_step or the "
                              "eager calls")
        ops.require_device(x)
        math_mode = state.math
        hidden = torch.float32 if (differentiable or math_mode == L.MATH_F32) else torch.bfloat16
        if math_mode == L.MATH_F32 and x.dtype != torch.float32:
            x = x.float()
        h, stats = x, []
        layers = self._layers()
        for i, (l, relu) in enumerate(layers):
            last = i == len(layers) - 1
            eps_mode = L.EPS_ZERO if not sample else (L.EPS_MEMORY if injected is not None else L.EPS_PHILOX)
            e_w, e_b = injected[i] if (sample and injected is not None) else (None, None)
            counter = state.device_counter if eps_mode == L.EPS_PHILOX else None
            if differentiable:
                call = FlipoutCall(n_samples=S, n_draws=D, prior=l._prior_spec, math_mode=math_mode, relu=relu, eps_mode=eps_mode,
                                   seed=state.seed, layer_id=l._layer_id, sample_offset=first, want_stats=want_stats,
                                   sample_counter=counter)
                h, lp, lq = FlipoutLinearFn.apply(h, l.weight_mu, l.weight_rho, l.bias_mu, l.bias_rho, e_w, e_b, call)
                stats.append((lp, lq))
                continue
            p = tuple(t.detach() for t in (l.weight_mu, l.weight_rho, l.bias_mu, l.bias_rho))
            common = dict(seed=state.seed, layer_id=l._layer_id, sample_offset=first, sample_counter=counter)
            prep = None
            if sample or math_mode == L.MATH_BF16:
                prep = ops.flipout_prepare(*p, n_samples=S, n_draws=D, prior=l._prior_spec, math_mode=math_mode, eps_mode=eps_mode,
                                           eps_w=e_w, eps_b=e_b, want_stats=want_stats, **common)
                stats.append((prep["log_prior"], prep["log_q"]))
            h = ops.flipout_fwd(h, prep, p[0], p[2], n_samples=S, n_draws=D, math_mode=math_mode, relu=relu, eps_mode=eps_mode,
                                y_dtype=torch.float32 if last else hidden, **common)
        return h, stats

    def forward(self, x, sample=False):
        """One forward: every batch row with its own weight sample when training or `sample`, else the mean network."""
        x = self._flat(x)
        training = self.training
        do_sample = training or sample
        layers = [l for l, _ in self._layers()]
        differentiable = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        injected = _collect_injected(layers, 1, x.device) if do_sample else None
        first = take_samples(1) if (do_sample and injected is None) else 0
        out, stats = self._run(x, 1, 1, first, sample=do_sample, want_stats=training, injected=injected,
                               differentiable=differentiable or training)
        for l, st in zip(layers, stats if training else [None] * 3):
            l.log_prior, l.log_variational_posterior = (st[0][0], st[1][0]) if training else (0, 0)
        return out[0]

    def forward_mc(self, x, samples, base_draws=None):
        """The outputs of `samples` stochastic passes, [samples, batch, classes] fp32, from `base_draws` base draws (default:
        the network's), one prepare launch and one layer launch per layer."""
        S = int(samples)
        D = self._draws(S, base_draws)
        x = self._flat(x)
        injected = _collect_injected([l for l, _ in self._layers()], D, x.device)
        first = take_samples(S) if injected is None else 0
        with torch.no_grad():
            logits, _ = self._run(x, S, D, first, sample=True, want_stats=False, injected=injected, differentiable=False)
        return logits

    def predict_mc(self, x, samples, base_draws=None):
        """(preds [batch], probs [batch, classes]), probs the mean softmax over `samples` Flipout passes."""
        probs, preds = ops.mc_softmax_mean(self.forward_mc(x, samples, base_draws), 1.0 / int(samples))
        return preds, probs

    def predictive(self, x, samples, *, quantiles=None, sigma=1., stacked=False, base_draws=None):
        """The predictive summaries (bnn_hip.ops.Predictive, as BayesianNetwork.predictive) of `samples` Flipout passes."""
        if stacked:
            raise BnnHipError("Flipout: stacked=True is not supported; call predictive once per minibatch")
        if self.mode not in ("classification", "regression"):
            raise Exception("Training mode must be either 'regression' or 'classification'")
        if self.mode == "classification" and quantiles:
            raise BnnHipError("predictive: quantiles are a regression summary")
        from .engine import _first_minibatch
        return _first_minibatch(ops.mc_predictive(self.forward_mc(x, samples, base_draws), self.mode, sigma=float(sigma),
                                                  quantiles=ops.quantile_levels(quantiles)))

    def score(self, x, y, samples, *, sigma=1., bins=10, stacked=False, base_draws=None):
        """The held-out scores (bnn_hip.ops.Scores, as BayesianNetwork.score) of `samples` Flipout passes against `y`."""
        if stacked:
            raise BnnHipError("Flipout: stacked=True is not supported; call score once per minibatch")
        if self.mode not in ("classification", "regression"):
            raise Exception("Training mode must be either 'regression' or 'classification'")
        return ops.mc_score(self.forward_mc(x, samples, base_draws), y, self.mode, sigma=float(sigma), bins=int(bins))

    def log_prior(self):
        return self.l1.log_prior + self.l2.log_prior + self.l3.log_prior

    def log_variational_posterior(self):
        return self.l1.log_variational_posterior + self.l2.log_variational_posterior + self.l3.log_variational_posterior

    def sample_elbo(self, input, target, beta, samples, sigma=1., base_draws=None):
        """The ELBO of `samples` Flipout passes: log q and log p averaged over the base draws, the NLL over the samples; the
        reference's return tuple (loss, log_prior, log_variational_posterior, negative_log_likelihood).  Differentiable."""
        if self.mode not in ('regression', 'classification'):
            raise Exception("Training mode must be either 'regression' or 'classification'")
        S = int(samples)
        D = self._draws(S, base_draws)
        x = self._flat(input)
        layers = [l for l, _ in self._layers()]
        injected = _collect_injected(layers, D, x.device)
        if injected is not None and state.device_counter is not None:
            raise BnnHipError("Flipout: host-drawn or injected epsilon (the .normal seam, BNN_HIP_EPS=host) cannot be captured; "
                              "restore the layers' .normal and use the on-chip generator")
        first = take_samples(S) if injected is None else 0
        differentiable = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        logits, stats = self._run(x, S, D, first, sample=True, want_stats=True, injected=injected, differentiable=differentiable)
        if differentiable:
            nll = NLLFn.apply(logits, target, self.mode, float(sigma))
        else:
            nll = ops.elbo_finalize(workspaces=[], layer_in=[], layer_out=[], local_reparam=False, prior=PriorSpec(), n_samples=S,
                                    logits=logits, target=target, mode=self.mode, nll_sigma=float(sigma))["nll"]
        lp, lq = stats[0]
        for p_, q_ in stats[1:]:
            lp, lq = lp + p_, lq + q_
        log_prior_mean, log_q_mean = lp.sum() / D, lq.sum() / D
        negative_log_likelihood = (nll.sum() / S).reshape(1)
        loss = beta * log_q_mean - beta * log_prior_mean + negative_log_likelihood
        return loss, log_prior_mean, log_q_mean, negative_log_likelihood

    def graphed_train_step(self, optimizer, x, y, samples, base_draws=1, sigma=1., warmup=2):
        """One training step (zero_grad, sample_elbo, backward, FusedAdam.step) for minibatches shaped like (x, y) as ONE
        captured hipGraph with train.GraphedTrainStep's contract: static x / y / beta, the optimiser's shared device sample
        counter (fresh noise each replay), warm-up undone, step / replay, sync_lr -- so epoch.EpochRunner and bnn_hip.tasks
        can drive it.  `optimizer`: bnn_hip.optim.FusedAdam(capturable=True)."""
        return FlipoutTrainStep(self, optimizer, x, y, int(samples), base_draws=base_draws, sigma=float(sigma), warmup=warmup)

    def take_samples(self, S):
        """Reserve S global MC sample indices (as a BBB evaluation of S samples does); returns the first."""
        return take_samples(int(S))


class FlipoutTrainStep(GraphedTrainStep):
    """train.GraphedTrainStep over a FlipoutNetwork.  The captured chain is the autograd one: FlipoutLinearFn per layer (prepare,
    layer, and in the backward bnn_flipout_bwd), NLLFn, the loss in tensor ops, FusedAdam -- exactly what the eager loop runs."""

    def __init__(self, net: FlipoutNetwork, optimizer, x, y, samples: int, base_draws: int = 1, sigma: float = 1.0, warmup: int = 2):
        _check_math()
        if L._recording is not None:
            raise BnnHipError("Flipout: recorded launch lists are not supported; graphed_train_step captures a hipGraph")
        self.base_draws = net._draws(int(samples), base_draws)
        super().__init__(net, optimizer, x, y, int(samples), sigma=sigma, warmup=warmup, autograd=True)

    # GraphedTrainStep.__init__ binds net.sample_elbo; the step's ELBO also carries its base draws
    @property
    def _elbo(self):
        return self._flipout_elbo

    @_elbo.setter
    def _elbo(self, _):
        pass

    def _flipout_elbo(self, x, y, beta, samples, sigma):
        return self.net.sample_elbo(x, y, beta, samples, sigma, base_draws=self.base_draws)
