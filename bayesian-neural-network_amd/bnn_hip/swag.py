"""F22: SWAG for MLP (Maddox et al. 2019; not in the reference) -- a Gaussian with a diagonal-plus-low-rank covariance fitted
to the iterates of plain SGD (csrc/swag.hip; include/bnn_hip.h F22).

`FusedSWAG` is torch.optim.SGD (momentum, weight decay) in the optimiser's place of K6's captured training step
(dense_train.GraphedDenseTrainStep): every parameter tensor in one launch (bnn_swag_step), and the launch of a collecting step
also folds the new iterate into the running mean, the Welford second moment and the ring of the last `rank` deviations of a
`SwagPosterior` -- an epoch driven by epoch.EpochRunner fits the posterior with no host decision.  From the posterior come the
SWA point estimate (`swa`), SWAG-Diagonal as a BayesianNetwork (`network`) and full SWAG as draws into a sgmcmc.WeightBank
(`sample_bank`, bnn_swag_sample: the moments read once per launch, the normals generated on chip), which predicts through the
bank's unchanged launches."""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib as L
from . import ops
from .capture import word32
from .mcdropout import layers_of
from .ops import BnnHipError
from .runtime import state, take_samples
from .sgmcmc import WeightBank, _read_word, _set_word, _word


def diag_rho(m2: torch.Tensor, n: int, scale: float = 1.0, var_clamp: float = 1e-30) -> torch.Tensor:
    """float32 rho = softplus^-1(sqrt(scale * max(m2 / n, var_clamp))) of SWAG-Diagonal, formed in fp64 and rounded once
    (softplus^-1(s) = s + log(-expm1(-s)): no overflow at large s, no cancellation at small s)."""
    s = torch.sqrt(float(scale) * torch.clamp(m2.double() / float(n), min=float(var_clamp)))
    return (s + torch.log(-torch.expm1(-s))).float()


def require_three_layers(mlp, layers, who: str):
    """Refuse a network that is not BayesianNetwork's in -> hidden -> hidden -> classes with ReLUs between the layers."""
    m = mlp
    if [(d.relu, d.linear.in_features, d.linear.out_features) for d in layers] != \
            [(True, m.input_shape, m.hidden_units), (True, m.hidden_units, m.hidden_units), (False, m.hidden_units, m.classes)]:
        raise BnnHipError(f"{who}: BayesianNetwork has three layers in -> hidden -> hidden -> classes with "
                          "ReLUs between them; this network has another architecture")


def diag_network(mlp, layers, device, means, rhos, *, prior_sigma: float = 1.0, who: str):
    """A networks.BayesianNetwork on `device` holding a diagonal Gaussian over `mlp`'s parameters: mu = `means` (the bits),
    rho = `rhos` (both lists in layer order: weight, bias), a N(0, prior_sigma) prior, weight sampling (local_reparam=False).
    Refuses a network that is not BayesianNetwork's three layers.  SwagPosterior.network and FusedIVON.network build on it."""
    import networks
    m = mlp
    require_three_layers(mlp, layers, who)
    mp = dict(input_shape=m.input_shape, classes=m.classes, batch_size=m.batch_size, hidden_units=m.hidden_units,
              mode=m.mode, mu_init=[-0.2, 0.2], rho_init=[-5.0, -4.0], prior_init=[float(prior_sigma)], mixture_prior=False,
              local_reparam=False)
    with torch.device(device):
        net = networks.BayesianNetwork(mp)
    net.to(device)
    lays = (net.l1, net.l2, net.l3)
    mus = [t.data for l in lays for t in (l.weight_mu, l.bias_mu)]
    rho_params = [t.data for l in lays for t in (l.weight_rho, l.bias_rho)]
    with torch.no_grad():
        for mu, rho, a, r in zip(mus, rho_params, means, rhos):
            mu.copy_(a.view(mu.shape))
            rho.copy_(r.view(rho.shape))
    return net


class SwagPosterior:
    """The moments of SWAG over `mlp`'s parameters, on the device in the layout of one member of a sgmcmc.WeightBank (element i
    of parameter tensor t at offsets[t] + i): `mean` [stride], `m2` [stride] (Welford: m2 / count is the population variance
    of the collected iterates), `dev` [rank, stride] (the last min(count, rank) deviations iterate - running mean, a ring on
    count % rank; None when rank = 0: SWAG-Diagonal only) and the device words `count` (iterates collected) and `step`
    (optimiser steps taken), which a FusedSWAG advances inside its launch."""

    def __init__(self, mlp, rank: int = 20):
        self.mlp, self.rank = mlp, int(rank)
        if not 0 <= self.rank <= L.SWAG_MAX_RANK:
            raise BnnHipError(f"SwagPosterior: rank must lie in [0, {L.SWAG_MAX_RANK}], got {rank}")
        self.layers = layers_of(mlp)
        self.params = [t for d in self.layers for t in (d.linear.weight, d.linear.bias) if t is not None]
        if len(self.params) > L.SGMCMC_MAX_TENSORS:
            raise BnnHipError(f"SwagPosterior: at most {L.SGMCMC_MAX_TENSORS} parameter tensors")
        ops.require_device(*self.params)
        self.shapes = [tuple(p.shape) for p in self.params]
        self.numels = [p.numel() for p in self.params]
        self.offsets, self.stride = ops.bank_layout(self.numels)
        off = dict(zip(map(id, self.params), self.offsets))
        self._w_off = [off[id(d.linear.weight)] for d in self.layers]
        self._b_off = [None if d.linear.bias is None else off[id(d.linear.bias)] for d in self.layers]
        dev = self.device = self.params[0].device
        self.mean = torch.zeros(self.stride, dtype=torch.float32, device=dev)
        self.m2 = torch.zeros(self.stride, dtype=torch.float32, device=dev)
        self.dev = torch.zeros((self.rank, self.stride), dtype=torch.float32, device=dev) if self.rank else None
        self.count_word = _word(0, dev)
        self.step_word = _word(0, dev)

    # ---- the moments
    def count(self) -> int:
        """Iterates collected.  One device read."""
        return _read_word(self.count_word)

    def _views(self, flat: torch.Tensor) -> List[torch.Tensor]:
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]

    def mean_views(self) -> List[torch.Tensor]:
        """The running mean, shaped like the parameters (views of `mean`)."""
        return self._views(self.mean)

    def variance(self) -> List[torch.Tensor]:
        """m2 / count, shaped like the parameters (views of one new [stride] tensor)."""
        n = self.count()
        if n < 1:
            raise BnnHipError("SwagPosterior.variance: nothing has been collected yet")
        return self._views(self.m2 / float(n))

    def _params_of(self, net):
        ps = [t for d in layers_of(net) for t in (d.linear.weight, d.linear.bias) if t is not None]
        if [tuple(p.shape) for p in ps] != self.shapes:
            raise BnnHipError("SwagPosterior: the network's parameter shapes are not the posterior's")
        return ps

    def swa(self, into=None):
        """Copy the mean (the SWA point estimate) into a network (`into`, by default the posterior's own); returns it."""
        net = self.mlp if into is None else into
        if self.count() < 1:
            raise BnnHipError("SwagPosterior.swa: nothing has been collected yet")
        with torch.no_grad():
            for v, p in zip(self.mean_views(), self._params_of(net)):
                p.copy_(v)
        return net

    def state_dict(self) -> dict:
        return dict(mean=self.mean.clone(), m2=self.m2.clone(), dev=None if self.dev is None else self.dev.clone(),
                    count=self.count(), step=_read_word(self.step_word), rank=self.rank, shapes=[list(s) for s in self.shapes])

    def load_state_dict(self, sd: dict):
        """In place: the moments and the words keep their addresses (a captured step holds them)."""
        if int(sd["rank"]) != self.rank or [tuple(s) for s in sd["shapes"]] != self.shapes:
            raise BnnHipError("SwagPosterior.load_state_dict: another rank or other parameter shapes")
        self.mean.copy_(sd["mean"])
        self.m2.copy_(sd["m2"])
        if self.dev is not None:
            self.dev.copy_(sd["dev"])
        _set_word(self.count_word, int(sd["count"]))
        _set_word(self.step_word, int(sd["step"]))

    # ---- full SWAG: draws into a bank
    def sample_bank(self, members: int, bank: Optional[WeightBank] = None, *, scale: float = 1.0, low_rank: bool = True,
                    var_clamp: float = 1e-30, sample_offset: Optional[int] = None, members_per_launch: Optional[int] = None):
        """Fill slots 0 .. members - 1 of a sgmcmc.WeightBank (a new one of that capacity by default) with draws
        theta = mean + sqrt(scale / 2) sqrt(max(m2 / n, var_clamp)) z1 + sqrt(scale / (2 (Keff - 1))) D^T z2 (low_rank=False:
        mean + sqrt(scale) sqrt(...) z1, SWAG-Diagonal) and return the bank: bank.predict_mc / predictive / score / evaluate /
        predictive_graph then run unchanged.  Draw s uses the global sample index sample_offset + s (by default the next
        `members` of the process-wide counter), whatever the chunking (`members_per_launch`, at most SWAG_MAX_MEMBERS): the
        same offset gives the same bits.  A bank passed in has its slots 0 .. members - 1 overwritten; its `collected` word
        is raised to `members` if it held fewer and is otherwise left alone (KronLaplace.sample_bank's contract)."""
        M = int(members)
        if M < 1:
            raise BnnHipError(f"SwagPosterior.sample_bank: members must be >= 1, got {members}")
        if low_rank and self.rank == 0:
            raise BnnHipError("SwagPosterior.sample_bank: a rank-0 posterior holds no deviations; pass low_rank=False "
                              "(SWAG-Diagonal)")
        if self.count() < 2:
            raise BnnHipError(f"SwagPosterior.sample_bank: {self.count()} iterate(s) collected; a covariance needs at least 2")
        if bank is None:
            bank = WeightBank(self.mlp, M)
        elif bank.capacity < M or bank.shapes != self.shapes:
            raise BnnHipError(f"SwagPosterior.sample_bank: the bank must hold {M} members of this network's parameter shapes")
        base = take_samples(M) if sample_offset is None else int(sample_offset)
        chunk = L.SWAG_MAX_MEMBERS if members_per_launch is None else int(members_per_launch)
        if not 1 <= chunk <= L.SWAG_MAX_MEMBERS:
            raise BnnHipError(f"SwagPosterior.sample_bank: members_per_launch must lie in [1, {L.SWAG_MAX_MEMBERS}]")
        with torch.no_grad():
            for first in range(0, M, chunk):
                ops.swag_sample(self.numels, self.mean, self.m2, self.dev, self.count_word, bank.buffer,
                                members=min(chunk, M - first), first=first, scale=scale, low_rank=low_rank, var_clamp=var_clamp,
                                seed=state.seed, sample_base=word32(base + first) & 0xFFFFFFFF)
        if bank.count() < M:                                                  # (a fuller bank, or a wrapped ring, keeps its word)
            _set_word(bank.collected, M)
        return bank

    # ---- SWAG-Diagonal as a BayesianNetwork
    def network(self, scale: float = 1.0, var_clamp: float = 1e-30):
        """A networks.BayesianNetwork on the device holding SWAG-Diagonal: mu = the mean (the bits), rho =
        softplus^-1(sqrt(scale * max(m2 / n, var_clamp))) (diag_rho), a N(0, 1) prior, weight sampling (local_reparam=False)."""
        # (diag_network checks this again; the call here keeps the refusals in their order: the architecture, then the count)
        require_three_layers(self.mlp, self.layers, "SwagPosterior.network")
        n = self.count()
        if n < 2:
            raise BnnHipError(f"SwagPosterior.network: {n} iterate(s) collected; a variance needs at least 2")
        return diag_network(self.mlp, self.layers, self.device, self.mean_views(),
                            self._views(diag_rho(self.m2, n, scale, var_clamp)), who="SwagPosterior.network")


# ---------------------------------------------------------------------------------------------------- the collector
# _dev[gi]: every device object a warm-up step changes (capture.snapshot saves and restores them in place)
_LRW, _LR, _STEP, _COUNT, _TICKET, _MEAN, _M2, _DEV = range(8)


def _swag_supported(group):
    """dampening, nesterov and maximize are torch.optim.SGD features FusedSWAG does not implement: refuse them."""
    if group.get("dampening", 0) != 0 or group.get("nesterov", False) or group.get("maximize", False):
        raise BnnHipError("FusedSWAG: dampening, nesterov and maximize are not supported (momentum and weight decay are)")


class FusedSWAG(torch.optim.Optimizer):
    """torch.optim.SGD(params, lr, momentum, weight_decay) -- dampening 0, no nesterov; state[p]['momentum_buffer'] -- over
    every parameter tensor in one launch (bnn_swag_step) that also collects SWAG's moments into `swag` (a SwagPosterior of the
    network these parameters belong to): optimiser step k (counted from 0 on the device) collects when k >= start and
    (k - start + 1) % every == 0 -- with `start` = the pre-training steps and `every` = the steps of an epoch, at the end of
    every SWA epoch.  The parameter groups carry torch.optim.SGD's keys (plus `capturable`), so state dicts interchange with
    it.  `capturable=True` keeps the learning rate in a device word a captured training step reads
    (dense_train.GraphedDenseTrainStep); `param_groups[i]['lr']` stays the knob (sync_lr): StepLR, or a constant SWA rate
    switched in on the host, both work.  The step and count words, the ticket and the moments live on the device either way."""

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, *, start=0, every=1, swag: SwagPosterior,
                 capturable=True, dampening=0.0, nesterov=False, maximize=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if int(start) < 0 or int(every) < 1:
            raise ValueError("start must be >= 0 and every >= 1")
        _swag_supported(dict(dampening=dampening, nesterov=nesterov, maximize=maximize))
        if not isinstance(swag, SwagPosterior):
            raise BnnHipError("FusedSWAG: `swag` must be a SwagPosterior")
        super().__init__(params, dict(lr=lr, momentum=float(momentum), dampening=0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False, foreach=None, differentiable=False, fused=None, capturable=capturable))
        self.start, self.every, self.swag = int(start), int(every), swag
        if len(self.param_groups) != 1:
            raise BnnHipError("FusedSWAG: a posterior needs all parameters in one group")
        self._check_shapes(self.param_groups[0]["params"])
        self._dev = {}
        self._group_dev(0, self.param_groups[0], swag.device)
        if momentum != 0:
            # created here, zeroed (torch's first step leaves buf = g', as fma(mu, 0, g') does): a captured step holds their
            # addresses, and the warm-up's undo finds them in the saved state
            for p in self.param_groups[0]["params"]:
                self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _check_shapes(self, ps):
        if [tuple(p.shape) for p in ps] != self.swag.shapes:
            raise BnnHipError("FusedSWAG: the posterior was built for a network of other parameter shapes")
        if any(p.device != self.swag.device for p in ps):
            raise BnnHipError("FusedSWAG: the posterior lives on another device than the parameters")

    def _group_dev(self, gi, group, device):
        if gi not in self._dev:
            s = self.swag
            d = [torch.tensor([group["lr"]], dtype=torch.float32, device=device), group["lr"], s.step_word, s.count_word,
                 torch.zeros(16, dtype=torch.int32, device=device), s.mean, s.m2]
            if s.dev is not None:
                d.append(s.dev)
            self._dev[gi] = d
        return self._dev[gi]

    def sync_lr(self):
        """Push param_groups[i]['lr'] (what an lr scheduler changed) into the device word a captured graph reads.  Call
        outside capture, before replaying."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev and self._dev[gi][_LR] != group["lr"]:
                self._dev[gi][_LRW].fill_(group["lr"])
                self._dev[gi][_LR] = group["lr"]

    def device_step(self, gi: int = 0) -> int:
        return _read_word(self._dev[gi][_STEP]) if gi in self._dev else 0

    def state_dict(self):
        """torch.optim.SGD's format; the device step word is mirrored into state[p]['step'] first (one device read)."""
        step = self.device_step(0)
        for p in self.param_groups[0]["params"]:
            self.state[p]["step"] = step
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch.optim.SGD's format (a state dict of either optimiser).  Everything a captured training step holds the
        address of survives the load: the momentum tensors, the learning-rate word, the step word and the ticket are
        updated in place.  The moments and the count are the posterior's (SwagPosterior.load_state_dict)."""
        for g in state_dict["param_groups"]:
            _swag_supported(g)
        cap = self.param_groups[0]["capturable"]
        keep = {p: self.state[p]["momentum_buffer"] for g in self.param_groups for p in g["params"]
                if p in self.state and torch.is_tensor(self.state[p].get("momentum_buffer"))}
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            g.setdefault("capturable", cap)
        for p, m in keep.items():
            st = self.state.get(p)
            if st is not None and torch.is_tensor(st.get("momentum_buffer")) and st["momentum_buffer"] is not m:
                m.copy_(st["momentum_buffer"])
                st["momentum_buffer"] = m
        group = self.param_groups[0]
        steps = [int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]]
        d = self._dev[0]
        if steps:
            _set_word(d[_STEP], max(steps))
        d[_TICKET].zero_()
        d[_LRW].fill_(group["lr"])
        d[_LR] = group["lr"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        _swag_supported(group)
        ps = group["params"]
        if any(p.grad is None for p in ps):
            raise BnnHipError("FusedSWAG: every parameter needs a gradient (the moments cover all of them)")
        if any(p.grad.is_sparse for p in ps):
            raise RuntimeError("FusedSWAG does not support sparse gradients")
        self._check_shapes(ps)
        gs = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
        ms = None
        if group["momentum"] != 0:
            ms = []
            for p in ps:
                st = self.state[p]
                if not torch.is_tensor(st.get("momentum_buffer")):
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ms.append(st["momentum_buffer"])
        d = self._group_dev(0, group, ps[0].device)
        lr_dev = None
        if group["capturable"]:
            lr_dev = d[_LRW]
            if not torch.cuda.is_current_stream_capturing():
                self.sync_lr()
        s = self.swag
        ops.swag_step(ps, gs, lr=group["lr"], momentum=group["momentum"], weight_decay=group["weight_decay"], lr_device=lr_dev,
                      momenta=ms, start=self.start, every=self.every, mean=s.mean, m2=s.m2, dev=s.dev, step=d[_STEP],
                      count=d[_COUNT], ticket=d[_TICKET])
        return loss
