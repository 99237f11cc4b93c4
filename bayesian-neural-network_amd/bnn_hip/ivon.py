"""F24: IVON for MLP (Shen et al. 2024, "Variational Learning is Effective for Large Deep Networks"; not in the reference) --
natural-gradient variational learning of a diagonal Gaussian N(m, 1 / (ess (h + delta))) per weight at the cost of an Adam step
(csrc/ivon.hip; include/bnn_hip.h F24).

`FusedIVON` takes the optimiser's place in K6's captured training step (dense_train.GraphedDenseTrainStep): per MC sample one
draw launch in front of the forward pass (bnn_ivon_draw: theta = m + sigma eps into the parameter tensors, the noise generated on
chip) and, behind the last backward pass, one step launch over every parameter tensor (bnn_ivon_step).  Between steps the
parameter tensors hold the mean, so mlp(x), state_dict() and every consumer of the network see the mean; the posterior variance
is the optimiser's own Hessian estimate.  From it come the posterior as a BayesianNetwork (`network`) and draws into a
sgmcmc.WeightBank (`sample_bank`), which predicts through the bank's unchanged launches.

Left out: ensemble.EnsembleTrainStep with IVON, the BBB networks, multi-GPU."""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from . import _lib as L
from . import ops
from .capture import word32
from .mcdropout import layers_of
from .ops import BnnHipError
from .runtime import state, take_samples
from .sgmcmc import WeightBank, _read_word, _set_word, _word
from .swag import diag_network

# _dev[0]: every device object a warm-up step changes (capture.snapshot saves and restores them in place); the accumulators
# follow when samples > 1
_LRW, _LR, _STEP, _PROD, _TICKET, _MEAN, _HESS, _GM, _ACC_G, _ACC_H = range(10)


def default_loss_scale(loss: str, batch: int, sigma: Optional[float] = None) -> float:
    """The factor that turns K6's sum loss over a minibatch of `batch` rows into the mean negative log-likelihood IVON is
    defined on: 1 / B for cross-entropy; 1 / (2 sigma^2 B) for mse with the observation noise sigma given, 1 / B otherwise."""
    B = int(batch)
    if B < 1:
        raise ValueError("batch must be >= 1")
    if loss == "cross_entropy":
        return 1.0 / B
    if loss == "mse":
        return 1.0 / B if sigma is None else 1.0 / (2.0 * float(sigma) ** 2 * B)
    raise BnnHipError(f"default_loss_scale: loss must be 'cross_entropy' or 'mse', got {loss!r}")


def require_plain_mlp(mlp, who: str):
    """IVON here trains K6's networks (MLP / MLP_Dropout: a stack of nn.Linear in `mlp.net`); the BBB networks carry their own
    variational parameters and are refused."""
    if not isinstance(getattr(mlp, "net", None), torch.nn.Sequential):
        raise BnnHipError(f"{who}: IVON trains MLP / MLP_Dropout; a {type(mlp).__name__} (the BBB networks have their own "
                          "variational parameters) is not supported")


def beta1_product(beta1: float, step: int) -> float:
    """beta1^step as the step launch keeps it: a running fp64 product, one multiplication per step (no pow)."""
    prod, b = 1.0, float(beta1)
    for _ in range(int(step)):
        prod *= b
        if prod == 0.0:
            break
    return prod


class FusedIVON(torch.optim.Optimizer):
    """IVON over every parameter tensor in one launch per part.  With h the Hessian estimate (state[p]['hess'], initialised
    to hess_init), gm the gradient momentum (state[p]['avg_grad']), delta = weight_decay and c = loss_scale, step t does for
    samples s = 0 .. S - 1

        perturb(s):  theta = m + eps / sqrt(ess (h + delta))                 (s >= 1 also folds sample s - 1's gradient)
        step():      ghat = c mean_s g_s,   hhat = c mean_s g_s eps_s sqrt(ess (h + delta))
                     gm' = beta1 gm + (1 - beta1) ghat
                     h'  = beta2 h + (1 - beta2) hhat + (1 - beta2)^2 (h - hhat)^2 / (2 (h + delta))
                     m'  = m - lr_eff clip((gm' / (1 - beta1^(t+1)) + delta m) / (h' + delta))

    lr_eff = lr (hess_init + delta) with rescale_lr (the authors' package), lr otherwise.  K6's losses are sums over the
    minibatch: `loss_scale=None` lets dense_train.GraphedDenseTrainStep take default_loss_scale(loss, B, sigma); a plain torch
    loop `opt.perturb(); loss.backward(); opt.step()` on a mean loss passes loss_scale=1 (with samples > 1 zero the gradients
    between the samples).  `ess`: the effective sample size, normally the data-set size.  The means live in the parameters
    between steps; inside a step (after perturb) they hold the draw.

    One parameter group.  `capturable=True` keeps the rate in a device word a captured step reads; `param_groups[0]['lr']`
    stays the knob (sync_lr).  The state (flat `mean`, `hess`, `avg_grad` in a WeightBank member's padded layout, the
    accumulators when samples > 1), the step word, the fp64 word beta1^t and the ticket live on the device."""

    def __init__(self, params, lr, ess, hess_init=1.0, beta1=0.9, beta2=0.99999, weight_decay=1e-4, samples=1,
                 clip_radius=float("inf"), rescale_lr=True, loss_scale=None, capturable=True, *, sigma=None, seed=None, mlp=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < ess:
            raise ValueError(f"Invalid effective sample size: {ess}")
        if not 0.0 < hess_init:
            raise ValueError(f"Invalid Hessian initialisation: {hess_init}")
        if not 0.0 <= beta1 < 1.0:
            raise ValueError(f"Invalid beta1: {beta1}")
        if not 0.0 <= beta2 <= 1.0:
            raise ValueError(f"Invalid beta2: {beta2}")
        if not 0.0 < weight_decay:
            raise ValueError(f"Invalid weight_decay (IVON's prior precision per data point must be > 0): {weight_decay}")
        if int(samples) != samples or not 1 <= int(samples) <= L.IVON_MAX_SAMPLES:
            raise BnnHipError(f"FusedIVON: samples must lie in [1, {L.IVON_MAX_SAMPLES}], got {samples}")
        if not 0.0 < clip_radius:
            raise ValueError(f"Invalid clip_radius: {clip_radius}")
        if loss_scale is not None and not 0.0 < loss_scale:
            raise ValueError(f"Invalid loss_scale: {loss_scale}")
        if sigma is not None and not 0.0 < sigma:
            raise ValueError(f"Invalid sigma: {sigma}")
        super().__init__(params, dict(lr=lr, ess=float(ess), hess_init=float(hess_init), beta1=float(beta1), beta2=float(beta2),
                                      weight_decay=float(weight_decay), samples=int(samples), clip_radius=float(clip_radius),
                                      rescale_lr=bool(rescale_lr), capturable=capturable))
        if len(self.param_groups) != 1:
            raise BnnHipError("FusedIVON: the posterior needs all parameters in one group")
        self.loss_scale = None if loss_scale is None else float(loss_scale)
        self.sigma = None if sigma is None else float(sigma)
        self.seed = (state.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        if mlp is not None:
            require_plain_mlp(mlp, "FusedIVON")
        self.mlp = mlp
        ps = self.param_groups[0]["params"]
        if not 1 <= len(ps) <= L.SGMCMC_MAX_TENSORS:
            raise BnnHipError(f"FusedIVON: between 1 and {L.SGMCMC_MAX_TENSORS} parameter tensors, got {len(ps)}")
        dev = self.device = ps[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in ps):
            raise BnnHipError("FusedIVON: the parameters must be float32 tensors on one device")
        self.shapes = [tuple(p.shape) for p in ps]
        self.numels = [p.numel() for p in ps]
        self.offsets, self.stride = ops.bank_layout(self.numels)
        S = int(samples)

        def flat(value=0.0):
            return torch.full((self.stride,), float(value), dtype=torch.float32, device=dev)

        self.mean, self.hess, self.avg_grad = flat(), flat(hess_init), flat()
        self.acc_g, self.acc_h = (flat(), flat()) if S > 1 else (None, None)
        d = [torch.tensor([self.lr_eff()], dtype=torch.float32, device=dev), self.lr_eff(), _word(0, dev),
             torch.ones(1, dtype=torch.float64, device=dev), torch.zeros(16, dtype=torch.int32, device=dev), self.mean, self.hess,
             self.avg_grad]
        if S > 1:
            d += [self.acc_g, self.acc_h]
        self._dev = {0: d}
        for p, h, a in zip(ps, self._views(self.hess), self._views(self.avg_grad)):
            self.state[p]["hess"], self.state[p]["avg_grad"] = h, a
        self._drawn = 0                                   # samples drawn in the step under way

    # ---- the knobs
    def lr_eff(self) -> float:
        """The rate the launch uses: lr (hess_init + weight_decay) with rescale_lr, lr otherwise."""
        g = self.param_groups[0]
        return g["lr"] * (g["hess_init"] + g["weight_decay"]) if g["rescale_lr"] else g["lr"]

    def sync_lr(self):
        """Push param_groups[0]['lr'] (what an lr scheduler changed) into the device word a captured graph reads.  Call
        outside capture, before replaying."""
        d, lr = self._dev[0], self.lr_eff()
        if d[_LR] != lr:
            d[_LRW].fill_(lr)
            d[_LR] = lr

    def device_step(self, gi: int = 0) -> int:
        return _read_word(self._dev[0][_STEP])

    def _views(self, flat: torch.Tensor) -> List[torch.Tensor]:
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]

    def state_dict(self):
        """torch's format: state[p]['hess'] and state[p]['avg_grad'] (views into the flat buffers) and state[p]['step'], the
        device step word mirrored first (one device read)."""
        step = self.device_step()
        for p in self.param_groups[0]["params"]:
            self.state[p]["step"] = step
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Everything a captured training step holds the address of survives the load: the flat buffers, the words and the
        ticket are updated in place; the fp64 word beta1^step is rebuilt by `step` multiplications."""
        g0 = state_dict["param_groups"]
        if len(g0) != 1 or int(g0[0].get("samples", 1)) != self.param_groups[0]["samples"]:
            raise BnnHipError("FusedIVON.load_state_dict: one parameter group of the same `samples` is required")
        ps = self.param_groups[0]["params"]
        keep = [(self.state[p]["hess"], self.state[p]["avg_grad"]) for p in ps]
        super().load_state_dict(state_dict)
        steps = []
        with torch.no_grad():
            for p, (h, a) in zip(self.param_groups[0]["params"], keep):
                st = self.state[p]
                if torch.is_tensor(st.get("hess")) and st["hess"] is not h:
                    h.copy_(st["hess"].view(h.shape))
                if torch.is_tensor(st.get("avg_grad")) and st["avg_grad"] is not a:
                    a.copy_(st["avg_grad"].view(a.shape))
                st["hess"], st["avg_grad"] = h, a
                if "step" in st:
                    steps.append(int(st["step"]))
        d, step = self._dev[0], max(steps) if steps else 0
        _set_word(d[_STEP], step)
        d[_PROD].fill_(beta1_product(self.param_groups[0]["beta1"], step))
        d[_TICKET].zero_()
        d[_LRW].fill_(self.lr_eff())
        d[_LR] = self.lr_eff()
        self._drawn = 0

    # ---- the step's parts
    def _grads(self, ps, what):
        if any(p.grad is None for p in ps):
            raise BnnHipError(f"FusedIVON.{what}: every parameter needs a gradient (the posterior covers all of them)")
        if any(p.grad.is_sparse for p in ps):
            raise RuntimeError("FusedIVON does not support sparse gradients")
        return [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]

    @torch.no_grad()
    def perturb(self, s: int = 0, *, eps_mode: int = L.EPS_PHILOX, noise=None):
        """Draw sample s of the step under way into the parameters (in order: 0 .. samples - 1, then step()); s >= 1 first
        folds the gradients of sample s - 1 (p.grad) into the accumulators.  `noise` ([samples, stride]) with
        eps_mode=EPS_MEMORY, or eps_mode=EPS_ZERO: the draw on given noise (tests)."""
        g = self.param_groups[0]
        s = int(s)
        if s != self._drawn or s >= g["samples"]:
            raise BnnHipError(f"FusedIVON.perturb: sample {s} out of order (the step under way has drawn {self._drawn} of "
                              f"{g['samples']})")
        ps = g["params"]
        d = self._dev[0]
        ops.ivon_draw([p.data for p in ps], hess=d[_HESS], ess=g["ess"], weight_decay=g["weight_decay"], samples=g["samples"],
                      sample=s, mean=d[_MEAN], step=d[_STEP], grads=self._grads(ps, "perturb") if s else None,
                      acc_g=d[_ACC_G] if s else None, acc_h=d[_ACC_H] if s else None, eps_mode=eps_mode, seed=self.seed, noise=noise)
        self._drawn = s + 1

    @torch.no_grad()
    def step(self, closure=None, *, loss_scale: Optional[float] = None, eps_mode: int = L.EPS_PHILOX, noise=None):
        """The update from the gradients at the last draw.  `loss_scale` overrides the optimiser's (a captured step passes the
        one of its loss and batch size)."""
        if closure is not None:
            raise BnnHipError("FusedIVON.step takes no closure: draw with perturb(s), run forward and backward, then step()")
        g = self.param_groups[0]
        S = g["samples"]
        if self._drawn != S:
            raise BnnHipError(f"FusedIVON.step: call perturb(s) for s = 0 .. {S - 1} first (the gradients must be taken at a "
                              f"draw; {self._drawn} of {S} drawn)")
        c = self.loss_scale if loss_scale is None else float(loss_scale)
        if c is None:
            raise BnnHipError("FusedIVON.step: loss_scale is unresolved; pass loss_scale=1 for a mean loss (a "
                              "GraphedDenseTrainStep resolves it from its loss and batch size)")
        ps = g["params"]
        d = self._dev[0]
        lr_dev = None
        if g["capturable"]:
            lr_dev = d[_LRW]
            if not torch.cuda.is_current_stream_capturing():
                self.sync_lr()
        ops.ivon_step([p.data for p in ps], self._grads(ps, "step"), lr=self.lr_eff(), ess=g["ess"], weight_decay=g["weight_decay"],
                      beta1=g["beta1"], beta2=g["beta2"], loss_scale=c, clip_radius=g["clip_radius"], samples=S, lr_device=lr_dev,
                      mean=d[_MEAN], hess=d[_HESS], avg_grad=d[_GM], acc_g=d[_ACC_G] if S > 1 else None,
                      acc_h=d[_ACC_H] if S > 1 else None, step=d[_STEP], beta1_prod=d[_PROD], ticket=d[_TICKET], eps_mode=eps_mode,
                      seed=self.seed, noise=noise)
        self._drawn = 0
        return None

    # ---- the posterior
    def _between_steps(self, what):
        if self._drawn:
            raise BnnHipError(f"FusedIVON.{what}: a step is under way (the parameters hold a draw, not the mean); call step() first")

    def variance(self) -> List[torch.Tensor]:
        """sigma^2 = 1 / (ess (h + delta)), shaped like the parameters (views of one new [stride] tensor)."""
        g = self.param_groups[0]
        return self._views(1.0 / (g["ess"] * (self.hess + g["weight_decay"])))

    def _layer_order(self, what):
        """The network's layers, checked to hold the optimiser's parameters in its order (weight, bias per layer)."""
        if self.mlp is None:
            raise BnnHipError(f"FusedIVON.{what} needs the network: build the optimiser with mlp.ivon(...) or pass mlp=")
        layers = layers_of(self.mlp)
        ps = [t for d in layers for t in (d.linear.weight, d.linear.bias) if t is not None]
        if [id(p) for p in ps] != [id(p) for p in self.param_groups[0]["params"]]:
            raise BnnHipError(f"FusedIVON.{what}: the optimiser must hold the network's parameters in layer order")
        return layers

    def network(self):
        """A networks.BayesianNetwork on the device holding the posterior: mu = the mean (the bits), rho = softplus^-1(sigma)
        (formed in fp64, rounded once), the prior N(0, (ess delta)^-1/2) IVON's weight decay stands for, weight sampling
        (local_reparam=False)."""
        layers = self._layer_order("network")
        self._between_steps("network")
        g = self.param_groups[0]
        s = 1.0 / torch.sqrt(g["ess"] * (self.hess.double() + g["weight_decay"]))
        rho = (s + torch.log(-torch.expm1(-s))).float()
        return diag_network(self.mlp, layers, self.device, [p.data for p in g["params"]], self._views(rho),
                            prior_sigma=1.0 / math.sqrt(g["ess"] * g["weight_decay"]), who="FusedIVON.network")

    def sample_bank(self, members: int, bank: Optional[WeightBank] = None, sample_offset: Optional[int] = None, *,
                    members_per_launch: Optional[int] = None):
        """Fill slots 0 .. members - 1 of a sgmcmc.WeightBank (a new one of that capacity by default) with draws theta = m +
        sigma eps and return the bank: bank.predict_mc / predictive / score / evaluate run unchanged.  Draw j uses the global
        sample index sample_offset + j (by default the next `members` of the process-wide counter), whatever the chunking
        (`members_per_launch`, at most IVON_MAX_MEMBERS): the same offset gives the same bits.  A bank passed in has its slots
        0 .. members - 1 overwritten and its `collected` word raised to `members` if it held fewer."""
        M = int(members)
        if M < 1:
            raise BnnHipError(f"FusedIVON.sample_bank: members must be >= 1, got {members}")
        self._layer_order("sample_bank")
        self._between_steps("sample_bank")
        if bank is None:
            bank = WeightBank(self.mlp, M)
        elif bank.capacity < M or bank.shapes != self.shapes:
            raise BnnHipError(f"FusedIVON.sample_bank: the bank must hold {M} members of this network's parameter shapes")
        base = take_samples(M) if sample_offset is None else int(sample_offset)
        chunk = L.IVON_MAX_MEMBERS if members_per_launch is None else int(members_per_launch)
        if not 1 <= chunk <= L.IVON_MAX_MEMBERS:
            raise BnnHipError(f"FusedIVON.sample_bank: members_per_launch must lie in [1, {L.IVON_MAX_MEMBERS}]")
        g = self.param_groups[0]
        with torch.no_grad():
            for first in range(0, M, chunk):
                ops.ivon_draw([p.data for p in g["params"]], hess=self.hess, ess=g["ess"], weight_decay=g["weight_decay"],
                              bank=bank.buffer, members=min(chunk, M - first), first=first, seed=self.seed,
                              sample_base=word32(base + first) & 0xFFFFFFFF)
        if bank.count() < M:
            _set_word(bank.collected, M)
        return bank
