"""F21: training a deep ensemble (Lakshminarayanan et al. 2017; not in the reference) -- every member of a sgmcmc.WeightBank
per launch (csrc/ensemble.hip; include/bnn_hip.h F21).

`DeepEnsemble` holds M weight sets of an MLP / MLP_Dropout in a WeightBank and hands the optimiser ONE parameter: the bank's
buffer, flat.  `EnsembleTrainStep` is dense_train.GraphedDenseTrainStep for all M members at once:

  bnn_ens_fwd per layer (member j's kind-3 dropout mask at global sample index base + counter + j; the output layer's launch
  advances the device counter by M)  ->  bnn_ens_loss (loss[j], logits gradient, one block per member)  ->  bnn_ens_bwd per
  layer, top down (gradients into a bucket [M, stride] in the bank's layout)  ->  bnn_sgd_step / bnn_adam_step over the two
  flat tensors.

Three layers: 3 + 1 + 3 + 1 = 8 launches whatever M, captured once (11 with a svgd.SteinTransform, F23, which rewrites the bucket
into the SVGD / kde-WGD direction ahead of the optimiser's launch).  The step works in place on the bank's buffer: after any
number of steps bank.predictive(x) is the ensemble's predictive with nothing copied.  Per member every launch is bit-equal to
the single-network launch of K6, so M = 1 is a plain GraphedDenseTrainStep and member j of an M-member step t equals an
independent K6 step whose sample counter stands at base + M t + j."""
from __future__ import annotations

import copy
from typing import Optional, Sequence

import torch
from torch import nn

from . import ops
from .capture import SampleCounter, snapshot, warm_up
from .mcdropout import _math, flat_input
from .ops import BnnHipError
from .ivon import FusedIVON
from .optim import FusedAdam, FusedSGD, _sgd_supported
from .runtime import state
from .sgmcmc import FusedSGMCMC, WeightBank

LOSSES = ("cross_entropy", "mse")


def seeded_copy(mlp, seed: int):
    """A deep copy of `mlp` whose Linears were re-initialised, in layer order, by reset_parameters() under
    torch.manual_seed(seed) -- inside torch.random.fork_rng(), so the caller's generators and `mlp` are left untouched."""
    net = copy.deepcopy(mlp)
    with torch.random.fork_rng():
        torch.manual_seed(int(seed))
        for m in net.net:
            if isinstance(m, nn.Linear):
                m.reset_parameters()
    return net


class DeepEnsemble:
    """`members` weight sets of `mlp` (MLP or MLP_Dropout) in `self.bank`, a WeightBank of that capacity.  With `seeds` (one
    per member) member j is seeded_copy(mlp, seeds[j]); without, the caller pushes them (`ens.bank.push(net)`).
    `parameters()` is one nn.Parameter sharing the bank buffer's storage: what FusedSGD / FusedAdam(capturable=True) are
    built on; the padding between a member's tensors has zero gradients and stays exactly zero."""

    def __init__(self, mlp, members: int, seeds: Optional[Sequence[int]] = None):
        self.mlp, self.members = mlp, int(members)
        if self.members < 1:
            raise BnnHipError("DeepEnsemble: members must be >= 1")
        self.bank = WeightBank(mlp, self.members)
        self._param = nn.Parameter(self.bank.buffer.view(-1), requires_grad=True)
        if seeds is not None:
            seeds = [int(s) for s in seeds]
            if len(seeds) != self.members:
                raise BnnHipError(f"DeepEnsemble: {self.members} members need {self.members} seeds, got {len(seeds)}")
            for s in seeds:
                self.bank.push(seeded_copy(mlp, s))

    def parameters(self):
        return [self._param]

    def member(self, j: int, into=None):
        """Copy member j into a network (`into`, by default a deep copy of the ensemble's network); returns the network."""
        return self.bank.member(j, copy.deepcopy(self.mlp) if into is None else into)

    def state_dict(self) -> dict:
        return self.bank.state_dict()

    def load_state_dict(self, sd: dict):
        """In place: the buffer keeps its address (the parameter, a captured step and a captured predictive hold it)."""
        self.bank.load_state_dict(sd)

    def graphed_train_step(self, optimizer, x, y, loss=None, capture: bool = True, transform=None) -> "EnsembleTrainStep":
        return EnsembleTrainStep(self, optimizer, x, y, loss=loss, capture=capture, transform=transform)

    def svgd(self, *, dataset_size, batch_size, prior_precision: float = 1.0, temperature: float = 1.0, method: str = "svgd",
             bandwidth=None):
        """A svgd.SteinTransform over this ensemble's members (F23): pass it as `transform=` to graphed_train_step and the
        members are trained as SVGD particles (method="svgd") or as a kde-WGD repulsive ensemble ("wgd") instead of
        independently.  The prior enters through `prior_precision`: build the optimiser with weight_decay = 0."""
        from .svgd import SteinTransform
        return SteinTransform(self, dataset_size=dataset_size, batch_size=batch_size, prior_precision=prior_precision,
                              temperature=temperature, method=method, bandwidth=bandwidth)


class EnsembleTrainStep:
    def __init__(self, ens: DeepEnsemble, optimizer, x: torch.Tensor, y: torch.Tensor, loss=None, capture: bool = True,
                 transform=None):
        """`x`, `y`: an example minibatch -- the single network's shapes ([B, ...]: one minibatch shared by all members) or
        with a leading member dimension ([M, B, ...]: a minibatch per member); y follows x.  `optimizer`: FusedSGD or
        FusedAdam with capturable=True built on ens.parameters().  `loss`, `capture`: as GraphedDenseTrainStep.
        `transform`: a svgd.SteinTransform of this ensemble (ens.svgd(...)): its three launches rewrite the gradient bucket
        between the last bnn_ens_bwd and the optimiser's launch (11 launches instead of 8); None: independent members.

        Building the step runs one real warm-up step and then restores the bank, the optimiser state and the sample
        counter."""
        mlp, M = ens.mlp, ens.members
        if isinstance(optimizer, FusedSGMCMC):
            raise BnnHipError("EnsembleTrainStep: FusedSGMCMC is not supported (SG-MCMC chains per member are out of scope); "
                              "use FusedSGD or FusedAdam")
        if isinstance(optimizer, FusedIVON):
            raise BnnHipError("EnsembleTrainStep: FusedIVON is not supported (a posterior per member is out of scope); train "
                              "one network with mlp.graphed_train_step(mlp.ivon(...), x, y), or use FusedSGD or FusedAdam")
        if not isinstance(optimizer, (FusedSGD, FusedAdam)):
            raise BnnHipError("EnsembleTrainStep needs FusedSGD or FusedAdam (capturable=True)")
        if not all(g.get("capturable") for g in optimizer.param_groups):
            raise BnnHipError("EnsembleTrainStep needs a capturable optimiser (capturable=True)")
        if len(optimizer.param_groups) != 1:
            raise BnnHipError("EnsembleTrainStep: the optimiser must have one parameter group")
        ps = optimizer.param_groups[0]["params"]
        if len(ps) != 1 or ps[0] is not ens._param:
            raise BnnHipError("EnsembleTrainStep: the optimiser must be built on ens.parameters()")
        if isinstance(optimizer, FusedSGD):
            _sgd_supported(optimizer.param_groups[0])
        if state.shard_samples:
            raise BnnHipError("EnsembleTrainStep: MC-sample sharding is not supported; switch it off")
        if loss is None:
            loss = "cross_entropy" if mlp.mode == "classification" else "mse"
        if loss not in LOSSES:
            raise BnnHipError(f"EnsembleTrainStep: loss must be one of {LOSSES}, got {loss!r}")
        ops.require_device(x, y)
        self.layers = ens.bank.layers
        for d in self.layers[:-1]:
            if d.p and not d.relu:
                raise BnnHipError("EnsembleTrainStep: a Dropout needs a ReLU before it (the backward reads the mask off the "
                                  "layer's saved output)")
        if ens.bank.count() != M:
            raise BnnHipError(f"EnsembleTrainStep: the bank holds {ens.bank.count()} of {M} members; push the rest first "
                              "(ens.bank.push(net)) or give seeds")
        if transform is not None and (getattr(transform, "ens", None) is not ens or not callable(getattr(transform, "enqueue", None))):
            raise BnnHipError("EnsembleTrainStep: the transform must be built on this ensemble (ens.svgd(...))")
        self.ens, self.bank, self.opt, self.members, self.transform = ens, ens.bank, optimizer, M, transform
        self.loss_mode = "classification" if loss == "cross_entropy" else "regression"
        self.per_member = x.dim() == (5 if mlp.mode == "classification" else 3)
        if self.per_member:
            if x.shape[0] != M:
                raise BnnHipError(f"EnsembleTrainStep: a per-member minibatch must be [{M}, batch, ...], got {tuple(x.shape)}")
            xf = flat_input(mlp, x.reshape((-1,) + tuple(x.shape[2:])))
            self.x = xf.reshape(M, x.shape[1], -1).clone().contiguous()
        else:
            self.x = flat_input(mlp, x).clone().contiguous()
        B, dev = self.x.shape[-2], self.x.device
        C_out = self.layers[-1].linear.out_features
        copies = M if self.per_member else 1
        if self.loss_mode == "classification":
            if y.dtype != torch.int64 or y.numel() != copies * B:
                raise BnnHipError("EnsembleTrainStep: cross-entropy targets must be int64 labels, one per row")
        elif y.dtype != torch.float32 or y.numel() != copies * B * C_out:
            raise BnnHipError(f"EnsembleTrainStep: mse targets must be float32 with {copies * B * C_out} elements")
        self.y = y.clone().contiguous()
        self.math = _math()[0]

        # the gradient bucket in the bank's layout; the parameter's gradient is the bucket, flat
        stride = self.bank.stride
        self.bucket = torch.zeros((M, stride), dtype=torch.float32, device=dev)
        self._grad = self.bucket.view(-1)
        self.acts = [torch.empty((M, B, d.linear.out_features), dtype=torch.float32, device=dev) for d in self.layers]
        self.g_logits = torch.empty((M, B, C_out), dtype=torch.float32, device=dev)
        self.g_hidden = [torch.empty((M, B, d.linear.out_features), dtype=torch.float32, device=dev) for d in self.layers[:-1]]
        self.loss = torch.zeros((M,), dtype=torch.float32, device=dev)
        self.scales = [ops.dropout_params(d.p)[1] for d in self.layers]
        self.launches = 2 * len(self.layers) + 2 + (transform.launches if transform is not None else 0)

        sh = self._shared = SampleCounter.of(optimizer, dev)
        self.counter, self.base = sh["counter"], sh["base"]
        sh.sync()

        self.graph = None
        if capture:
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
        bank, M = self.bank, self.members
        with torch.no_grad():
            last = len(self.layers) - 1
            h = self.x
            for i, d in enumerate(self.layers):
                ops.ens_fwd(h, bank.buffer, bank._w_off[i], bank._b_off[i], out_features=d.linear.out_features, members=M,
                            relu=d.relu, drop_p=d.p, layer_id=d.layer_id, seed=state.seed, sample_offset=self.base,
                            sample_counter=self.counter, sample_counter_inc=M if i == last else 0, math_mode=self.math,
                            out=self.acts[i])
                h = self.acts[i]
            ops.ens_loss(self.acts[-1], self.y, self.loss_mode, loss=self.loss, g_logits=self.g_logits)
            for i in range(last, -1, -1):
                below = self.layers[i - 1] if i > 0 else None
                ops.ens_bwd(self.x if i == 0 else self.acts[i - 1], self.g_logits if i == last else self.g_hidden[i],
                            bank.buffer, bank._w_off[i], self.bucket, bank._b_off[i],
                            g_x=self.g_hidden[i - 1] if i > 0 else None, gx_mask=below is not None and below.relu,
                            gx_scale=self.scales[i - 1] if i > 0 else 1.0, math_mode=self.math)
            if self.transform is not None:
                self.transform.enqueue(self.bank, self.bucket)
        self.ens._param.grad = self._grad
        if isinstance(self.opt, FusedAdam):
            self.opt._bump = None                # the sample counter advances in the forward, not in Adam's launch
        self.opt.step()

    # ---- the public step
    def step(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """One optimiser step of every member on minibatch (x, y) of the example's shapes; returns the static [M] loss
        tensor (read it before the next call)."""
        ops.require_device(x, y)
        if x.dtype != torch.float32 or x.numel() != self.x.numel() or y.numel() != self.y.numel() or y.dtype != self.y.dtype:
            raise BnnHipError("EnsembleTrainStep.step: the minibatch must have the example's shape and dtype")
        if x.is_contiguous() and y.is_contiguous():
            ops.stage_inputs(x, self.x, y, self.y)                        # one launch instead of two
        else:
            self.x.copy_(x.reshape(self.x.shape), non_blocking=True)
            self.y.copy_(y.reshape(self.y.shape), non_blocking=True)
        return self.replay()

    def replay(self) -> torch.Tensor:
        """The step on whatever the static buffers (x, y) hold; GraphedDenseTrainStep.replay's bookkeeping, the sample
        counter advancing by M."""
        self.opt.sync_lr()
        self._shared.sync()
        if self.graph is not None:
            self.ens._param.grad = self._grad
            self.graph.replay()
        else:
            self._enqueue()
        self._shared.advance(self.members)
        return self.loss
