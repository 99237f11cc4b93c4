"""F19: stochastic-gradient MCMC for MLP (not in the reference) and a device-resident bank of weight snapshots that predicts
as an ensemble (csrc/sgmcmc.hip; include/bnn_hip.h F19).

`FusedSGMCMC` is the sampler in the optimiser's place of K6's captured training step (dense_train.GraphedDenseTrainStep):
SGLD (Welling & Teh 2011) or SGHMC (Chen et al. 2014) over every parameter tensor in one launch (bnn_sgmcmc_step), constant
or cyclical (Zhang et al. 2020) step sizes from a device table, the noise from its own Philox stream.  The launch that
updates the weights also files them into a `WeightBank` when the table row says so: an epoch driven by epoch.EpochRunner
fills the bank with no host decision.  `WeightBank` is also where a deep ensemble (Lakshminarayanan et al. 2017) puts its
members (`push`).  Its forward runs one minibatch through M members in one launch per layer (bnn_bank_fwd) and feeds the same
summaries as every other posterior here (ops.mc_softmax_mean / mc_predictive / mc_score)."""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .capture import capture_on_side_stream, word32
from .engine import _first_minibatch
from .mcdropout import _math, _summary_args, flat_input, layers_of
from .ops import BnnHipError, Predictive
from .runtime import state


# ---------------------------------------------------------------------------------------------------- the schedule table
def learning_rates(lr: float, thin: int = 1, cycle_length: Optional[int] = None) -> np.ndarray:
    """fp64 step sizes of the table's rows: `thin` equal rows, or the cyclical cosine schedule lr / 2 (cos(pi j / L) + 1)
    over L = cycle_length rows."""
    if cycle_length is None:
        return np.full(int(thin), float(lr), dtype=np.float64)
    Lc = int(cycle_length)
    return float(lr) / 2.0 * (np.cos(np.pi * np.arange(Lc, dtype=np.float64) / Lc) + 1.0)


def collect_flags(thin: int = 1, cycle_length: Optional[int] = None, collect_fraction: float = 0.25) -> np.ndarray:
    """The rows whose step is filed into the bank.  Constant schedule: the last of the `thin` rows (every thin-th step).
    Cyclical: the last n = max(1, floor(collect_fraction L)) rows of the cycle, every thin-th counted back from the cycle's
    last row (the smallest step size is always taken)."""
    thin = int(thin)
    if cycle_length is None:
        f = np.zeros(thin, dtype=bool)
        f[-1] = True
        return f
    Lc = int(cycle_length)
    n = max(1, int(math.floor(float(collect_fraction) * Lc + 1e-9)))
    j = np.arange(Lc)
    return (j >= Lc - n) & ((Lc - 1 - j) % thin == 0)


def build_table(lr: float, *, temperature: float = 1.0, friction: Optional[float] = None, thin: int = 1,
                cycle_length: Optional[int] = None, collect_fraction: float = 0.25) -> np.ndarray:
    """float32 [L, 4] rows (a, b, c, collect flag) of bnn_sgmcmc_step, formed in fp64 and rounded once.  SGLD (friction
    None): a = lr_j / 2, b = 0, c = sqrt(lr_j T); SGHMC: a = lr_j, b = 1 - friction, c = sqrt(2 friction lr_j T)."""
    if int(thin) < 1 or (cycle_length is not None and int(cycle_length) < 1):
        raise ValueError("thin and cycle_length must be >= 1")
    if not 0.0 < float(collect_fraction) <= 1.0:
        raise ValueError(f"collect_fraction must lie in (0, 1], got {collect_fraction}")
    if friction is not None and not 0.0 < float(friction) <= 1.0:
        raise ValueError(f"friction must lie in (0, 1], got {friction}")
    lrs = learning_rates(lr, thin, cycle_length)
    T = float(temperature)
    t = np.zeros((len(lrs), L.SGMCMC_TABLE_COLS), dtype=np.float64)
    if friction is None:
        t[:, 0], t[:, 1], t[:, 2] = lrs / 2.0, 0.0, np.sqrt(lrs * T)
    else:
        al = float(friction)
        t[:, 0], t[:, 1], t[:, 2] = lrs, 1.0 - al, np.sqrt(2.0 * al * lrs * T)
    t[:, 3] = collect_flags(thin, cycle_length, collect_fraction)
    return t.astype(np.float32)


def _word(value: int, device) -> torch.Tensor:
    """A uint32 device word held as int32[1] (the kernels read it unsigned)."""
    return torch.tensor([word32(value)], dtype=torch.int32, device=device)


def _read_word(w: torch.Tensor) -> int:
    return int(w.item()) & 0xFFFFFFFF


def _set_word(w: torch.Tensor, value: int):
    w.fill_(word32(value))


# ---------------------------------------------------------------------------------------------------- the bank
class WeightBank:
    """`capacity` weight sets of `mlp` (MLP; an MLP_Dropout's members are run with the dropout off) in one float32 device
    buffer [capacity, stride]: element i of parameter tensor t (layer order: weight, bias) of member m at
    buffer[m, offsets[t] + i], every tensor starting at a multiple of 64 elements.  `collected` counts the members ever
    filed (the ring's next slot is collected % capacity), `step` is the chain's step word when a FusedSGMCMC fills it."""

    def __init__(self, mlp, capacity: int):
        self.mlp, self.capacity = mlp, int(capacity)
        if self.capacity < 1:
            raise BnnHipError("WeightBank: capacity must be >= 1")
        self.layers = layers_of(mlp)
        self.params = [t for d in self.layers for t in (d.linear.weight, d.linear.bias) if t is not None]
        if len(self.params) > L.SGMCMC_MAX_TENSORS:
            raise BnnHipError(f"WeightBank: at most {L.SGMCMC_MAX_TENSORS} parameter tensors")
        self.shapes = [tuple(p.shape) for p in self.params]
        self.numels = [p.numel() for p in self.params]
        self.offsets, self.stride = ops.bank_layout(self.numels)
        off = dict(zip(map(id, self.params), self.offsets))
        self._w_off = [off[id(d.linear.weight)] for d in self.layers]
        self._b_off = [None if d.linear.bias is None else off[id(d.linear.bias)] for d in self.layers]
        dev = self.params[0].device
        self.device = dev
        self.buffer = torch.zeros((self.capacity, self.stride), dtype=torch.float32, device=dev)
        self.collected = _word(0, dev)
        self.step = _word(0, dev)

    # ---- members
    def views(self, m: int) -> List[torch.Tensor]:
        """Slot m's tensors, shaped like the parameters (views of the buffer)."""
        m = int(m)
        if not 0 <= m < self.capacity:
            raise BnnHipError(f"WeightBank: slot {m} outside [0, {self.capacity})")
        return [self.buffer[m, o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]

    def _params_of(self, mlp):
        ps = [t for d in layers_of(mlp) for t in (d.linear.weight, d.linear.bias) if t is not None]
        if [tuple(p.shape) for p in ps] != self.shapes:
            raise BnnHipError("WeightBank: the network's parameter shapes are not the bank's")
        return ps

    def count(self) -> int:
        """Members held: min(collected, capacity).  One device read."""
        return min(_read_word(self.collected), self.capacity)

    def push(self, mlp=None) -> int:
        """Copy the network's current weights into the ring's next slot and advance `collected`; returns the slot."""
        ps = self._params_of(self.mlp if mlp is None else mlp)
        c = _read_word(self.collected)
        m = c % self.capacity
        with torch.no_grad():
            for v, p in zip(self.views(m), ps):
                v.copy_(p.detach())
        _set_word(self.collected, c + 1)
        return m

    def member(self, m: int, into=None):
        """Copy slot m into a network (`into`, by default the bank's own); returns the network."""
        net = self.mlp if into is None else into
        with torch.no_grad():
            for v, p in zip(self.views(m), self._params_of(net)):
                p.copy_(v)
        return net

    def state_dict(self) -> dict:
        return dict(buffer=self.buffer.detach().clone(), collected=_read_word(self.collected), step=_read_word(self.step),
                    capacity=self.capacity, shapes=[list(s) for s in self.shapes])

    def load_state_dict(self, sd: dict):
        """In place: the buffer and the words keep their addresses (a captured step or predictive holds them)."""
        if int(sd["capacity"]) != self.capacity or [tuple(s) for s in sd["shapes"]] != self.shapes:
            raise BnnHipError("WeightBank.load_state_dict: another capacity or other parameter shapes")
        self.buffer.copy_(sd["buffer"])
        _set_word(self.collected, int(sd["collected"]))
        _set_word(self.step, int(sd["step"]))

    # ---- forward
    def _span(self, members, first):
        first = int(first)
        M = self.count() - first if members is None else int(members)
        if M < 1 or first < 0 or first + M > self.capacity:
            raise BnnHipError(f"WeightBank: members [{first}, {first + M}) -- the bank holds none there")
        return M, first

    def _chain(self, xf: torch.Tensor, M: int, first: int, bufs=None) -> torch.Tensor:
        math_mode, hidden = _math()
        h, last = xf, len(self.layers) - 1
        for i, d in enumerate(self.layers):
            h = ops.bank_fwd(h, self.buffer, self._w_off[i], self._b_off[i], out_features=d.linear.out_features, members=M,
                             first=first, relu=d.relu, math_mode=math_mode, y_dtype=torch.float32 if i == last else hidden,
                             out=None if bufs is None else bufs[i])
        return h

    def forward(self, x: torch.Tensor, members: Optional[int] = None, first: int = 0) -> torch.Tensor:
        """[M, B, out] fp32: the minibatch through members first .. first + M - 1 (by default all count() of them), one
        bnn_bank_fwd per layer -- x shared into layer 1, per-member activations (bf16 in bf16 math) after."""
        M, first = self._span(members, first)
        with torch.no_grad():
            return self._chain(flat_input(self.mlp, x), M, first)

    __call__ = forward

    # ---- summaries (the unchanged F3 / F12 launches)
    def predict_mc(self, x: torch.Tensor):
        """(preds [B], probs [B, C]): probs the mean softmax over the members."""
        logits = self.forward(x)
        probs, preds = ops.mc_softmax_mean(logits, 1.0 / logits.shape[0])
        return preds, probs

    def predictive(self, x: torch.Tensor, quantiles=None, sigma: float = 1.0) -> Predictive:
        q = _summary_args(self.mlp.mode, quantiles)
        return _first_minibatch(ops.mc_predictive(self.forward(x), self.mlp.mode, sigma=float(sigma), quantiles=q))

    def score(self, x: torch.Tensor, y: torch.Tensor, sigma: float = 1.0, bins: int = 10, record=None,
              n_valid: Optional[int] = None) -> "ops.Scores":
        if self.mlp.mode not in ("classification", "regression"):
            raise Exception("Training mode must be either 'regression' or 'classification'")
        return ops.mc_score(self.forward(x), y, self.mlp.mode, sigma=float(sigma), bins=int(bins), record=record, n_valid=n_valid)

    def rows_per_launch(self, M: int, n_rows: int, budget_bytes: int = 1 << 28) -> int:
        """Rows of an evaluation launch: the launch streams the whole bank whatever its rows, so as many as `budget_bytes`
        of the widest layer's [M, rows, width] activations allow (a multiple of 64, at most n_rows)."""
        width = max(d.linear.out_features for d in self.layers)
        per_row = M * width * (2 if _math()[1] == torch.bfloat16 else 4)
        r = max(64, budget_bytes // per_row // 64 * 64)
        return int(min(r, n_rows))

    def evaluate(self, loader, *, sigma: float = 1.0, bins: int = 10, rows: Optional[int] = None) -> "ops.Scores":
        """The held-out scores (ops.Scores; `.read()` is the one copy) of the ensemble over every row the loader covers
        (a DeviceLoader or EvalLoader, walked in identity order; drop_last leaves the rows behind the last full minibatch
        out, as epoch.score does).  `rows` per launch: by default rows_per_launch -- the bank is read once per launch, not
        once per minibatch."""
        from .epoch import fill_rows
        ds, B = loader.dataset, int(loader.batch_size)
        ops.require_device(ds.x)
        N, d = ds.x.shape
        total = (N // B) * B if loader.drop_last else N
        M, first = self._span(None, 0)
        R = self.rows_per_launch(M, total) if rows is None else max(1, min(int(rows), total))
        cls = self.mlp.mode == "classification"
        scores = ops.Scores(self.mlp.mode, bins, ds.device)
        xb = torch.empty((R, d), dtype=torch.float32, device=ds.device)
        yb = torch.zeros((R,) if cls else (R, ds.y.shape[1]), dtype=ds.y.dtype, device=ds.device)
        with torch.no_grad():
            for a in range(0, total, R):
                b = min(total, a + R)
                fill_rows(ds, xb, a, b)
                yb[:b - a].copy_(ds.y[a:b])
                ops.mc_score(self._chain(xb, M, first), yb, self.mlp.mode, sigma=float(sigma), bins=int(bins), record=scores,
                             n_valid=b - a)
        return scores

    def predictive_graph(self, x: torch.Tensor, quantiles=None, sigma: float = 1.0, capture: bool = True):
        return GraphedBankPredictive(self, x, quantiles=quantiles, sigma=sigma, capture=capture)


class GraphedBankPredictive:
    """WeightBank.predictive for one input shape and the members the bank held when it was built, as a replayable
    evaluation: static input `.x` ([B, in], the flattened input), static outputs, one launch per layer plus the summary
    launch on one stream -- a linear chain, captured once as a hipGraph (`capture=False`: launched eagerly on every
    replay).  The launches read the bank's buffer in place: members overwritten since are seen by the next replay."""

    def __init__(self, bank: WeightBank, x: torch.Tensor, quantiles=None, sigma: float = 1.0, capture: bool = True):
        self.bank, self.sigma, self.mode = bank, float(sigma), bank.mlp.mode
        self.q = _summary_args(self.mode, quantiles)
        self.members, self.first = bank._span(None, 0)
        self.x = flat_input(bank.mlp, x).clone().contiguous()
        dev, B, M = self.x.device, self.x.shape[0], self.members
        _, hidden = _math()
        last = len(bank.layers) - 1
        self.bufs = [torch.empty((M, B, d.linear.out_features), dtype=torch.float32 if i == last else hidden, device=dev)
                     for i, d in enumerate(bank.layers)]
        self._pred = ops.predictive_buffers(self.mode, 1, B, bank.layers[-1].linear.out_features, dev, self.q)
        self.result = _first_minibatch(self._pred)
        self.graph = None
        if capture:
            with torch.no_grad():
                self._enqueue()                  # warm-up (also validates the arguments eagerly)
            torch.cuda.synchronize()
            with torch.no_grad():
                self.graph = capture_on_side_stream(self._enqueue)

    def _enqueue(self):
        logits = self.bank._chain(self.x, self.members, self.first, bufs=self.bufs)
        ops.mc_predictive(logits, self.mode, sigma=self.sigma, quantiles=self.q, out=self._pred)

    def replay(self) -> Predictive:
        if self.graph is not None:
            self.graph.replay()
        else:
            with torch.no_grad():
                self._enqueue()
        return self.result

    @property
    def logits(self) -> torch.Tensor:
        return self.bufs[-1]


# ---------------------------------------------------------------------------------------------------- the sampler
# _dev[gi]: the entries a captured step holds the address of (capture.snapshot saves and restores them around a warm-up)
_STEP, _COLLECTED, _TICKET, _TABLE, _LR = range(5)


class FusedSGMCMC(torch.optim.Optimizer):
    """SGLD (`friction=None`) or SGHMC (`friction=alpha`, a momentum buffer in state[p]['momentum']) on the posterior of an
    MLP's weights under a N(0, 1 / prior_precision) prior, every parameter tensor in one launch (bnn_sgmcmc_step):

        g = (dataset_size / batch_size) grad + prior_precision p,   grad of the SUM loss over the minibatch (K6's losses)
        SGLD:  p += -lr / 2 g + sqrt(lr T) eps          SGHMC:  v = (1 - alpha) v - lr g + sqrt(2 alpha lr T) eps,  p += v

    `cycle_length=L`: the cyclical cosine schedule lr_j = lr / 2 (cos(pi j / L) + 1), j = step % L.  With a `bank` the
    launch also files the weights into it after burn_in steps: every `thin`-th step, or with a cycle every thin-th step of
    the last `collect_fraction` of each cycle (collect_flags).  The step word, the collected count, the ticket and the
    schedule table live on the device (`_dev[gi]`), so a captured training step (dense_train.GraphedDenseTrainStep) samples
    and collects by itself; `param_groups[i]['lr']` stays the knob (sync_lr).  `seed`: the noise stream's key
    (runtime.state.seed by default)."""

    def __init__(self, params, lr=1e-3, *, dataset_size, batch_size, prior_precision=1.0, temperature=1.0, friction=None,
                 burn_in=0, thin=1, cycle_length=None, collect_fraction=0.25, seed=None, bank: Optional[WeightBank] = None,
                 capturable=True):
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if int(dataset_size) < 1 or int(batch_size) < 1:
            raise ValueError("dataset_size and batch_size must be >= 1")
        if not 0.0 <= prior_precision or not 0.0 <= temperature or int(burn_in) < 0:
            raise ValueError("prior_precision, temperature and burn_in must be >= 0")
        build_table(lr, temperature=temperature, friction=friction, thin=thin, cycle_length=cycle_length,
                    collect_fraction=collect_fraction)                       # (validates the schedule's arguments)
        super().__init__(params, dict(lr=lr, prior_precision=float(prior_precision), temperature=float(temperature),
                                      friction=None if friction is None else float(friction), thin=int(thin),
                                      cycle_length=None if cycle_length is None else int(cycle_length),
                                      collect_fraction=float(collect_fraction), capturable=capturable))
        self.grad_scale = float(dataset_size) / float(batch_size)
        self.burn_in = int(burn_in)
        self.seed = (state.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.bank = bank
        if bank is not None:
            if len(self.param_groups) != 1:
                raise BnnHipError("FusedSGMCMC: a bank needs all parameters in one group")
            self._check_bank(self.param_groups[0]["params"])
        self._dev = {}
        for gi, group in enumerate(self.param_groups):
            dev = group["params"][0].device
            if dev.type == "cuda":
                self._group_dev(gi, group, dev)

    def _check_bank(self, ps):
        if [tuple(p.shape) for p in ps] != self.bank.shapes:
            raise BnnHipError("FusedSGMCMC: the bank was built for a network of other parameter shapes")

    def _table(self, group) -> np.ndarray:
        return build_table(group["lr"], temperature=group["temperature"], friction=group["friction"], thin=group["thin"],
                           cycle_length=group["cycle_length"], collect_fraction=group["collect_fraction"])

    def _group_dev(self, gi, group, device):
        if gi not in self._dev:
            steps = [int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]]
            bank = self.bank
            if bank is not None and bank.device != device:
                raise BnnHipError("FusedSGMCMC: the bank lives on another device than the parameters")
            step = bank.step if bank is not None else _word(max(steps) if steps else 0, device)
            collected = bank.collected if bank is not None else _word(0, device)
            self._dev[gi] = [step, collected, torch.zeros(16, dtype=torch.int32, device=device),
                             torch.from_numpy(self._table(group)).to(device), group["lr"]]
            if bank is not None:
                # the warm-up step of a captured training step may file its weights over the ring's oldest member: the
                # buffer is among what that warm-up saves and restores (one bank-sized copy when a step is built)
                self._dev[gi].append(bank.buffer)
        return self._dev[gi]

    def sync_lr(self):
        """Rebuild the device table in place where param_groups[i]['lr'] changed (an lr scheduler).  Call outside capture,
        before replaying."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev and self._dev[gi][_LR] != group["lr"]:
                self._dev[gi][_TABLE].copy_(torch.from_numpy(self._table(group)))
                self._dev[gi][_LR] = group["lr"]

    def device_step(self, gi: int = 0) -> int:
        return _read_word(self._dev[gi][_STEP]) if gi in self._dev else 0

    def state_dict(self):
        """torch's format; the device step word is mirrored into state[p]['step'] first (one device read per group)."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev:
                step = self.device_step(gi)
                for p in group["params"]:
                    self.state[p]["step"] = step
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """torch's format.  Everything a captured training step holds the address of survives the load: the momentum
        tensors, the device words and the table are updated in place (as FusedAdam.load_state_dict)."""
        keep = {p: self.state[p]["momentum"] for g in self.param_groups for p in g["params"]
                if p in self.state and "momentum" in self.state[p]}
        super().load_state_dict(state_dict)
        for p, m in keep.items():
            st = self.state.get(p)
            if st and "momentum" in st and st["momentum"] is not m:
                m.copy_(st["momentum"])
                st["momentum"] = m
        for gi, group in enumerate(self.param_groups):
            if gi not in self._dev:
                continue
            steps = [int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]]
            d = self._dev[gi]
            _set_word(d[_STEP], max(steps) if steps else 0)
            d[_TICKET].zero_()
            d[_TABLE].copy_(torch.from_numpy(self._table(group)))
            d[_LR] = group["lr"]

    @torch.no_grad()
    def step(self, closure=None, noise=None, eps_mode: int = L.EPS_PHILOX):
        """`noise` (a dict parameter -> tensor) with eps_mode=EPS_MEMORY, or eps_mode=EPS_ZERO: the update on given noise
        (tests; gradient descent on the log posterior)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            gs = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in ps]
            if any(g.is_sparse for g in gs):
                raise RuntimeError("FusedSGMCMC does not support sparse gradients")
            ms = None
            if group["friction"] is not None:
                ms = []
                for p in ps:
                    st = self.state[p]
                    if "momentum" not in st:
                        st["momentum"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    ms.append(st["momentum"])
            bank = self.bank
            if bank is not None:
                if len(ps) != len(group["params"]):
                    raise BnnHipError("FusedSGMCMC: with a bank every parameter needs a gradient")
                self._check_bank(ps)
            d = self._group_dev(gi, group, ps[0].device)
            if not torch.cuda.is_current_stream_capturing():
                self.sync_lr()
            ops.sgmcmc_step(ps, gs, table=d[_TABLE], step=d[_STEP], ticket=d[_TICKET], grad_scale=self.grad_scale,
                            tau=group["prior_precision"], eps_mode=eps_mode, seed=self.seed, momenta=ms,
                            noise=None if noise is None else [noise[p] for p in ps], burn_in=self.burn_in,
                            collected=d[_COLLECTED], bank=None if bank is None else bank.buffer)
        return loss
