"""F3 / F4 host side: the reference's post-hoc analyses on device tensors.

`ECELoss` mirrors compute_ece.py:14-57 (same constructor, same return triple) and `compute_snr` /
`prune_weights` mirror weight_pruning.py:85-115 (same names and argument meaning), so the reference's scripts can
call them with the tensors they already hold; the per-element work runs in bnn_ece / bnn_snr_db / bnn_snr_prune.
Neither reference module can be imported in the build container (both need seaborn at import), so these two rows
have no reference-recorded vectors: the oracle restates them from the source text (parity UNPINNED).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class ECELoss(torch.nn.Module):
    """compute expected calibration error (compute_ece.py:14-57).  forward(probs [n, classes], labels [n]) with
    device tensors returns (ece float, bin_centers[have_data] ndarray, bin_acc ndarray) like the reference."""

    def __init__(self, bin_step=0.1, num_classes=10):
        super().__init__()
        self.bin_step = bin_step
        self.num_classes = num_classes

    def forward(self, probs, labels):
        bins = np.arange(0, 1.1, self.bin_step)                      # compute_ece.py:32, verbatim: the same float64 edges
        if not torch.is_tensor(probs):
            probs = torch.as_tensor(np.asarray(probs, np.float32))
            labels = torch.as_tensor(np.asarray(labels, np.int64))
            dev = torch.device("cuda", torch.cuda.current_device())
            probs, labels = probs.to(dev), labels.to(dev)
        out = ops.ece_bins(probs, labels, bins).double().cpu().numpy()
        stats = out[1:].reshape(-1, 3)
        counts, corrects = stats[:, 0], stats[:, 1]
        bin_centers = bins[1:] - self.bin_step / 2                   # :36
        have_data = counts > 0                                       # :50
        bin_acc = corrects[have_data] / counts[have_data]            # :51
        return float(out[0]), bin_centers[have_data], bin_acc

    def bins(self, probs, labels):
        """(counts, corrects, mean confidence) per bin -- what the reliability diagram plots."""
        bins = np.arange(0, 1.1, self.bin_step)
        st = ops.ece_bins(probs, labels, bins).double().cpu().numpy()[1:].reshape(-1, 3)
        with np.errstate(invalid="ignore", divide="ignore"):
            return st[:, 0], st[:, 1], st[:, 2] / st[:, 0]


def _bayesian_layers(model):
    return [l for l in model.children() if hasattr(l, "weight_mu") and hasattr(l, "weight_rho")]


def collect_weights(model, bnn=False, sample=None):
    """weight_pruning.py:16-38 on the device: the parameters whose names hold neither 'mu' nor 'rho', flattened and
    concatenated in named_parameters() order; with bnn=True `[mus, sigmas]` (sigma = log1p(exp(rho)), rho_to_sigma :40-41);
    with `sample` set (a global MC sample index) ONE draw per posterior instead, mu + sigma * eps on the network's seed and
    epsilon tensor ids -- the vector sample_bnn_weights (:43-44) makes.  Flat fp32 device tensors; the sigmas and the draws
    come out of bnn_param_hist's values_out, nothing goes through Python lists."""
    from . import _lib as L
    mus, rhos, weights = [], [], []
    for name, p in model.named_parameters():
        (mus if "mu" in name else rhos if "rho" in name else weights).append(p.detach())
    if not bnn:
        return torch.cat([w.flatten() for w in weights]) if weights else torch.empty(0)
    if not mus or len(mus) != len(rhos):
        raise ops.BnnHipError("collect_weights: bnn=True needs (mu, rho) parameter pairs")
    ops.require_device(*mus, *rhos)
    sizes = [r.numel() for r in rhos]
    out = torch.empty(sum(sizes), dtype=torch.float32, device=rhos[0].device)
    outs = list(torch.split(out, sizes))
    if sample is None:
        jobs = [dict(kind=L.HIST_SIGMA, src0=r, values_out=o) for r, o in zip(rhos, outs)]
    else:
        from .runtime import state
        ids = [4 * int(getattr(l, "_layer_id", i)) + k for i, l in enumerate(_bayesian_layers(model)) for k in (0, 1)]
        if len(ids) != len(mus):
            raise ops.BnnHipError("collect_weights: sample needs Bayesian layers of one weight and one bias posterior each")
        jobs = [dict(kind=L.HIST_SAMPLE, src0=m, src1=r, values_out=o, seed=state.seed, tensor_id=t, sample=int(sample))
                for m, r, o, t in zip(mus, rhos, outs, ids)]
    for i in range(0, len(jobs), L.HIST_MAX_JOBS):
        ops.param_hist(ops.param_hist_args(jobs[i:i + L.HIST_MAX_JOBS], (-1.0, 1.0)))
    return out if sample is not None else [torch.cat([m.flatten() for m in mus]), out]


def compute_snr(model_or_mu, sigma=None):
    """weight_pruning.py:85-87.  compute_snr(mu, sigma) with numpy / python inputs keeps the reference's numpy
    arithmetic; compute_snr(model) returns the SNR (dB, fp32 device tensor) of every stochastic parameter of the
    model in named_parameters() order of the (mu, rho) pairs -- the vector the reference builds through
    collect_weights (weight_pruning.py:15-40) -- in one device pass per tensor."""
    if sigma is not None:
        return 10 * np.log10(abs(model_or_mu) / sigma)
    parts = []
    for l in _bayesian_layers(model_or_mu):
        parts.append(ops.snr_db(l.weight_mu.detach(), l.weight_rho.detach()).flatten())
        parts.append(ops.snr_db(l.bias_mu.detach(), l.bias_rho.detach()).flatten())
    return torch.cat(parts)


def snr_threshold(snrs, drop_percentage: float) -> float:
    """np.percentile(snrs, 100 * drop_percentage) (weight_pruning.py:92: linear interpolation between order
    statistics), from a device sort when `snrs` is a device tensor."""
    if not torch.is_tensor(snrs):
        return float(np.percentile(snrs, 100 * drop_percentage))
    v, _ = torch.sort(snrs.flatten())
    pos = (v.numel() - 1) * float(drop_percentage)
    lo = int(np.floor(pos))
    hi = min(lo + 1, v.numel() - 1)
    a, b = float(v[lo]), float(v[hi])
    if a == b:                                                      # also covers (-inf, -inf): no inf - inf
        return a
    return a + (b - a) * (pos - lo)


def prune_weights(model, snrs=None, drop_percentage=0.5):
    """Remove weights with the lowest SNR (weight_pruning.py:89-115): in place, mu *= mask and rho *= mask with
    mask = snr > threshold, for the weights and biases of every Bayesian layer.  `snrs` None: computed here."""
    if snrs is None:
        snrs = compute_snr(model)
    thr = snr_threshold(snrs, drop_percentage)
    with torch.no_grad():
        for l in _bayesian_layers(model):
            for mu, rho in ((l.weight_mu, l.weight_rho), (l.bias_mu, l.bias_rho)):
                if not (mu.data.is_contiguous() and rho.data.is_contiguous()):
                    mu.data, rho.data = mu.data.contiguous(), rho.data.contiguous()
                ops.snr_prune_(mu.data, rho.data, thr)
    return thr


# ---------------------------------------------------------------------------------------------------- F9 pruning sweep
def _snr_segments(model_or_snrs):
    """The fp32 SNR vector as a list of device segments: a tensor, a list of tensors, or a model (one segment per
    (mu, rho) tensor, in compute_snr's order -- never concatenated)."""
    if torch.is_tensor(model_or_snrs):
        return [model_or_snrs.flatten()]
    if isinstance(model_or_snrs, (list, tuple)):
        return [s.flatten() for s in model_or_snrs]
    segs = []
    for l in _bayesian_layers(model_or_snrs):
        segs.append(ops.snr_db(l.weight_mu.detach(), l.weight_rho.detach()).flatten())
        segs.append(ops.snr_db(l.bias_mu.detach(), l.bias_rho.detach()).flatten())
    return segs


def snr_thresholds(model_or_snrs, drop_percentages):
    """[snr_threshold(snrs, p) for p in drop_percentages] as a float64 device tensor, by selection (bnn_snr_select): no
    sort, no concatenation, no host read.  `model_or_snrs`: a model, an fp32 SNR device tensor or a list of them."""
    return ops.snr_select(_snr_segments(model_or_snrs), drop_percentages)


def _round_up(v, m):
    return -(-int(v) // m) * m


class PruneSweepResult:
    """What PruneSweep.evaluate leaves on the device; every host-side field is read (one synchronising copy) on access.
    Per level, in the caller's order: correct (device int64), accuracy, nll (the summed cross-entropy), ece, bins
    ((counts, corrects, mean confidence) as ECELoss.bins), reliability ((centers, accuracy, counts) of the bins that hold
    data, as ECELoss.forward's diagram), thresholds, kept; probs [P, N, classes] and labels [N] stay on the device.
    Regression: sse (the summed squared error) instead of correct / nll / ece / probs."""

    def __init__(self, mode, total, correct, loss, ece_out, probs, labels, thresholds, kept, bin_step):
        self.mode, self.total, self.correct, self._loss, self._ece_out = mode, int(total), correct, loss, ece_out
        self.probs, self.labels, self.thresholds, self.kept, self.bin_step = probs, labels, thresholds, kept, bin_step

    @property
    def accuracy(self):
        return None if self.correct is None else self.correct.cpu().numpy() / float(self.total)

    @property
    def nll(self):
        return None if self.mode != "classification" else self._loss.cpu().numpy()

    @property
    def sse(self):
        return None if self.mode == "classification" else self._loss.cpu().numpy()

    def _stats(self):
        return None if self._ece_out is None else self._ece_out.double().cpu().numpy()

    @property
    def ece(self):
        st = self._stats()
        return None if st is None else st[:, 0].copy()

    @property
    def bins(self):
        st = self._stats()
        if st is None:
            return None
        out = []
        for row in st:
            b = row[1:].reshape(-1, 3)
            with np.errstate(invalid="ignore", divide="ignore"):
                out.append((b[:, 0], b[:, 1], b[:, 2] / b[:, 0]))
        return out

    @property
    def reliability(self):
        st = self._stats()
        if st is None:
            return None
        centers = np.arange(0, 1.1, self.bin_step)[1:] - self.bin_step / 2
        out = []
        for row in st:
            b = row[1:].reshape(-1, 3)
            have = b[:, 0] > 0
            out.append((centers[have], b[have, 1] / b[have, 0], b[have, 0]))
        return out


class PruneSweep:
    """weight_pruning.py's table -- the network pruned at each of `drop_percentages`, evaluated -- without pruning or
    copying anything: the thresholds of all levels by one selection (bnn_snr_select), one byte of level code and one
    matmul-ready mu per parameter (bnn_prune_codes), then every forward runs all levels together (bnn_pruned_fwd).
    `net`: a BayesianNetwork of either layer type; it is read at construction (a snapshot of mu and rho, in the math mode
    set then) and never written.  Levels may come in any order; every per-level result is in the caller's order."""

    def __init__(self, net, drop_percentages=(0., .5, .75, .95, .98)):
        from . import _lib as L
        from .runtime import state
        ps = [float(p) for p in drop_percentages]
        if not 1 <= len(ps) <= L.PRUNE_MAX_LEVELS or any(not 0.0 <= p <= 1.0 for p in ps):
            raise ops.BnnHipError(f"PruneSweep: 1 to {L.PRUNE_MAX_LEVELS} drop fractions in [0, 1]")
        layers = _bayesian_layers(net)
        if len(layers) != 3 or not hasattr(net, "local_reparam"):
            raise ops.BnnHipError("PruneSweep: a BayesianNetwork (three Bayesian layers)")
        self.net, self.drop_percentages, self.levels = net, tuple(ps), len(ps)
        self.mode = net.mode
        self.math = L.MATH_BF16 if state.math == L.MATH_BF16 else L.MATH_F32
        order = sorted(range(len(ps)), key=lambda i: ps[i])              # ascending fractions = ascending thresholds
        pos = [0] * len(ps)
        for j, i in enumerate(order):
            pos[i] = j
        dev = layers[0].weight_mu.device
        ops.require_device(layers[0].weight_mu)
        self._pos = None if pos == list(range(len(ps))) else torch.tensor(pos, dtype=torch.int64, device=dev)
        self.level_rank = tuple(pos)                                    # caller's level i is the level_rank[i]-th threshold
        lr = bool(net.local_reparam)
        P = self.levels
        with torch.no_grad():
            thr = ops.snr_select(_snr_segments(net), [ps[i] for i in order])
            kept = torch.zeros(P, dtype=torch.int64, device=dev)
            wdt = torch.bfloat16 if self.math == L.MATH_BF16 else torch.float32
            self._layers = []
            self.total_parameters = 0
            for l in layers:
                fin, fout = (l.weight_mu.shape if lr else l.weight_mu.shape[::-1])
                fin, fout = int(fin), int(fout)
                shape = (_round_up(fout, 64), _round_up(fin, 32))
                code = torch.zeros(shape, dtype=torch.uint8, device=dev)
                mu = torch.zeros(shape, dtype=wdt, device=dev)
                ops.prune_codes(l.weight_mu.detach(), l.weight_rho.detach(), thr, code, mu, kept, out_features=fout,
                                in_features=fin, transposed=lr)
                bcode = torch.zeros((1, _round_up(fout, 32)), dtype=torch.uint8, device=dev)
                b = torch.zeros((1, _round_up(fout, 32)), dtype=torch.float32, device=dev)
                ops.prune_codes(l.bias_mu.detach(), l.bias_rho.detach(), thr, bcode, b, kept, out_features=1,
                                in_features=fout, transposed=False)
                self._layers.append((fin, fout, mu, code, b, bcode))
                self.total_parameters += l.weight_mu.numel() + l.bias_mu.numel()
        self._thr_sorted = thr
        self.thresholds = self._caller_order(thr)
        self.kept = self._caller_order(kept)
        self._plans = {}

    def _caller_order(self, t):
        return t if self._pos is None else t[self._pos]

    def codes(self):
        """[(weight codes uint8 [out, in], bias codes uint8 [out])] per layer, views of the canonical images: the parameter
        survives the caller's level i exactly when its code > level_rank[i]."""
        return [(code[:fout, :fin], bcode[0, :fout]) for fin, fout, _, code, _, bcode in self._layers]

    def _plan(self, rows, dev):
        """The static buffers and argument blocks of a forward over `rows` rows (hidden activations padded to a multiple
        of 32 columns, zero there for good: the next layer's vector loads need no tail)."""
        from . import _lib as L
        pl = self._plans.get(rows)
        if pl is None:
            P, bf = self.levels, self.math == L.MATH_BF16
            hdt = torch.bfloat16 if bf else torch.float32
            (i1, o1, *_), (i2, o2, *_), (i3, o3, *_) = self._layers
            x0 = torch.zeros((rows, i1), dtype=hdt, device=dev)
            h1 = torch.zeros((P, rows, _round_up(o1, 32)), dtype=hdt, device=dev)
            h2 = torch.zeros((P, rows, _round_up(o2, 32)), dtype=hdt, device=dev)
            logits = torch.zeros((P, rows, o3), dtype=torch.float32, device=dev)
            args = []
            for (fin, fout, mu, code, b, bcode), xin, yout, relu in zip(self._layers, (x0, h1, h2), (h1, h2, logits),
                                                                       (True, True, False)):
                args.append(ops.pruned_fwd_args(x=xin, mu=mu, code=code, b=b, bcode=bcode, y=yout, n_levels=P, rows=rows,
                                                in_features=fin, out_features=fout, math_mode=self.math, relu=relu,
                                                x_shared=xin is x0))
            pl = self._plans[rows] = (x0, logits, args, (h1, h2))
        return pl

    def _forward(self, x):
        """Logits [P, rows, classes] of all levels in ASCENDING-threshold order, in the plan's own buffer."""
        from . import _lib as L
        ops.require_device(x)
        x = x.reshape(-1, self._layers[0][0]) if self.mode == "classification" else x
        if x.dim() != 2 or x.shape[1] != self._layers[0][0] or x.dtype != torch.float32:
            raise ops.BnnHipError(f"PruneSweep: x must be float32 [rows, {self._layers[0][0]}]")
        x = x if x.is_contiguous() else x.contiguous()
        x0, logits, args, _ = self._plan(x.shape[0], x.device)
        if self.math == L.MATH_BF16:
            ops.cast_bf16(x, out=x0)
            args[0].x = x0.data_ptr()
        else:
            args[0].x = x.data_ptr()
        for a in args:
            ops.pruned_fwd(a)
        return logits

    def forward(self, x):
        """[P, rows, classes] float32: what net pruned at each level (prune_weights on a copy) returns in eval mode."""
        with torch.no_grad():
            y = self._forward(x)
            return y.clone() if self._pos is None else y[self._pos]

    __call__ = forward

    def evaluate(self, data, bin_step=0.1, batch_size=128):
        """The reference's evaluation of every pruned level over a data set: `data` a DeviceLoader (its minibatches, in its
        order) or a pair of device tensors (x [N, ...], y) walked in minibatches of `batch_size` (a short last one
        included).  Returns a PruneSweepResult; nothing is read back before one of its host fields is."""
        from . import _lib as L
        from .epoch import DeviceLoader
        cls = self.mode == "classification"
        P, C = self.levels, self._layers[2][1]
        if isinstance(data, DeviceLoader):
            N = len(data) * data.batch_size
            batches = iter(data)
            dev = data.dataset.device
        else:
            X, Y = data
            ops.require_device(X, Y)
            N, dev = int(X.shape[0]), X.device
            bs = int(batch_size)
            batches = ((X[i:i + bs], Y[i:i + bs]) for i in range(0, N, bs))
        loss = torch.zeros(P, dtype=torch.float64, device=dev)
        probs = correct = labels = ece_out = None
        if cls:
            probs = torch.empty((P, N, C), dtype=torch.float32, device=dev)
            correct = torch.zeros(P, dtype=torch.int64, device=dev)
            labels = torch.empty(N, dtype=torch.int64, device=dev)
        mode = L.NLL_CLASSIFICATION if cls else L.NLL_REGRESSION
        row0 = 0
        with torch.no_grad():
            for x, y in batches:
                logits = self._forward(x)
                rows = logits.shape[1]
                y = (y if cls else y.reshape(rows, C)).contiguous()
                if cls:
                    labels[row0:row0 + rows].copy_(y)
                ops.prune_sweep_tail(logits, y, mode=mode, probs=probs, correct=correct, loss=loss, row0=row0, n_total=N)
                row0 += rows
            if row0 != N:
                raise ops.BnnHipError(f"PruneSweep.evaluate: the data handed out {row0} rows, not {N}")
            if cls:
                edges = np.arange(0, 1.1, bin_step)
                ece_out = torch.stack([ops.ece_bins(probs[p], labels, edges) for p in range(P)])
                ece_out, probs, correct = self._caller_order(ece_out), self._caller_order(probs), self._caller_order(correct)
            loss = self._caller_order(loss)
        return PruneSweepResult(self.mode, N, correct, loss, ece_out, probs, labels, self.thresholds, self.kept, bin_step)
