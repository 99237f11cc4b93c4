"""F3 / F4 host side: the reference's post-hoc analyses on device tensors.

`ECELoss` mirrors compute_ece.py:14-57 (same constructor, same return triple) and `compute_snr` /
`prune_weights` mirror weight_pruning.py:85-115 (same names and argument meaning), so the reference's scripts can
call them with the tensors they already hold; the per-element work runs in bnn_ece / bnn_snr_db / bnn_snr_prune.
Parity pinned by tests/golden/posthoc.npz: what the real ECELoss, collect_weights, compute_snr and prune_weights
returned on seeded cases (oracle/make_golden_posthoc.py).  Two behaviours differ from the reference on purpose (DESIGN.md
section 2): a NaN in a device-side SNR list orders last (the reference's np.percentile turns NaN and everything is masked),
and a local_reparam network is pruned (the reference's isinstance(layer, BayesianLinear) leaves it unchanged).
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

    def compress(self, level_index, zero_signs=True):
        """The network pruned at the caller's level `level_index` of this sweep as a CompressedNetwork (CSR, run over the
        survivors only).  Reads the fp32 parameters of the sweep's network, which must not have changed since the sweep was
        built, and the three nnz words (the one host read)."""
        i = int(level_index)
        if not 0 <= i < self.levels:
            raise ops.BnnHipError(f"PruneSweep.compress: level_index must lie in [0, {self.levels})")
        images = [(fin, fout, code, bcode) for fin, fout, _, code, _, bcode in self._layers]
        return CompressedNetwork._build(_bayesian_layers(self.net), images, self.level_rank[i], bool(self.net.local_reparam),
                                        self.mode, zero_signs, self.drop_percentages[i], self.thresholds[i:i + 1])

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


# ---------------------------------------------------------------------------------------------------- F13 compressed network
_BIT_WEIGHTS = (1, 2, 4, 8, 16, 32, 64, 128)


def _pack_bits(flags):
    """bool [n] -> uint8 [ceil(n / 8)], bit i % 8 of byte i // 8."""
    f = flags.flatten().to(torch.uint8)
    f = torch.nn.functional.pad(f, (0, (-f.numel()) % 8)).view(-1, 8)
    w = torch.tensor(_BIT_WEIGHTS, dtype=torch.uint8, device=f.device)
    return (f * w).sum(1, dtype=torch.uint8)


def _unpack_bits(packed, n):
    w = torch.tensor(_BIT_WEIGHTS, dtype=torch.uint8, device=packed.device)
    return ((packed[:, None] & w) != 0).flatten()[:n]


def compressed_state_bytes(shapes, nnzs, zero_signs=True):
    """The bytes CompressedNetwork.state_dict holds for layers of `shapes` [(in, out)] with `nnzs` surviving weights:
    per layer 4 (out + 1) of row_ptr + nnz (2 + 4 + 4) of col, mu_val, rho_val + 2 * 4 out of the masked bias vectors
    + (zero_signs) 2 ceil(in out / 8) of the sign bits of mu and rho."""
    total = 0
    for (fin, fout), nnz in zip(shapes, nnzs):
        total += 4 * (fout + 1) + 10 * int(nnz) + 8 * fout
        if zero_signs:
            total += 2 * (-(-(fin * fout) // 8))
    return total


class _CsrLayer:
    __slots__ = ("fin", "fout", "nnz", "layer_id", "row_ptr", "col", "mu_val", "rho_val", "sigma_val", "b_mu", "b_rho", "b_sigma",
                 "mu_sign", "rho_sign")


class CompressedNetwork:
    """A BayesianNetwork pruned at one SNR level, kept as CSR and run over the surviving weights only (bnn_sparse_count,
    bnn_sparse_fill, bnn_sparse_fwd): per layer row_ptr (int32 [out + 1]), col (uint16 bits in an int16 tensor), mu_val,
    rho_val and the derived sigma_val = bnn_softplus(rho_val), the bias vectors multiplied by their mask, the mode and the
    layer ids.  Build one with PruneSweep.compress(level_index) or posthoc.compress(net, drop_percentage).

    The posterior this object samples: a surviving weight is N(mu, softplus(rho)^2) and draws the epsilon the dense
    network draws for it (the weight-space Philox map on the canonical [out, in] indices, also for a local-reparameterisation
    network: a draw from the same factorised posterior, not its activation-space draw); a pruned weight is EXACTLY zero in
    every sample.  That is not what sampling a prune_weights copy gives: there a pruned weight has mu = rho = 0, i.e.
    sigma = softplus(0) = ln 2.

    Arithmetic: exact fp32, one ascending fmaf chain per output element, whatever the math mode set -- the result depends on
    no tiling, on no cut of a batch into calls and not on the number of samples.

    Host reads: construction reads the three nnz words back ONCE, to size the arrays; that is the only one.  forward /
    forward_mc allocate their buffers at the first call for a (rows, samples) shape and then neither allocate nor read
    anything back, so they can be captured; they return their OWN static buffer, overwritten by the next call of that shape
    (clone it to keep it).  A captured forward_mc bakes x's address, the seed and sample_offset: pass a device
    `sample_counter` to draw fresh epsilon on every replay.

    `zero_signs` (default True) also keeps one bit per dense weight for each of mu and rho: the sign of the zero that
    prune_weights' `mu * 0` leaves, so that to_dense() equals prune_weights on a copy bit for bit; without them to_dense()
    writes +0 there (equal in value) and state_bytes shrinks by in * out / 4 bytes per layer."""

    def __init__(self, layers, mode, local_reparam, drop_percentage=None, threshold=None, prior=None):
        self._layers, self.mode, self.local_reparam = list(layers), mode, bool(local_reparam)
        self.drop_percentage, self.threshold = drop_percentage, threshold
        self.prior = prior                  # the source network's ops.PriorSpec (_build); None for an object built by hand
        self._plans = {}
        self._params = None

    # ------------------------------------------------------------------------------------------------ construction
    @classmethod
    def _build(cls, net_layers, images, rank, lr, mode, zero_signs, drop_percentage=None, threshold=None):
        """images: per layer (fin, fout, code [>= out, ld], bcode [1, >= out]) of a sweep; rank: the level's threshold rank."""
        with torch.no_grad():
            rps = []
            for (fin, fout, code, _bcode) in images:
                rp = torch.empty(fout + 1, dtype=torch.int32, device=code.device)
                rps.append(ops.sparse_count(code, rank, rp, out_features=fout, in_features=fin))
            nnzs = [int(v) for v in torch.stack([rp[-1] for rp in rps]).cpu().tolist()]      # the one host read
            out = []
            for l, (fin, fout, code, bcode), rp, nnz in zip(net_layers, images, rps, nnzs):
                dev = code.device
                c = _CsrLayer()
                c.fin, c.fout, c.nnz, c.layer_id, c.row_ptr = fin, fout, nnz, int(getattr(l, "_layer_id", len(out))), rp
                c.col = torch.zeros(max(nnz, 1), dtype=torch.int16, device=dev)              # (never an empty tensor: its address is NULL)
                c.mu_val = torch.zeros(max(nnz, 1), dtype=torch.float32, device=dev)
                c.rho_val = torch.zeros(max(nnz, 1), dtype=torch.float32, device=dev)
                wmu, wrho = l.weight_mu.detach(), l.weight_rho.detach()
                ops.sparse_fill(code, rank, rp, wmu, wrho, c.col, c.mu_val, c.rho_val, out_features=fout, in_features=fin,
                                transposed=lr)
                keep = bcode[0, :fout] > rank
                bmu, brho = l.bias_mu.detach(), l.bias_rho.detach()
                c.b_mu = torch.where(keep, bmu, bmu * 0.0).contiguous()                      # prune_weights' mu * 0: a signed zero
                c.b_rho = torch.where(keep, brho, brho * 0.0).contiguous()
                c.mu_sign = _pack_bits(torch.signbit(wmu)) if zero_signs else None           # (source layout, flattened)
                c.rho_sign = _pack_bits(torch.signbit(wrho)) if zero_signs else None
                cls._derive(c)
                out.append(c)
        return cls(out, mode, lr, drop_percentage, threshold, prior=getattr(net_layers[0], "_prior_spec", None))

    @staticmethod
    def _derive(c):
        """What is not state: sigma_val and the masked bias sigma, from the bits bnn_softplus gives."""
        c.sigma_val = ops.softplus(c.rho_val)
        keep = (c.b_mu != 0) | (c.b_rho != 0)                          # a kept bias has rho != 0 or mu != 0 (SNR > threshold needs mu != 0)
        c.b_sigma = torch.where(keep, ops.softplus(c.b_rho), torch.zeros_like(c.b_rho)).contiguous()

    # ------------------------------------------------------------------------------------------------ size
    @property
    def nnz(self):
        """Surviving weights per layer (biases not counted)."""
        return tuple(c.nnz for c in self._layers)

    @property
    def density(self):
        return sum(self.nnz) / float(sum(c.fin * c.fout for c in self._layers))

    @property
    def zero_signs(self):
        return self._layers[0].mu_sign is not None

    @property
    def state_bytes(self):
        """Bytes of state_dict(): compressed_state_bytes of the shapes and nnz."""
        return compressed_state_bytes([(c.fin, c.fout) for c in self._layers], self.nnz, self.zero_signs)

    # ------------------------------------------------------------------------------------------------ state
    def state_dict(self):
        sd = {}
        for i, c in enumerate(self._layers):
            p = f"l{i + 1}."
            sd[p + "row_ptr"], sd[p + "col"] = c.row_ptr, c.col[:c.nnz]
            sd[p + "mu_val"], sd[p + "rho_val"] = c.mu_val[:c.nnz], c.rho_val[:c.nnz]
            sd[p + "bias_mu"], sd[p + "bias_rho"] = c.b_mu, c.b_rho
            if c.mu_sign is not None:
                sd[p + "mu_sign"], sd[p + "rho_sign"] = c.mu_sign, c.rho_sign
        return sd

    def load_state_dict(self, sd):
        """Replace the CSR tensors by those of `sd` (a state_dict() of a network of the same shapes; device tensors);
        sigma_val is derived again.  Reads the nnz words of `sd` (their lengths: no device read)."""
        with torch.no_grad():
            for i, c in enumerate(self._layers):
                p = f"l{i + 1}."
                rp = sd[p + "row_ptr"]
                ops.require_device(rp)
                if rp.numel() != c.fout + 1 or sd[p + "bias_mu"].numel() != c.fout:
                    raise ops.BnnHipError("CompressedNetwork.load_state_dict: a layer of another shape")
                nnz = int(sd[p + "col"].numel())
                c.nnz, c.row_ptr = nnz, rp.to(torch.int32).contiguous().clone()
                for name, dt, dst in (("col", torch.int16, "col"), ("mu_val", torch.float32, "mu_val"), ("rho_val", torch.float32, "rho_val")):
                    buf = torch.zeros(max(nnz, 1), dtype=dt, device=rp.device)
                    buf[:nnz].copy_(sd[p + name])
                    setattr(c, dst, buf)
                c.b_mu, c.b_rho = sd[p + "bias_mu"].clone().contiguous(), sd[p + "bias_rho"].clone().contiguous()
                c.mu_sign = sd[p + "mu_sign"].clone() if p + "mu_sign" in sd else None
                c.rho_sign = sd[p + "rho_sign"].clone() if p + "rho_sign" in sd else None
                self._derive(c)
        self._plans = {}
        self._params = None
        return self

    # ------------------------------------------------------------------------------------------------ training (F14)
    def parameters(self):
        """The twelve nn.Parameters of the surviving posterior, in the order l1.weight_mu, l1.weight_rho, l1.bias_mu,
        l1.bias_rho, l2...: flat fp32 tensors sharing storage with mu_val[:nnz], rho_val[:nnz], b_mu, b_rho, so an optimiser
        step on them IS a step of this object (sigma_val / b_sigma are refreshed by the training step).  Created once and
        cached; load_state_dict drops the cache."""
        if self._params is None:
            self._params = [torch.nn.Parameter(t, requires_grad=True) for c in self._layers
                            for t in (c.mu_val[:c.nnz], c.rho_val[:c.nnz], c.b_mu, c.b_rho)]
        return list(self._params)

    def graphed_train_step(self, opt, x, y, samples, sigma=1.0, prior=None, warmup=2):
        """One Bayes-by-backprop step over the surviving weights only, captured as one hipGraph: a
        sparse_train.SparseTrainStep (train.GraphedTrainStep's contract).  `opt`: FusedAdam(self.parameters(),
        capturable=True); `prior`: an ops.PriorSpec, by default the source network's (self.prior)."""
        from .sparse_train import SparseTrainStep
        return SparseTrainStep(self, opt, x, y, samples, sigma=sigma, prior=prior, warmup=warmup)

    def to_dense(self):
        """The 12-key state dict of the pruned BayesianNetwork: what prune_weights(copy, None, drop_percentage) leaves --
        bit for bit with zero_signs, equal in value (+0 for every pruned entry) without."""
        sd = {}
        for i, c in enumerate(self._layers):
            dev = c.row_ptr.device
            counts = (c.row_ptr[1:] - c.row_ptr[:-1]).to(torch.int64)
            r = torch.repeat_interleave(torch.arange(c.fout, device=dev), counts, output_size=c.nnz)
            k = c.col[:c.nnz].to(torch.int64) & 0xFFFF
            flat = (k * c.fout + r) if self.local_reparam else (r * c.fin + k)         # index in the source layout
            shape = (c.fin, c.fout) if self.local_reparam else (c.fout, c.fin)
            for name, val, sign in (("weight_mu", c.mu_val, c.mu_sign), ("weight_rho", c.rho_val, c.rho_sign)):
                d = torch.zeros(c.fin * c.fout, dtype=torch.float32, device=dev)
                if sign is not None:
                    d = torch.where(_unpack_bits(sign, d.numel()), -d, d)               # the signed zeros of mu * 0
                d[flat] = val[:c.nnz]
                sd[f"l{i + 1}.{name}"] = d.view(shape)
            sd[f"l{i + 1}.bias_mu"], sd[f"l{i + 1}.bias_rho"] = c.b_mu.clone(), c.b_rho.clone()
        return sd

    # ------------------------------------------------------------------------------------------------ forward
    def _plan(self, rows, S, dev):
        from . import _lib as L
        key = (rows, S)
        pl = self._plans.get(key)
        if pl is None:
            c1, c2, c3 = self._layers
            f = dict(dtype=torch.float32, device=dev)
            xt = torch.empty((c1.fin, rows), **f)
            h1, h2 = torch.empty((S, c1.fout, rows), **f), torch.empty((S, c2.fout, rows), **f)
            logits = torch.empty((S, rows, c3.fout), **f)
            x0 = xt.view(rows, c1.fin)                                                  # stands in for x until a call sets it
            args = {}
            for mode in (L.EPS_ZERO, L.EPS_PHILOX):
                if mode == L.EPS_ZERO and S != 1:
                    continue
                args[mode] = [
                    ops.sparse_fwd_args(row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, sigma_val=c.sigma_val, b_mu=c.b_mu,
                                        b_sigma=c.b_sigma, x=xin, y=yout, n_samples=S, rows=rows, in_features=c.fin,
                                        out_features=c.fout, eps_mode=mode, relu=relu, x_per_sample=xps, x_feature_major=xfm,
                                        y_feature_major=yfm, layer_id=c.layer_id, x_scratch=scr)
                    for c, xin, yout, relu, xps, xfm, yfm, scr in ((c1, x0, h1, True, 0, False, True, xt),
                                                                   (c2, h1, h2, True, 1, True, True, None),
                                                                   (c3, h2, logits, False, 1, True, False, None))]
            pl = self._plans[key] = (args, logits)
        return pl

    def _x(self, x):
        ops.require_device(x)
        fin = self._layers[0].fin
        x = x.reshape(-1, fin) if self.mode == "classification" else x
        if x.dim() != 2 or x.shape[1] != fin or x.dtype != torch.float32:
            raise ops.BnnHipError(f"CompressedNetwork: x must be float32 [rows, {fin}]")
        return x if x.is_contiguous() else x.contiguous()

    def forward(self, x):
        """The mean-weight forward (eps = 0): float32 [rows, classes], in the plan's own buffer."""
        from . import _lib as L
        x = self._x(x)
        args, logits = self._plan(x.shape[0], 1, x.device)
        a = args[L.EPS_ZERO]
        a[0].x = x.data_ptr()
        for al in a:
            ops.sparse_fwd(al)
        return logits[0]

    __call__ = forward

    def forward_mc(self, x, samples, seed=None, sample_offset=None, sample_counter=None):
        """[samples, rows, classes]: `samples` draws of the surviving weights, global MC sample indices sample_offset ..
        (the next unused ones by default, as BayesianNetwork.forward_mc), Philox key `seed` (the process seed by default);
        `sample_counter`: an optional device int32 word added to sample_offset when the kernels run."""
        from . import _lib as L
        from .runtime import state, take_samples
        x, S = self._x(x), int(samples)
        args, logits = self._plan(x.shape[0], S, x.device)
        a = args[L.EPS_PHILOX]
        first = take_samples(S) if sample_offset is None else int(sample_offset)
        sd = state.seed if seed is None else int(seed)
        a[0].x = x.data_ptr()
        for al in a:
            al.seed, al.sample_offset = sd & 0xFFFFFFFFFFFFFFFF, first & 0xFFFFFFFF
            al.sample_counter = None if sample_counter is None else sample_counter.data_ptr()
            ops.sparse_fwd(al)
        return logits

    def predict_mc(self, x, samples, **kw):
        """(preds [rows], probs [rows, classes]): the mean softmax over forward_mc's samples (ops.mc_predictive)."""
        p = ops.mc_predictive(self.forward_mc(x, samples, **kw), "classification")
        return p.preds[0], p.probs[0]

    def predictive(self, x, samples, *, quantiles=None, sigma=1., **kw):
        """BayesianNetwork.predictive over forward_mc's samples: ops.mc_predictive, one minibatch."""
        from .engine import _first_minibatch
        q = ops.quantile_levels(quantiles) if self.mode == "regression" else ()
        return _first_minibatch(ops.mc_predictive(self.forward_mc(x, samples, **kw), self.mode, sigma=float(sigma), quantiles=q))

    def score(self, x, y, samples, *, sigma=1., bins=10, **kw):
        """BayesianNetwork.score over forward_mc's samples: ops.mc_score (an ops.Scores)."""
        return ops.mc_score(self.forward_mc(x, samples, **kw), y, self.mode, sigma=float(sigma), bins=int(bins))

    def evaluate(self, data, bin_step=0.1, batch_size=128):
        """PruneSweep.evaluate for this one level with the mean-weight forward: a PruneSweepResult of one level (accuracy,
        nll, ece, bins ... or sse); `data` a DeviceLoader or a pair of device tensors."""
        from . import _lib as L
        from .epoch import DeviceLoader
        cls = self.mode == "classification"
        C_ = self._layers[2].fout
        if isinstance(data, DeviceLoader):
            N, batches, dev = len(data) * data.batch_size, iter(data), data.dataset.device
        else:
            X, Y = data
            ops.require_device(X, Y)
            N, dev, bs = int(X.shape[0]), X.device, int(batch_size)
            batches = ((X[i:i + bs], Y[i:i + bs]) for i in range(0, N, bs))
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        probs = correct = labels = ece_out = None
        if cls:
            probs = torch.empty((1, N, C_), dtype=torch.float32, device=dev)
            correct = torch.zeros(1, dtype=torch.int64, device=dev)
            labels = torch.empty(N, dtype=torch.int64, device=dev)
        mode = L.NLL_CLASSIFICATION if cls else L.NLL_REGRESSION
        row0 = 0
        with torch.no_grad():
            for x, y in batches:
                logits = self.forward(x).unsqueeze(0)
                rows = logits.shape[1]
                y = (y if cls else y.reshape(rows, C_)).contiguous()
                if cls:
                    labels[row0:row0 + rows].copy_(y)
                ops.prune_sweep_tail(logits, y, mode=mode, probs=probs, correct=correct, loss=loss, row0=row0, n_total=N)
                row0 += rows
            if row0 != N:
                raise ops.BnnHipError(f"CompressedNetwork.evaluate: the data handed out {row0} rows, not {N}")
            if cls:
                ece_out = ops.ece_bins(probs[0], labels, np.arange(0, 1.1, bin_step)).unsqueeze(0)
        kept = torch.tensor([sum(self.nnz)], dtype=torch.int64)
        return PruneSweepResult(self.mode, N, correct, loss, ece_out, probs, labels, self.threshold, kept, bin_step)


def compress(net, drop_percentage=0.5, zero_signs=True):
    """prune_weights(net, None, drop_percentage) without touching net: a one-level PruneSweep, compressed."""
    return PruneSweep(net, (float(drop_percentage),)).compress(0, zero_signs=zero_signs)
