"""F11 host side: the reference's per-epoch posterior histograms (utils/logger_utils.py:13-26, write_weight_histograms) and
the SNR density / CDF of weight_pruning.py:59-79 from ONE device pass over the parameters (bnn_param_hist): the transform
(softplus, SNR, a posterior sample) is fused into the binning, a few KB of counts are written, and nothing is read back
before `read()` -- one device-to-host copy of every record.

`PosteriorStats.read()` returns, per tag, the keyword arguments of SummaryWriter.add_histogram_raw (TensorBoard is not a
dependency: the bin table of SummaryWriter.default_bins and the trimming of make_histogram are restated here)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import ops


def tensorboard_bins() -> np.ndarray:
    """SummaryWriter.default_bins: v = 1e-12, v *= 1.1 while v < 1e20, mirrored around 0 -- by the same repeated
    multiplication, so the float64 edges are the writer's own."""
    v, buckets = 1e-12, []
    while v < 1e20:
        buckets.append(v)
        v *= 1.1
    return np.array([-b for b in buckets[::-1]] + [0.0] + buckets, dtype=np.float64)


def uniform_bins(lo: float, hi: float, n: int) -> np.ndarray:
    """n + 1 evenly spaced float64 edges from lo to hi."""
    if not (int(n) >= 1 and float(lo) < float(hi)):
        raise ops.BnnHipError("uniform_bins: n >= 1 bins over lo < hi")
    return np.linspace(float(lo), float(hi), int(n) + 1, dtype=np.float64)


def trim_histogram(counts, limits):
    """The support rule of torch.utils.tensorboard.summary.make_histogram: the bins from the first to the last non-empty
    one, with one (possibly added) empty bin on the left so that the leftmost limit survives; TensorBoard keeps right limits
    only, so both results have the same length.  All counts zero: both are empty (make_histogram raises there)."""
    counts, limits = np.asarray(counts), np.asarray(limits)
    cum = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum, [0, cum[-1] - 1], side="right")
    start, end = int(start), int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    if counts.size == 0 or limits.size == 0 or not counts.any():
        return counts[:0], limits[:0]
    return counts, limits


def _bayesian_network_layers(net):
    layers = [getattr(net, n, None) for n in ("l1", "l2", "l3")]
    if all(l is not None and hasattr(l, "weight_mu") and hasattr(l, "weight_rho") and hasattr(l, "bias_mu") for l in layers):
        return layers
    return None


class _Call:
    """One bnn_param_hist call: its tags, its edge table and where its records sit in the shared buffer."""

    def __init__(self, tags, jobs, edges):
        self.tags, self.jobs, self.edges = tags, jobs, ops.hist_edges(edges)
        self.words = L.hist_record_bytes(self.edges.size) // 8
        self.args, self.offset = None, 0


class PosteriorStats:
    """Histograms and moments of a model's parameters, planned once into static buffers.

    net: a BayesianNetwork (either layer type) -- the reference's twelve tags `histogram/w1_mu`, `histogram/w1_rho` (which,
    as in the reference, holds sigma = softplus(rho)) ... `histogram/b3_rho` over `bins`; with `snr_bins` also `snr/w1` ...
    `snr/b3` (10 log10(|mu| / sigma), dB) over that table.  Any other module: `histogram/<parameter name>` of its float32
    parameters.  `update()` launches bnn_param_hist once per table (the twelve tensors of a network are one call), is
    capturable and reads nothing; `update(sample=s)` also bins one posterior sample per (mu, rho) tensor,
    `sample/w1` ... `sample/b3`, on the network's seed and epsilon tensor ids at global sample index s.  `read()` is one copy."""

    def __init__(self, net, bins=None, snr_bins=None, sample_bins=None):
        bins = tensorboard_bins() if bins is None else bins
        layers = _bayesian_network_layers(net)
        self._calls, self._sample_call, self._sampled, self._snapshot = [], None, False, None
        if layers is not None:
            pairs = []
            for which, mu, rho, kind in (("w", "weight_mu", "weight_rho", 0), ("b", "bias_mu", "bias_rho", 1)):
                for i, l in enumerate(layers):
                    pairs.append((f"{which}{i + 1}", getattr(l, mu).detach(), getattr(l, rho).detach(),
                                  4 * int(getattr(l, "_layer_id", i)) + kind))
            tags, jobs = [], []
            for name, mu, rho, _ in pairs:
                tags += [f"histogram/{name}_mu", f"histogram/{name}_rho"]
                jobs += [dict(kind=L.HIST_VALUE, src0=mu), dict(kind=L.HIST_SIGMA, src0=rho)]
            self._calls.append(_Call(tags, jobs, bins))
            if snr_bins is not None:
                self._calls.append(_Call([f"snr/{n}" for n, *_ in pairs],
                                         [dict(kind=L.HIST_SNR_DB, src0=mu, src1=rho) for _, mu, rho, _ in pairs], snr_bins))
            from .runtime import state
            self._sample_call = _Call([f"sample/{n}" for n, *_ in pairs],
                                      [dict(kind=L.HIST_SAMPLE, src0=mu, src1=rho, seed=state.seed, tensor_id=t, sample=0)
                                       for _, mu, rho, t in pairs], bins if sample_bins is None else sample_bins)
        else:
            named = [(n, p.detach()) for n, p in net.named_parameters()]
            if not named:
                raise ops.BnnHipError("PosteriorStats: the module has no parameters")
            for i in range(0, len(named), L.HIST_MAX_JOBS):
                part = named[i:i + L.HIST_MAX_JOBS]
                self._calls.append(_Call([f"histogram/{n}" for n, _ in part], [dict(kind=L.HIST_VALUE, src0=p) for _, p in part], bins))
        calls = self._calls + ([self._sample_call] if self._sample_call is not None else [])
        total = 0
        for c in calls:
            c.offset = total
            total += len(c.jobs) * c.words
        probe = calls[0].jobs[0]["src0"]
        ops.require_device(probe)                                            # no CPU fallback: nothing is allocated off the device
        self._records = torch.zeros(total, dtype=torch.int64, device=probe.device)
        for c in calls:
            view = self._records[c.offset:c.offset + len(c.jobs) * c.words].view(len(c.jobs), c.words)
            c.args = ops.param_hist_args(c.jobs, c.edges, records=view)
        self.tags = tuple(t for c in self._calls for t in c.tags)

    def update(self, sample=None):
        """Enqueue the pass on the current stream.  Static buffers, no allocation, no host read: capturable."""
        for c in self._calls:
            ops.param_hist(c.args)
        self._sampled = sample is not None
        if self._sampled:
            if self._sample_call is None:
                raise ops.BnnHipError("PosteriorStats: posterior samples need a BayesianNetwork")
            for i in range(len(self._sample_call.jobs)):
                self._sample_call.args.jobs[i].sample = int(sample) & 0xFFFFFFFF
            ops.param_hist(self._sample_call.args)
        self._snapshot = None
        return self

    # ---- host side
    def _raw(self, refresh=False):
        if refresh or self._snapshot is None:
            host = self._records.cpu().numpy()                                # the one device-to-host copy
            snap = {}
            for c in self._calls + ([self._sample_call] if self._sampled else []):
                nb = c.edges.size - 1
                rec = host[c.offset:c.offset + len(c.jobs) * c.words].reshape(len(c.jobs), c.words)
                for i, tag in enumerate(c.tags):
                    row = rec[i]
                    head = row[nb:nb + 4].view(np.uint64)
                    mnmx = row[nb + 4:nb + 5].view(np.float32)
                    sums = row[nb + 5:nb + 7].view(np.float64)
                    snap[tag] = dict(edges=c.edges, counts=row[:nb].view(np.uint64).astype(np.int64), n_in=int(head[0]),
                                     n_below=int(head[1]), n_above=int(head[2]), n_nan=int(head[3]), min=float(mnmx[0]),
                                     max=float(mnmx[1]), sum=float(sums[0]), sum_sq=float(sums[1]),
                                     num=int(c.args.jobs[i].n))
            self._snapshot = snap
        return self._snapshot

    def raw(self, tag=None):
        """The untrimmed record(s) as of the last read() (read now when there was none): edges, counts, n_in, n_below,
        n_above, n_nan, min, max, sum, sum_sq, num.  density() and cdf() look at the same snapshot."""
        snap = self._raw()
        return snap if tag is None else snap[tag]

    def read(self):
        """{tag: fields}: `writer.add_histogram_raw(tag, **fields, global_step=step)`.  num counts every element, as
        make_histogram's len(values); bucket_limits are right edges.  Every call copies the records anew (a replayed graph
        may have rewritten them)."""
        out = {}
        for tag, r in self._raw(refresh=True).items():
            counts, limits = trim_histogram(r["counts"], r["edges"])
            out[tag] = dict(min=r["min"], max=r["max"], num=r["num"], sum=r["sum"], sum_squares=r["sum_sq"],
                            bucket_limits=limits.tolist(), bucket_counts=counts.tolist())
        return out

    def density(self, tag):
        """(bin centres, counts / (n_in * bin width)): the histogram as a probability density over the table's range."""
        r = self._raw()[tag]
        e, c = r["edges"], r["counts"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (e[:-1] + e[1:]) / 2, c / (r["n_in"] * np.diff(e))

    def cdf(self, tag):
        """The cumulative share of the tag's elements at each right edge (raw(tag)["edges"][1:]), counting the elements inside
        the table's range: the last entry is n_in / num."""
        r = self._raw()[tag]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.cumsum(r["counts"]) / r["num"]
