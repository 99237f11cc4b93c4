"""numpy restatement of F11 (bnn_param_hist, bnn_hip.diagnostics): the bin table of SummaryWriter.default_bins, the binning
of np.histogram with the out-of-range / NaN tallies and the moments of a record, the support rule of
torch.utils.tensorboard.summary.make_histogram, and the reference's write_weight_histograms (utils/logger_utils.py:13-26) and
collect_weights (weight_pruning.py:16-41) on numpy arrays."""
import numpy as np

TAGS = tuple(f"histogram/{p}{i}_{s}" for i in (1, 2, 3) for p in ("w",) for s in ("mu", "rho")) + \
    tuple(f"histogram/{p}{i}_{s}" for i in (1, 2, 3) for p in ("b",) for s in ("mu", "rho"))   # logger_utils.py:15-26, in order
SCALARS_4 = ("logs/loss", "logs/complexity_cost", "logs/log_prior", "logs/log_variational_posterior", "logs/negative_log_likelihood")
SCALARS_3 = ("logs/loss", "logs/complexity_cost", "logs/negative_log_likelihood")


def default_bins():
    """torch.utils.tensorboard.SummaryWriter.__init__: the loop, verbatim."""
    v = 1e-12
    buckets = []
    neg_buckets = []
    while v < 1e20:
        buckets.append(v)
        neg_buckets.append(-v)
        v *= 1.1
    return buckets, neg_buckets[::-1] + [0] + buckets


def record(v, edges):
    """What a job's record must hold for the fp32 values v."""
    v = np.asarray(v, np.float32).reshape(-1)
    edges = np.asarray(edges, np.float64)
    d = v.astype(np.float64)
    nan = np.isnan(d)
    ok = d[~nan]
    fin = ok[np.isfinite(ok)]
    counts = np.histogram(ok, bins=edges)[0]
    return dict(counts=counts.astype(np.int64), n_in=int(counts.sum()), n_below=int((ok < edges[0]).sum()),
                n_above=int((ok > edges[-1]).sum()), n_nan=int(nan.sum()),
                min=np.float32(ok.min()) if ok.size else np.float32(np.inf), max=np.float32(ok.max()) if ok.size else np.float32(-np.inf),
                sum=float(fin.sum()), sum_sq=float((fin * fin).sum()), abs_sum=float(np.abs(fin).sum()), n=int(v.size))


def trim(counts, limits):
    """make_histogram's support rule: returns (bucket_counts, bucket_limits) exactly as its slices come out."""
    counts, limits = np.asarray(counts), np.asarray(limits)
    cum_counts = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum_counts, [0, cum_counts[-1] - 1], side="right")
    start = int(start)
    end = int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    return counts, limits


def softplus(rho):
    """torch.log1p(torch.exp(rho)) in fp32 (logger_utils.py:16)."""
    return np.log1p(np.exp(np.asarray(rho, np.float32))).astype(np.float32)


def weight_histograms(params, edges):
    """write_weight_histograms over {"l1.weight_mu": ndarray, ...}: per tag what add_histogram -> make_histogram records
    (counts, limits, num, min, max), with the fp32 softplus the caller supplies under "<name>_sigma" keys."""
    out = {}
    for p, q in (("w", "weight"), ("b", "bias")):                       # logger_utils.py:15-26: w1 .. w3, then b1 .. b3
        for i in (1, 2, 3):
            for s, v in (("mu", params[f"l{i}.{q}_mu"]), ("rho", params[f"l{i}.{q}_sigma"])):
                v = np.asarray(v, np.float32).reshape(-1)
                counts, limits = trim(*np.histogram(v.astype(np.float64), bins=edges))
                out[f"histogram/{p}{i}_{s}"] = dict(bucket_counts=counts.tolist(), bucket_limits=limits.tolist(), num=int(v.size),
                                                    min=float(v.min()), max=float(v.max()))
    return out


def collect_weights(named, bnn=False):
    """weight_pruning.py:16-38 over [(name, ndarray)]: python lists of floats, sigma = np.log(1 + np.exp(rho)) per element."""
    mus, rhos, weights = [], [], []
    for name, param in named:
        if 'mu' in name:
            mus.append(param.flatten().tolist())
        elif 'rho' in name:
            rhos.append(param.flatten().tolist())
        else:
            weights.append(param.flatten().tolist())
    mus = [item for sublist in mus for item in sublist]
    rhos = [item for sublist in rhos for item in sublist]
    weights = [item for sublist in weights for item in sublist]
    if bnn:
        sigmas = [np.log(1 + np.exp(rho)) for rho in rhos]
        weights = [mus, sigmas]
    return weights
