"""float64 numpy restatement of bnn_mc_score (include/bnn_hip.h F12): per-row values and the record fields, and for each
case the margins that say whether a comparison of integer words (argmax, bins) is meaningful -- the smallest top-2 gap of
the mean probabilities and the smallest distance of conf * M / u * M to a bin edge.

Bin edges: only the interior edges 1 .. M-1 separate bins.  conf = 1 (conf * M = M) and u = 0 or 1 (u * M = 0 or M) sit on
the OUTER edges, where the clamp min(M - 1, .) decides and a rounding error cannot move a value into another bin (conf and u
cannot leave [0, 1]); the margins therefore measure the distance to the nearest interior edge."""
import math

import numpy as np

try:
    from scipy.special import erfc as _erfc
except Exception:                                           # scipy is optional
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _interior_margin(v, M):
    """min over the finite entries of v of the distance of v * M to the nearest integer in 1 .. M - 1 (inf without one)."""
    v = np.asarray(v, np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    if M < 2 or v.size == 0:
        return float("inf")
    edges = np.arange(1, M, dtype=np.float64)
    return float(np.abs(v[:, None] * M - edges[None, :]).min())


def _logsumexp(a, axis):
    """log sum exp along `axis`; -inf where every term is -inf, NaN where a term is NaN."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(np.where(np.isnan(a), -np.inf, a), axis=axis, keepdims=True)
        safe = np.where(np.isfinite(m), m, 0.0)
        out = np.log(np.exp(a - safe).sum(axis=axis)) + np.squeeze(safe, axis)
    return out


def classification(logits, labels, n_bins, n_valid=None):
    """logits [G, S, B, C], labels int [G, B].  Returns a dict: per-row lpd, nll, brier, conf, pred, correct, bin ([n_valid]
    in flat row order; bin -1 = none) and the record fields rows, n_correct, sum_lpd, sum_nll, sum_brier, bin_count,
    bin_correct, bin_conf, plus min_top2_gap and min_edge_distance."""
    lg = np.asarray(logits, np.float32).astype(np.float64)
    G, S, B, C = lg.shape
    n_valid = G * B if n_valid is None else int(n_valid)
    z = lg.transpose(0, 2, 1, 3).reshape(G * B, S, C)[:n_valid]              # [rows, S, C]
    y = np.asarray(labels, np.int64).reshape(G * B)[:n_valid]
    M = int(n_bins)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = z.max(-1, keepdims=True)                                         # NaN if the sample holds one
        e = np.exp(z - m)
        se = e.sum(-1, keepdims=True)
        p = e / se
        onehot = np.arange(C)[None, :] == y[:, None]                         # [rows, C]; all False for a label outside [0, C)
        inside = onehot.any(-1)
        zy = np.where(onehot[:, None, :], z, 0.0).sum(-1)                    # [rows, S]
        logp = (zy - m[..., 0]) - np.log(se[..., 0])
        logp = np.where(inside[:, None], logp, -np.inf)
        lpd = _logsumexp(logp, 1) - math.log(S)
        nll = -logp.sum(1) / S
        pbar = p.sum(1) / S
        brier = ((pbar - onehot) ** 2).sum(-1)
        nan_row = np.isnan(pbar).any(-1)
        safe = np.where(nan_row[:, None], 0.0, pbar)
        pred = safe.argmax(-1)                                               # first maximum: lowest index on ties
        conf = np.where(nan_row, np.nan, safe.max(-1))
        correct = (~nan_row) & (pred == y)
        bins = np.full(n_valid, -1, np.int64)
        if M > 0:
            ok = ~nan_row
            bins[ok] = np.minimum(M - 1, np.ceil(conf[ok] * M).astype(np.int64) - 1)
        top2 = np.sort(safe, -1)[:, -2:] if C > 1 else None
    count = np.array([(bins == i).sum() for i in range(M)], np.int64)
    bcorrect = np.array([correct[bins == i].sum() for i in range(M)], np.int64)
    bconf = np.array([conf[bins == i].sum() for i in range(M)], np.float64)
    gap = float("inf") if C == 1 or (~nan_row).sum() == 0 else float((top2[~nan_row, 1] - top2[~nan_row, 0]).min())
    return dict(lpd=lpd, nll=nll, brier=brier, conf=conf, pred=pred, correct=correct, bin=bins, rows=n_valid,
                n_correct=int(correct.sum()), sum_lpd=float(lpd.sum()), sum_nll=float(nll.sum()), sum_brier=float(brier.sum()),
                bin_count=count, bin_correct=bcorrect, bin_conf=bconf, min_top2_gap=gap,
                min_edge_distance=_interior_margin(conf, M))


def regression(outputs, targets, sigma, n_bins, n_valid=None):
    """outputs [G, S, B, C], targets [G, B, C]; sigma as the kernel sees it (a float32 value).  Returns per-element lpd, nll,
    sq_err, abs_err, pit, bin ([n_valid * C]), per-row row_lpd / row_nll ([n_valid]) and the record fields rows, elements,
    sum_lpd, sum_nll, sum_sq, sum_abs, bin_count, plus min_edge_distance."""
    f = np.asarray(outputs, np.float32).astype(np.float64)
    G, S, B, C = f.shape
    n_valid = G * B if n_valid is None else int(n_valid)
    f = f.transpose(0, 2, 3, 1).reshape(G * B * C, S)[:n_valid * C]          # [elements, S]
    y = np.asarray(targets, np.float32).astype(np.float64).reshape(G * B * C)[:n_valid * C]
    sg = float(np.float32(sigma))
    M = int(n_bins)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = y[:, None] - f
        q = d * d / (2.0 * sg * sg)
        norm = math.log(sg) + HALF_LOG_2PI
        lpd = _logsumexp(-q, 1) - math.log(S) - norm
        nll = q.sum(1) / S + norm
        err = y - f.sum(1) / S
        u = (0.5 * _erfc(-(d / sg) / math.sqrt(2.0))).sum(1) / S
        bins = np.full(u.shape, -1, np.int64)
        if M > 0:
            ok = ~np.isnan(u)
            bins[ok] = np.minimum(M - 1, np.floor(u[ok] * M).astype(np.int64))
    count = np.array([(bins == i).sum() for i in range(M)], np.int64)
    return dict(lpd=lpd, nll=nll, sq_err=err * err, abs_err=np.abs(err), pit=u, bin=bins,
                row_lpd=lpd.reshape(n_valid, C).sum(1), row_nll=nll.reshape(n_valid, C).sum(1), rows=n_valid,
                elements=n_valid * C, sum_lpd=float(lpd.sum()), sum_nll=float(nll.sum()), sum_sq=float((err * err).sum()),
                sum_abs=float(np.abs(err).sum()), bin_count=count, min_edge_distance=_interior_margin(u, M))


def record_words(ref, mode, n_bins):
    """The restatement's record as bnn_mc_score lays it out: int64 [8 + 3 * n_bins] (fp64 words by their bits)."""
    w = np.zeros(8 + 3 * n_bins, np.int64)
    f = w.view(np.float64)
    w[0] = ref["rows"]
    f[2], f[3] = ref["sum_lpd"], ref["sum_nll"]
    if mode == "classification":
        w[1], f[4] = ref["n_correct"], ref["sum_brier"]
    else:
        w[1], f[4], f[5] = ref["elements"], ref["sum_sq"], ref["sum_abs"]
    for i in range(n_bins):
        w[8 + 3 * i] = ref["bin_count"][i]
        if mode == "classification":
            w[8 + 3 * i + 1] = ref["bin_correct"][i]
            f[8 + 3 * i + 2] = ref["bin_conf"][i]
    return w


INT_WORDS = lambda n_bins: [0, 1] + [8 + 3 * i + j for i in range(n_bins) for j in (0, 1)]        # noqa: E731
F64_WORDS = lambda n_bins: [2, 3, 4, 5] + [8 + 3 * i + 2 for i in range(n_bins)]                  # noqa: E731


def assert_record(got_words, ref, mode, n_bins, rel=1e-10):
    """Integer words exact; fp64 words within rel * max(1, |ref|), NaN where the restatement is NaN."""
    got = np.asarray(got_words, np.int64).reshape(-1)
    want = record_words(ref, mode, n_bins)
    assert got.shape == want.shape
    ii = INT_WORDS(n_bins)
    assert np.array_equal(got[ii], want[ii]), (got[ii], want[ii])
    assert (got[6:8] == 0).all()
    gf, wf = got.view(np.float64), want.view(np.float64)
    for i in F64_WORDS(n_bins):
        if np.isnan(wf[i]):
            assert np.isnan(gf[i]), (i, gf[i])
        elif np.isinf(wf[i]):
            assert gf[i] == wf[i], (i, gf[i], wf[i])
        else:
            assert abs(gf[i] - wf[i]) <= rel * max(1.0, abs(wf[i])), (i, gf[i], wf[i])
