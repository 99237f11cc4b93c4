"""TEST INFRASTRUCTURE: the ELBO loss tail in float64 -- per-sample NLL, its logit gradient, the loss assembly and the
ELBO sums -- and the fp32 error bound the HIP tail kernels are held to.  Inputs are the fp32 arrays a launch read (its own
logits, its own per-sample scalars); everything here is computed in float64 from them, so the bound only has to cover
the tail's own fp32 rounding, not the matmul's.

Reference arithmetic: networks.py:183-190 (get_nll: cross-entropy with reduction='sum', or -sum Normal(y, sigma).log_prob(t)),
:205-208 / :222-224 (the ELBO), and the device's loss seeds (reduce.hip elbo_loss_block / bnn_fin.h fin_loss_assemble).

A label outside [0, C) gives NaN for its row here, as the kernels do (they poison the row instead of reading out of bounds).
"""
import math

import numpy as np

ULP = 2.0 ** -23           # fp32 spacing at 1.0 (= 2 u, u the unit roundoff of round-to-nearest)
C0 = 0.5 * math.log(2.0 * math.pi)

SPECIAL_KINDS = ("plain", "equal", "spike_up", "spike_down", "offset")


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_logits(S, B, C, seed, scale=3.0, special=True):
    """fp32 [S, B, C] logits, seeded N(0, scale^2).  `special` (the classification inputs): rows b < 4 of sample s are of
    kind SPECIAL_KINDS[(s + b) % 5] -- all-equal (CE = log C exactly), one logit at +60 / -60 against the rest, a common
    offset of 1e3 (no max-subtraction: exp overflows)."""
    rs = np.random.RandomState(seed)
    lg = (rs.standard_normal((S, B, C)) * scale).astype(np.float32)
    for s in range(S if special else 0):
        for b in range(min(B, 4)):
            kind = SPECIAL_KINDS[(s + b) % 5]
            if kind == "equal":
                lg[s, b] = np.float32(0.375)
            elif kind == "spike_up":
                lg[s, b, (s + 7 * b) % C] = 60.0
            elif kind == "spike_down":
                lg[s, b, (s + 3 * b) % C] = -60.0
            elif kind == "offset":
                lg[s, b] += np.float32(1000.0)
    return lg


def make_labels(B, C, seed, groups=1):
    """int64 [groups, B]: seeded labels with 0 and C-1 placed on purpose (first and last row of every group; row 1 of
    group g > 0 holds (g * 7) % C, so that the groups differ)."""
    rs = np.random.RandomState(seed + 1)
    t = rs.randint(0, C, (groups, B)).astype(np.int64)
    t[:, 0] = 0
    t[:, -1] = C - 1
    for g in range(1, groups):
        if B > 2:
            t[g, 1] = (g * 7) % C
    return t


def make_reg_targets(B, C, seed, groups=1):
    rs = np.random.RandomState(seed + 2)
    return rs.standard_normal((groups, B, C)).astype(np.float32)


def per_sample_targets(target, S):
    """Targets of each of the S samples from `target` [G, B] / [G, B, C]: one block shared by all samples (G = 1), or one
    per group of S / G consecutive samples (sample s reads block s // (S / G): group_samples with target_per_group)."""
    t = np.asarray(target)
    G = t.shape[0]
    assert S % G == 0, "target groups must divide the samples"
    return t[np.arange(S) // (S // G)]


# ------------------------------------------------------------------------------------------------------------------ NLL
def _lse_parts(lg):
    x = np.asarray(lg, np.float64)
    m = x.max(-1)
    se = np.exp(x - m[..., None]).sum(-1)
    return x, m, np.log(se)


def _picked(x, t, C):
    ok = (t >= 0) & (t < C)
    tc = np.where(ok, t, 0)
    pk = np.take_along_axis(x, tc[..., None], -1)[..., 0]
    return np.where(ok, pk, np.nan), ok


def nll_rows(logits, target, mode, sigma=1.0):
    """float64 [S, B]: the NLL of every row (classification: lse - picked; regression: -sum_c log N(t; y, sigma))."""
    lg = np.asarray(logits)
    S, B, C = lg.shape
    t = per_sample_targets(target, S)
    if mode == "classification":
        x, m, l = _lse_parts(lg)
        pk, _ = _picked(x, t.reshape(S, B), C)
        return (m + l) - pk
    d = np.asarray(t, np.float64).reshape(S, B, C) - np.asarray(lg, np.float64)
    return (d * d / (2.0 * sigma * sigma) + math.log(sigma) + C0).sum(-1)


def nll(logits, target, mode, sigma=1.0):
    """float64 [S]: the per-sample summed NLL (networks.py:183-190)."""
    return nll_rows(logits, target, mode, sigma).sum(-1)


def nll_tol(logits, target, mode, sigma=1.0):
    """float64 [S]: what fp32 arithmetic may move the per-sample NLL by, summed from per-row bounds.

    Classification, a row with max m, lse = m + log sum exp(x - m), picked logit p (bnn_fin.h fin_nll, the K1r / K3r inline
    copies):  ULP * (4 (|m| + |lse - m| + |p|) + 2 (1 + ln C) + C / 2)
      4 (|m| + |lse - m| + |p|): (m + log se) - p is two fp32 roundings, u each of operands bounded by these three, and
        __logf / logf (v_log_f32 times ln 2) adds <= 2 roundings of |lse - m|: 4 u (...) = 2 ULP (...), doubled for margin;
      2 (1 + ln C): each exp term is off by u (v_exp_f32) + u |x - m| (the rounding of x - m and of (x - m) log2 e);
        weighted by the softmax, E_p |x - m| <= H(p) <= ln C, so log se moves by <= 2 u (1 + ln C) = ULP (1 + ln C), x2;
      C / 2: the fp32 sum of the C positive terms, <= (C - 1) u relative (sequential; the wave-strided form is shallower),
        which log turns into an absolute error on lse.
    Regression, a row with sum_c d^2 / (2 sigma^2) = q and C constants log sigma + c0:
      ULP * (2 q n_q + 2 C |log sigma + c0|), n_q = ceil(B / 4) ceil(C / 64) + min(C, 16) + 8 terms at most on one accumulator (the
      wide form sums d^2 in fp32 over a lane's rows and columns before the affine map; the narrow forms convert every
      element to fp32 and add it, <= 16 per thread; +8 for the fma and subtraction roundings and the fold).
    Row sum: each row value is added in fp32 to an accumulator that takes at most ceil(B / 4) rows (a wave-per-row lane
    takes every fourth row) and then 6 wave-tree levels and one fp32 rounding of the fp64 fold:
      + ULP * (ceil(B / 4) + 8) * sum_b |row_b|   (ULP rather than u: margin for the tree's regrouping)."""
    lg = np.asarray(logits)
    S, B, C = lg.shape
    t = per_sample_targets(target, S)
    rows = nll_rows(logits, target, mode, sigma)
    if mode == "classification":
        x, m, l = _lse_parts(lg)
        pk, ok = _picked(x, t.reshape(S, B), C)
        pk = np.where(ok, pk, 0.0)
        per = ULP * (4.0 * (np.abs(m) + np.abs(l) + np.abs(pk)) + 2.0 * (1.0 + math.log(C)) + C / 2.0)
    else:
        d = np.asarray(t, np.float64).reshape(S, B, C) - np.asarray(lg, np.float64)
        q = (d * d).sum(-1) / (2.0 * sigma * sigma)
        n_q = math.ceil(B / 4) * math.ceil(C / 64) + min(C, 16) + 8
        per = ULP * (2.0 * q * n_q + 2.0 * C * abs(math.log(sigma) + C0))
    rsum = ULP * (math.ceil(B / 4) + 8) * np.nansum(np.abs(rows), -1)
    return np.nansum(per, -1) + rsum


# ------------------------------------------------------------------------------------------------------------------ gradient
def nll_grad(logits, target, mode, sigma=1.0, gs=1.0):
    """float64 [S, B, C]: d (per-sample summed NLL) / d logits times gs (a scalar or [S]): (softmax - onehot) gs or
    (y - t) / sigma^2 gs.  A bad label makes its row NaN."""
    lg = np.asarray(logits)
    S, B, C = lg.shape
    g = np.broadcast_to(np.asarray(gs, np.float64), (S,))[:, None, None]
    t = per_sample_targets(target, S)
    if mode == "classification":
        x, m, l = _lse_parts(lg)
        p = np.exp(x - (m + l)[..., None])
        t = t.reshape(S, B)
        ok = (t >= 0) & (t < C)
        oh = (np.arange(C)[None, None, :] == t[..., None]).astype(np.float64)
        out = (p - oh) * g
        return np.where(ok[..., None], out, np.nan)
    return (np.asarray(lg, np.float64) - np.asarray(t, np.float64).reshape(S, B, C)) / (sigma * sigma) * g


def nll_grad_tol(logits, target, mode, sigma=1.0, gs=1.0):
    """float64 [S, B, C], elementwise.  Classification: (exp(x - m) * (1 / se) - onehot) * gs in fp32 --
      |gs| ULP (p_i (|x_i - m| + 1 + ln C + C / 2 + 4) + 2 |p_i - onehot_i|) + |gs| 2^-125:
      p_i |x_i - m| + p_i: the exp term's own error (as in nll_tol); p_i (ln C + C / 2): se's error through 1 / se; 4 p_i: the
      reciprocal and the product; 2 |p_i - onehot_i|: the subtraction and the scaling by gs; 2^-125: exp results that
      fall below the smallest normal fp32 may be flushed to zero.
    Regression, (y - t) * (1 / sigma^2) * gs: three roundings of the result and one of y - t: 3 ULP |result| + tiny."""
    lg = np.asarray(logits)
    S, B, C = lg.shape
    g = np.abs(np.broadcast_to(np.asarray(gs, np.float64), (S,)))[:, None, None]
    if mode == "classification":
        x, m, l = _lse_parts(lg)
        p = np.exp(x - (m + l)[..., None])
        t = per_sample_targets(target, S).reshape(S, B)
        oh = (np.arange(C)[None, None, :] == t[..., None]).astype(np.float64)
        return g * (ULP * (p * (np.abs(x - m[..., None]) + 1.0 + math.log(C) + C / 2.0 + 4.0) + 2.0 * np.abs(p - oh)) + 2.0 ** -125)
    r = np.abs(nll_grad(logits, target, mode, sigma, gs))
    return 3.0 * ULP * r + g * 2.0 ** -125


# ------------------------------------------------------------------------------------------------------------------ loss
def loss_assembly(a, b, nll_s, beta, total, grad_scale, local_reparam):
    """float64 (out4, g_a, g_b, g_kl3) of elbo_loss_block / fin_loss_assemble from the per-sample scalars a (log p | KL),
    b (log q; ignored under local reparameterisation) and nll, and the fp32 beta the device reads:
      out4 = {beta mean b - beta mean a + mean nll | beta mean kl + mean nll, mean a, mean b, mean nll} (means over `total`),
      g_a = -beta grad_scale / total (0 for LR), g_b = beta grad_scale / total, g_kl3 = {beta grad_scale, 0, 0}."""
    a = np.asarray(a, np.float64)
    S = a.shape[0]
    b = np.zeros(S) if (b is None or local_reparam) else np.asarray(b, np.float64)
    n = np.asarray(nll_s, np.float64)
    beta = float(np.float32(beta))
    am, bm, nm = a.sum() / total, b.sum() / total, n.sum() / total
    loss = beta * am + nm if local_reparam else beta * bm - beta * am + nm
    inv = grad_scale / total
    g_a = np.full(S, 0.0 if local_reparam else -beta * inv)
    g_b = np.full(S, beta * inv)
    return np.array([loss, am, bm, nm]), g_a, g_b, np.array([beta * grad_scale, 0.0, 0.0])


def loss_assembly_tol(a, b, nll_s, beta, total, grad_scale, local_reparam):
    """Bounds for loss_assembly's outputs in fp32: the means are an fp64 sum rounded to fp32 and one fp32 division (2
    roundings: 1 ULP of the mean); the loss adds up to three products (beta * mean: one more rounding) in fp32:
    ULP (2 (|beta am| + |beta bm| + |nm|) + |loss|) -- every operand rounded at most twice more, and the result once.
    The seeds are one or two fp32 operations: 1 ULP of their size."""
    (loss, am, bm, nm), g_a, g_b, g_kl3 = loss_assembly(a, b, nll_s, beta, total, grad_scale, local_reparam)
    beta = float(np.float32(beta))
    t4 = np.array([ULP * (2.0 * (abs(beta * am) + abs(beta * bm) + abs(nm)) + abs(loss)), ULP * abs(am), ULP * abs(bm),
                   ULP * abs(nm)]) + 1e-30
    return t4, ULP * np.abs(g_a) + 1e-30, ULP * np.abs(g_b) + 1e-30, ULP * np.abs(g_kl3) + 1e-30


def elbo_sums(a, b, nll_s, group_samples=0):
    """float64 [G, 4]: per group of consecutive samples (all S when 0): sum a, sum b, sum nll, group size."""
    n = np.asarray(nll_s, np.float64)
    S = n.shape[0]
    g = group_samples or S
    a = np.zeros(S) if a is None else np.asarray(a, np.float64)
    b = np.zeros(S) if b is None else np.asarray(b, np.float64)
    G = S // g
    return np.stack([a.reshape(G, g).sum(1), b.reshape(G, g).sum(1), n.reshape(G, g).sum(1), np.full(G, float(g))], 1)


# ------------------------------------------------------------------------------------------------------------------ checks
def assert_close(got, want, tol, what=""):
    """|got - want| <= tol elementwise; NaN exactly where the reference is NaN."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    assert np.array_equal(nan_w, nan_g), f"{what}: NaN pattern differs from the reference's (NaN only where a label is bad) at {np.argwhere(nan_g != nan_w)[:8].tolist()}"
    ok = ~nan_w
    err = np.abs(got[ok] - want[ok])
    bad = err > tol[ok]
    if bad.any():
        i = int(np.argmax(err - tol[ok]))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(ok.sum())} outside the bound; worst |err| {err[i]:.3e} "
                             f"vs tol {tol[ok][i]:.3e} (got {got[ok][i]!r}, want {want[ok][i]!r})")
