"""TEST INFRASTRUCTURE: fp64 restatement of the forward statistics -- log q(w), log p(w) under the Gaussian and the
scale-mixture prior, the closed-form KL of the local-reparameterisation layers and its three component sums, the sampled
w, b, y -- with a derived error bound for EVERY returned scalar, the table of regime cells, the reference's own fp32
formula (used to classify a cell, never as the yardstick), an fp32 emulation of the kernels' arithmetic and the seeded
wrong variants the bound has to reject.  numpy / torch-CPU only: imports without a GPU.

What is restated (float64, from the fp32 inputs as given; the prior's scales travel through the ABI as fp32 and are inputs)
----------------------------------------------------------------------------------------------------------------------
per MC sample s, sigma = log1p(exp(rho)), w_s = mu + sigma eps_s over the n = N K + N weights and biases of a layer:
    log q_s = n c0 - sum log sigma - sum eps_s^2 / 2                       c0 = -log sqrt(2 pi)
    log p_s = n (c0 - log sp) - sum w_s^2 / (2 sp^2)                       (Gauss)
            = sum logaddexp(log pi + c0 - log s1 - w^2 / (2 s1^2), log(1 - pi) + c0 - log s2 - w^2 / (2 s2^2))   (mixture)
    y_s     = x W_s^T + b_s
per layer:  ls = sum log sigma,  s2 = sum sigma^2,  m2 = sum mu^2,  KL = (2 n log sp - 2 ls - n + (s2 + m2) / sp^2) / 2.
log q is written with eps, as the kernels form it; the reference forms (w - mu)^2 / (2 sigma^2) from the sampled w, which
in fp32 loses eps altogether once sigma |eps| < u |w| and in fp64 still carries 2^-53 |w| |eps| / sigma per term:
`oracle_lq_slack` is that figure, the one place the comparison with the oracle is wider than 1e-12 relative.

Regime cells
------------
A cell is (prior, rho level, |mu| level): every weight and bias of the launch lies within 2 % of the cell's rho (0.02 absolute
at rho = 0) and of its |mu|, signs mixed, so a layer's sum is a sum of like terms and a slip in one regime cannot hide under
another.  Epsilon rides in the sample dimension: S = 4 with |eps| <= 0, 0.5, 3, 6 (whatever Philox draws on the generator
paths); from rho = 2 on sigma eps dominates the sampled weight and |mu| only seeds it.
  rho     RHO_LEVELS (12, regular)  +  band -100 (sigma a denormal)  +  edges 89 (sigma = +inf), -200 (sigma = 0)
          (89 is drawn from [89, 90.78], the upper half of its neighbourhood: exp overflows from rho = 128 ln 2 = 88.72 on)
  |mu|    0, 1e-4, the mixture's crossover (the two weighted components equal, solved in fp64; sigma1 where there is none),
          0.05, 0.5, 2, 5, 12.5 sigma1 (drawn from [0.98, 1] of it)  +  band 13.6 sigma1  +  edge 15 sigma1
          (sigma_p for sigma1 under a Gauss prior, which has no exponential and is regular at all of them).
  96 regular cells per prior, 2 band cells (rho = -100 at |mu| 0.05; 13.6 sigma1 at rho -8), 3 edge cells (rho 89 and -200 at
  |mu| 0.05; 15 sigma1 at rho -8).  log q, y and the KL are regular in every regular cell.  The log prior is judged per
  SAMPLE by m = max |w_s| / sigma1 (mixtures): m <= 12.5 regular (the bound); 12.5 < m <= 14.3 band (the bound, or -inf: the
  raw exp2 may flush the wide component's denormal density); m >= 14.7 beyond fp32 (exp(c1 - m^2 / 2) < 2^-150 for every
  prior here: non-finite); in between nothing is asserted.  A regular cell's sample 0 (eps = 0) is always regular when
  |mu| <= 12.5 sigma1; sigma1 = e^-1, e^-2 put the levels 2 and 5 themselves into the band or beyond, and large sigma eps
  does the same for any prior -- that is the regime, not a re-tagging: the cell stays regular for everything else.

The bound
---------
u = 2^-24.  A scalar the kernel forms as a sum of n fp32 terms t_i and a double-precision combine obeys, for ANY summation
order (Higham 3.1, first order), |got - ref| <= sum_i delta(t_i) + (n + C_TAIL) u sum |t_i| + 2 u |result|, with C_TAIL = 16
for the constants' roundings and the final cast.  Per term:
  sigma = softplus(rho)   relative (E_SP + A_RHO |rho|) u.  exp2(rho * log2 e): the product's rounding is one u of the ARGUMENT,
                          |rho| u of the result, and the fp32 constant log2 e is off by 0.22 u: A_RHO = 1.25; E_SP is the
                          measured rest.  For rho > 0 the same figure bounds log2(1 + e) ln 2 relative to its value ~ rho.
  log sigma (log q, ls)   d sigma / sigma  +  E_LOG u max(|log sigma|, 1) (v_log_f32 on |log2 sigma|)  +  2 u |log sigma| (ln 2,
                          the fma or product).
  eps^2                   exact input, one fma: in the summation term.
  w = fma(sigma, eps, mu) delta_w = |eps| d sigma + u |w|.   Gauss: w^2 / (2 sp^2) moves by (2 |w| delta_w + delta_w^2) / (2 sp^2).
  sigma^2, mu^2 (KL)      sigma^2 (2 d sigma / sigma + u);  u mu^2;  2^-126 each for a square that underflows (fp32 has no 1e-87).
  mixture term L = log(pi p1 + (1 - pi) p2), p_i = exp(c_i - A_i), A_i = w^2 / (2 s_i^2): the exponent's argument is off by
                          A_i (2 delta_w / |w| + 2 u) + u |c_i| + u |c_i - A_i| (w^2, the fp32 1 / 2 s^2, c_i, the fma), its product
                          with log2 e by A_RHO |arg| u, exp2 by E_EXP u: together d_i, and d_i = 1 where the true p_i is below
                          2^-126 (a flushed denormal; only a band cell can give that a responsibility that matters).  The sum
                          moves by r_1 d_1 + r_2 d_2 + 3 u relative (r_i the responsibilities), the log by E_LOG u max(|L|, 1) +
                          2 u |L| on top.
  KL                      ABSOLUTE: B(ls) + (B(s2) + B(m2)) / (2 sp^2) + 2 u |KL| -- at sigma ~ sigma_p, mu ~ 0 the three sums
                          cancel to ~ 0 and a relative bound on the result would mean nothing.
  y (fp32 math only)      (K + 1 + C_TAIL) u (sum |x| |w| + |b|) + sum |x| delta_w + delta_b.

The hardware constants, measured on an MI355X against fp64 (tests/test_gpu_fwd_stats.py re-measures them and asserts
measured <= constant / 2; each constant is at least twice the measured figure, rounded up to a power of two):
  E_SP   ops.softplus, largest err / (u sigma) - A_RHO |rho| over softplus_probe_points() ([-20, 80]):   2.778, E_SP = 8
         (the error itself is largest at rho = -16.6, 15.4 u; the exactly rounded emulation below gives the same 2.778)
  E_EXP  v_exp_f32: ops.softplus at rho <= -17.5 returns exp2(fl(rho * log2 e)) itself (1 + e rounds to 1, the residue is
         e); against 2^p with p the fp32 product, exact on the CPU:                                      1.257, E_EXP = 4
  E_LOG  v_log_f32 (+ the product with ln 2): ops.gauss_kl on ONE element returns fast_log(sigma) of the sigma that
         ops.softplus returns bit for bit; against log(sigma) in units of u max(|log sigma|, 1):         2.165, E_LOG = 8
Nothing else is tuned on device figures.  The same probe found bnn::softplus itself wrong between the regime levels: it added
the residue e - (fl(1 + e) - 1) undivided at every e -- tens of u wherever 1 + e crosses a binade (rho > 0), 12 % of sigma for
rho in [16.64, 17.33); the residue now stops at e = 1 (emu_softplus(residue_limit=False) keeps the old form as a seeded variant).

What the device does in the bands (recorded from the MI355X; tests/test_gpu_fwd_stats.py prints it): both flush.  rho = -100:
exp2 returns 0 for the denormal, sigma = 0, log q = +inf and the KL = +inf where the reference has log sigma = -100;
|w| = 13.6 sigma1: the wide component's density flushes to 0 and log p = -inf where the reference is finite up to 14.2 sigma1.
The hot path keeps the raw transcendentals; the convention is stated in DESIGN.md and INTEGRATION.md.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

from oracle import bnn_oracle as O

U = 2.0 ** -24
C0 = -0.5 * math.log(2.0 * math.pi)
A_RHO = 1.25
E_SP_MEASURED, E_SP = 2.778, 8.0        # MI355X; the constants are twice the measured figures rounded up to a power of two
E_EXP_MEASURED, E_EXP = 1.257, 4.0
E_LOG_MEASURED, E_LOG = 2.165, 8.0
C_TAIL = 16.0
LN_MIN_NORMAL = -126.0 * math.log(2.0)
MIN_NORMAL = 2.0 ** -126
f32 = np.float32
F64 = np.float64

Prior = collections.namedtuple("Prior", "mixture sigma_p pi sigma1 sigma2")


def _r(v):
    return float(f32(v))


PRIORS = {
    "gauss-0.05": Prior(False, _r(0.05), 0.5, 1.0, 1.0),
    "gauss-1": Prior(False, 1.0, 0.5, 1.0, 1.0),
    "gauss-e": Prior(False, _r(math.e), 0.5, 1.0, 1.0),
    "mix-0.5-0-6": Prior(True, 1.0, 0.5, 1.0, _r(math.exp(-6.0))),
    "mix-0.5-0-8": Prior(True, 1.0, 0.5, 1.0, _r(math.exp(-8.0))),
    "mix-0.25-1-7": Prior(True, 1.0, 0.25, _r(math.exp(-1.0)), _r(math.exp(-7.0))),
    "mix-0.75-2-8": Prior(True, 1.0, 0.75, _r(math.exp(-2.0)), _r(math.exp(-8.0))),
    "mix-equal": Prior(True, 1.0, 0.5, 1.0, 1.0),               # both components N(0, 1): must match gauss-1
    "mix-pi1": Prior(True, 1.0, 1.0, 1.0, _r(math.exp(-6.0))),  # the ABI accepts pi = 1: the wide component alone
}
GAUSS_NAMES = tuple(k for k, p in PRIORS.items() if not p.mixture)
MIX_NAMES = tuple(k for k, p in PRIORS.items() if p.mixture)
NONDEGENERATE_MIX = ("mix-0.5-0-6", "mix-0.5-0-8", "mix-0.25-1-7", "mix-0.75-2-8")
LR_SIGMA_P = {"lr-0.05": _r(0.05), "lr-1": 1.0, "lr-e": _r(math.e)}

RHO_LEVELS = (-20.0, -12.0, -8.0, -5.0, -2.0, 0.0, 0.55, 2.0, 5.0, 15.0, 30.0, 80.0)
RHO_BAND, RHO_EDGES = -100.0, (89.0, -200.0)
MU_BAND, MU_EDGE, MU_TOP = 13.6, 15.0, 12.5                     # in units of sigma1
EPS_SCALES = (0.0, 0.5, 3.0, 6.0)
SIDE_MU, SIDE_RHO = 0.05, -8.0                                  # where the off-grid cells sit in the other coordinate
REG_M, BAND_M, EDGE_M = 12.5, 14.3, 14.7

Cell = collections.namedtuple("Cell", "name prior rho mu tag")  # tag: regular | band | edge


def wide_scale(pr):
    return max(pr.sigma1, pr.sigma2) if pr.mixture else pr.sigma_p


def crossover(pr):
    """|w| at which pi N(w; 0, s1) = (1 - pi) N(w; 0, s2), fp64; sigma1 where the two never meet."""
    if not pr.mixture or pr.pi in (0.0, 1.0) or pr.sigma1 == pr.sigma2:
        return wide_scale(pr)
    a1, a2 = pr.pi / pr.sigma1, (1.0 - pr.pi) / pr.sigma2
    q = 2.0 * math.log(a2 / a1) / (1.0 / pr.sigma2 ** 2 - 1.0 / pr.sigma1 ** 2)
    return math.sqrt(q) if q > 0 else wide_scale(pr)


def mu_levels(pr):
    return (0.0, 1e-4, crossover(pr), 0.05, 0.5, 2.0, 5.0, MU_TOP * wide_scale(pr))


@functools.lru_cache(maxsize=None)
def cells(prior_name):
    pr = PRIORS[prior_name]
    s1 = wide_scale(pr)
    out = [Cell(f"{prior_name}/rho{r:g}/mu{i}", prior_name, r, m, "regular") for r in RHO_LEVELS for i, m in enumerate(mu_levels(pr))]
    out.append(Cell(f"{prior_name}/rho{RHO_BAND:g}/band", prior_name, RHO_BAND, SIDE_MU, "band"))
    out.append(Cell(f"{prior_name}/mu{MU_BAND:g}s/band", prior_name, SIDE_RHO, MU_BAND * s1, "band"))
    out += [Cell(f"{prior_name}/rho{r:g}/edge", prior_name, r, SIDE_MU, "edge") for r in RHO_EDGES]
    out.append(Cell(f"{prior_name}/mu{MU_EDGE:g}s/edge", prior_name, SIDE_RHO, MU_EDGE * s1, "edge"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def lr_cells(name):
    """KL cells of LR_SIGMA_P[name]: the rho x |mu| grid, the cancellation cell (sigma = sigma_p, mu ~ 0), band and edges."""
    sp = LR_SIGMA_P[name]
    pr = Prior(False, sp, 0.5, 1.0, 1.0)
    out = [Cell(f"{name}/rho{r:g}/mu{i}", name, r, m, "regular") for r in RHO_LEVELS for i, m in enumerate(mu_levels(pr))]
    out.append(Cell(f"{name}/cancel", name, math.log(math.expm1(sp)), 1e-4 * sp, "regular"))
    out.append(Cell(f"{name}/rho{RHO_BAND:g}/band", name, RHO_BAND, SIDE_MU, "band"))
    out += [Cell(f"{name}/rho{r:g}/edge", name, r, SIDE_MU, "edge") for r in RHO_EDGES]
    return tuple(out)


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _draw(rs, cell, shape, top):
    rho = cell.rho + max(0.02 * abs(cell.rho), 0.02) * rs.uniform(0 if cell.rho == RHO_EDGES[0] else -1, 1, shape)
    lo, hi = (0.98, 1.0) if top else (0.98, 1.02)
    mu = cell.mu * rs.uniform(lo, hi, shape) * np.where(rs.uniform(size=shape) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray(mu, f32), np.ascontiguousarray(rho, f32)


@functools.lru_cache(maxsize=None)
def cell_params(cell, N, K, lr=False):
    """(w_mu, w_rho, b_mu, b_rho) of a cell, fp32; weights [N, K] (BBB) or [K, N] (`lr`)."""
    rs = _rs(f"{cell.name}/{N}x{K}")
    s1 = wide_scale(PRIORS[cell.prior]) if cell.prior in PRIORS else LR_SIGMA_P[cell.prior]
    top = cell.tag == "regular" and abs(cell.mu - MU_TOP * s1) < 1e-12
    w_mu, w_rho = _draw(rs, cell, (K, N) if lr else (N, K), top)
    b_mu, b_rho = _draw(rs, cell, (N,), top)
    return w_mu, w_rho, b_mu, b_rho


@functools.lru_cache(maxsize=None)
def cell_eps(S, N, K):
    """Injected epsilon: sample s uniform in [-EPS_SCALES[s % 4], +...]; fp32 [S, N, K], [S, N]."""
    rs = _rs(f"eps/{S}/{N}x{K}")
    sc = np.array([EPS_SCALES[s % 4] for s in range(S)])
    return (np.ascontiguousarray(sc[:, None, None] * rs.uniform(-1, 1, (S, N, K)), f32),
            np.ascontiguousarray(sc[:, None] * rs.uniform(-1, 1, (S, N)), f32))


@functools.lru_cache(maxsize=None)
def cell_x(B, K, S=0):
    rs = _rs(f"x/{S}/{B}x{K}")
    return np.ascontiguousarray(rs.uniform(-1, 1, (S, B, K) if S else (B, K)), f32)


# ------------------------------------------------------------------------------------------------------ fp64 restatement
def softplus64(rho):
    return np.logaddexp(0.0, np.asarray(rho, F64))


def rel_sigma(rho):
    return (E_SP + A_RHO * np.abs(rho)) * U


def _sum_bound(terms_abs, per_term, n, result):
    return per_term.sum(-1) + (n + C_TAIL) * U * terms_abs.sum(-1) + 2 * U * np.abs(result)


def _log_sigma_terms(rho):
    """(log sigma, its per-term delta) of fp64 rho."""
    sg = softplus64(rho)
    lg = np.log(sg)
    return sg, lg, rel_sigma(rho) + E_LOG * U * np.maximum(np.abs(lg), 1.0) + 2 * U * np.abs(lg)


def mix_terms(w, dw, pr):
    """Per-weight (L, delta L) of the mixture log density at fp64 w with input error dw."""
    w2 = w * w
    with np.errstate(divide="ignore"):
        lpi = (math.log(pr.pi) if pr.pi > 0 else -np.inf, math.log1p(-pr.pi) if pr.pi < 1 else -np.inf)
    comp, d = [], []
    dw2 = 2 * np.abs(w) * dw + dw * dw
    for s, lp_ in zip((pr.sigma1, pr.sigma2), lpi):
        c = C0 - math.log(s)
        A = w2 / (2.0 * s * s)
        arg = c - A
        di = dw2 / (2.0 * s * s) + 2 * U * A + U * abs(c) + U * np.abs(arg) + (A_RHO * np.abs(arg) + E_EXP) * U
        d.append(np.where(arg <= LN_MIN_NORMAL + 1e-3, 1.0, di))
        comp.append(lp_ + arg)
    L = np.logaddexp(comp[0], comp[1])
    with np.errstate(invalid="ignore"):
        r1, r2 = np.exp(comp[0] - L), np.exp(comp[1] - L)
    rel = r1 * d[0] + r2 * d[1] + 3 * U
    return L, rel + E_LOG * U * np.maximum(np.abs(L), 1.0) + 2 * U * np.abs(L)


Stats = collections.namedtuple("Stats", "log_q log_prior y b_log_q b_log_prior b_y m w bias")
Flat = collections.namedtuple("Flat", "log_q log_prior b_log_q b_log_prior m w dw")


def stats_ref(mu, rho, eps, pr, sigma=None):
    """fp64 (log q, log p) [S] over the flat parameters mu, rho [n] with eps [S, n], and their bounds.  `sigma` (fp32, as an
    INPUT: a kernel that is handed sigma, e.g. the sparse step's sigma_val): used as is, without softplus's error."""
    mu, eps = np.asarray(mu, F64).ravel(), np.asarray(eps, F64)
    n = mu.size
    if sigma is None:
        rho = np.asarray(rho, F64).ravel()
        sg, lg, dlg = _log_sigma_terms(rho)
        rs = rel_sigma(rho)
    else:
        sg = np.asarray(sigma, F64).ravel()
        lg = np.log(sg)
        rs = np.zeros(n)
        dlg = E_LOG * U * np.maximum(np.abs(lg), 1.0) + 2 * U * np.abs(lg)
    ls, e2 = lg.sum(), (eps * eps).sum(1)
    log_q = n * C0 - ls - 0.5 * e2
    b_ls = dlg.sum() + (n + C_TAIL) * U * np.abs(lg).sum()
    b_lq = b_ls + 0.5 * (n + C_TAIL) * U * e2 + 2 * U * np.abs(log_q)
    w = mu + sg * eps
    dw = np.abs(eps) * rs * sg + U * np.abs(w)
    if pr.mixture:
        L, dL = mix_terms(w, dw, pr)
        log_p = L.sum(1)
        b_lp = _sum_bound(np.abs(L), dL, n, log_p)
    else:
        iv = 1.0 / (2.0 * pr.sigma_p ** 2)
        a = (w * w).sum(1)
        log_p = n * (C0 - math.log(pr.sigma_p)) - a * iv
        b_lp = ((2 * np.abs(w) * dw + dw * dw).sum(1) + (n + C_TAIL) * U * a) * iv + 2 * U * (np.abs(log_p) + a * iv)
    m = np.abs(w).max(1) / wide_scale(pr) if n else np.zeros(eps.shape[0])
    return Flat(log_q, log_p, b_lq, b_lp, m, w, dw)


def bbb_ref(x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, pr):
    """fp64 statistics of one launch and their bounds.  w_mu [N, K], eps_w [S, N, K], eps_b [S, N]; x [B, K] or [S, B, K].
    Returns Stats: log_q [S], log_prior [S], y [S, B, N], the bounds, m [S] = max |w_s| / (the prior's wide scale)."""
    x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b = (np.asarray(a, F64) for a in (x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b))
    S = eps_w.shape[0]
    N, K = w_mu.shape
    f = stats_ref(np.concatenate([w_mu.ravel(), b_mu]), np.concatenate([w_rho.ravel(), b_rho]),
                  np.concatenate([eps_w.reshape(S, -1), eps_b.reshape(S, -1)], 1), pr)
    W, bias = f.w[:, :N * K].reshape(S, N, K), f.w[:, N * K:]
    dW, db = f.dw[:, :N * K].reshape(S, N, K), f.dw[:, N * K:]
    x3 = x if x.ndim == 3 else np.broadcast_to(x, (S,) + x.shape)
    y = np.einsum("sbk,snk->sbn", x3, W) + bias[:, None, :]
    ax = np.abs(x3)
    b_y = (K + 1 + C_TAIL) * U * (np.einsum("sbk,snk->sbn", ax, np.abs(W)) + np.abs(bias)[:, None, :]) \
        + np.einsum("sbk,snk->sbn", ax, dW) + db[:, None, :]
    return Stats(f.log_q, f.log_prior, y, f.b_log_q, f.b_log_prior, b_y, f.m, W, bias)


def oracle_lq_slack(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b):
    """The fp64 oracle's own error in log q, per sample: it forms (w - mu)^2 / (2 sigma^2) from w = mu + sigma eps, so each
    term carries 4 * 2^-53 |w| |eps| / sigma."""
    mu = np.concatenate([np.asarray(w_mu, F64).ravel(), np.asarray(b_mu, F64)])
    rho = np.concatenate([np.asarray(w_rho, F64).ravel(), np.asarray(b_rho, F64)])
    S = eps_w.shape[0]
    eps = np.concatenate([np.asarray(eps_w, F64).reshape(S, -1), np.asarray(eps_b, F64).reshape(S, -1)], 1)
    sg = softplus64(rho)
    return (4 * 2.0 ** -53 * np.abs(mu + sg * eps) * np.abs(eps) / sg).sum(1)


Kl = collections.namedtuple("Kl", "value bound")     # each: (kl, ls, s2, m2)


def kl_ref(mu, rho, sigma_p):
    """fp64 (KL, sum log sigma, sum sigma^2, sum mu^2) over the flat (mu, rho) and an absolute bound for each."""
    mu, rho = np.asarray(mu, F64).ravel(), np.asarray(rho, F64).ravel()
    n = mu.size
    sg, lg, dlg = _log_sigma_terms(rho)
    ls, s2, m2 = lg.sum(), (sg * sg).sum(), (mu * mu).sum()
    b_ls = dlg.sum() + (n + C_TAIL) * U * np.abs(lg).sum() + 2 * U * abs(ls)
    b_s2 = (sg * sg * (2 * rel_sigma(rho) + U)).sum() + (n + C_TAIL + 2) * U * s2 + n * MIN_NORMAL
    b_m2 = (n + C_TAIL + 3) * U * m2 + n * MIN_NORMAL
    sp2 = sigma_p * sigma_p
    kl = 0.5 * (2 * n * math.log(sigma_p) - 2 * ls - n + (s2 + m2) / sp2)
    b_kl = b_ls + 0.5 * (b_s2 + b_m2) / sp2 + 2 * U * abs(kl)
    return Kl((kl, ls, s2, m2), (b_kl, b_ls, b_s2, b_m2))


# ------------------------------------------------------------------------------ the reference's own formula, fp32 torch
def reference_fp32(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, pr):
    """(log_q [S], log_prior [S]) as the reference's modules compute them in float32 on the CPU: sigma = log1p(exp(rho)),
    w = mu + sigma * eps, GaussianNode.log_prob = sum(c0 - log sigma - (w - mu)^2 / (2 sigma^2)), the prior through
    torch.distributions.Normal and, for the mixture, log(pi exp(lp1) + (1 - pi) exp(lp2))."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32))
    lq, lp = [], []
    for s in range(eps_w.shape[0]):
        ql, pl = 0.0, 0.0
        for mu, rho, eps in ((t(w_mu), t(w_rho), t(eps_w[s])), (t(b_mu), t(b_rho), t(eps_b[s]))):
            sigma = torch.log1p(torch.exp(rho))
            w = mu + sigma * eps
            ql = ql + (-math.log(math.sqrt(2 * math.pi)) - torch.log(sigma) - ((w - mu) ** 2) / (2 * sigma ** 2)).sum()
            if pr.mixture:
                p1 = torch.exp(torch.distributions.Normal(0.0, pr.sigma1, validate_args=False).log_prob(w))
                p2 = torch.exp(torch.distributions.Normal(0.0, pr.sigma2, validate_args=False).log_prob(w))
                pl = pl + torch.log(pr.pi * p1 + (1 - pr.pi) * p2).sum()
            else:
                pl = pl + torch.distributions.Normal(0.0, pr.sigma_p, validate_args=False).log_prob(w).sum()
        lq.append(float(ql))
        lp.append(float(pl))
    return np.array(lq), np.array(lp)


def reference_slack(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, pr):
    """(log q, log p) [S]: what the reference's fp32 formula loses ON TOP of the kernels' bound, by its own construction.
    log q: it re-derives eps from w - mu, per term 2 u (|w| + |mu|) |eps| / sigma (the whole eps^2 / 2 once w == mu in fp32), and
    its quotient by 2 sigma^2 costs 6 u eps^2 / 2.  Both: it carries the constants c0 (- log sigma_p) inside every term of an
    fp32 sum, (n + C_TAIL) u n |c|, where the kernels add n c in double.  Not part of the kernels' bound."""
    mu = np.concatenate([np.asarray(w_mu, F64).ravel(), np.asarray(b_mu, F64)])
    rho = np.concatenate([np.asarray(w_rho, F64).ravel(), np.asarray(b_rho, F64)])
    S = eps_w.shape[0]
    eps = np.concatenate([np.asarray(eps_w, F64).reshape(S, -1), np.asarray(eps_b, F64).reshape(S, -1)], 1)
    n = mu.size
    sg = softplus64(rho)
    aw = np.abs(mu + sg * eps) + np.abs(mu)
    d = 2 * U * aw / sg
    lq = (np.abs(eps) * d + 0.5 * d * d).sum(1) + (6 * U * eps * eps).sum(1) + (n + C_TAIL) * U * n * abs(C0)
    lp = np.zeros(S) if pr.mixture else np.full(S, (n + C_TAIL) * U * n * abs(C0 - math.log(pr.sigma_p)))
    return lq, lp


def reference_kl_fp32(mu, rho, sigma_p):
    """compute_kl_cost semantics in float32: 0.5 * sum(2 log(sp / sigma) - 1 + (sigma / sp)^2 + (mu / sp)^2)."""
    mu, rho = torch.from_numpy(np.ascontiguousarray(mu, f32)).ravel(), torch.from_numpy(np.ascontiguousarray(rho, f32)).ravel()
    sigma = torch.log1p(torch.exp(rho))
    return float(0.5 * (2 * torch.log(sigma_p / sigma) - 1 + (sigma / sigma_p).pow(2) + ((0.0 - mu) / sigma_p).pow(2)).sum())


# ----------------------------------------------------------------- fp32 emulation of the kernels' arithmetic, and variants
LOG2E_F, LN2_F = f32(1.442695040888963407), f32(0.693147180559945309)
VARIANTS = ("softplus_no_residue", "mix_no_inv_sigma", "mix_drop_narrow", "kl_sigma2_bf16", "kl_fp32_combine", "logq_sigma_bf16")


def _fma(a, b, c):
    return (a.astype(F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(f32)


def _exp2(p, flush):
    with np.errstate(over="ignore", under="ignore"):
        r = np.exp2(p.astype(F64)).astype(f32)
    return np.where(np.abs(r) < MIN_NORMAL, f32(0), r) if flush else r


def _log2(v, flush):
    v = np.where(np.abs(v) < MIN_NORMAL, f32(0), v) if flush else v
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log2(v.astype(F64)).astype(f32)


def _bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v, f32)).to(torch.bfloat16).to(torch.float32).numpy()


def emu_softplus(rho, flush=False, residue=True, residue_limit=True):
    """bnn::softplus of csrc/bnn_device.h: log2(fl(1 + e)) ln 2 + the residue e - (fl(1 + e) - 1) while e < 1.
    `residue_limit` False: the residue added at every e, as the kernels did before this module existed -- half an ulp of
    1 + e wherever that crosses a binade (46 u at rho ~ 5.5), 0 or +-2 for e in [2^24, 2^25), i.e. sigma off by up to 12 % for
    rho in [16.64, 17.33).  The regime cells' sums barely see it; the probe of E_SP does."""
    rho = np.asarray(rho, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = _exp2(rho * LOG2E_F, flush)
        u = f32(1) + e
        d = u - f32(1)
        r = np.where(e < f32(1), e - d, f32(0)) if residue_limit else np.where(e > f32(3.0e38), f32(0), e - d)
        s = _fma(_log2(u, flush), LN2_F, r if residue else np.zeros_like(e))
    return s


def _seq(terms):
    """Plain left-to-right fp32 accumulation along the last axis."""
    return np.cumsum(terms.astype(f32), axis=-1, dtype=f32)[..., -1].astype(F64)


def emu_bbb(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, pr, flush=False, variant=None):
    """(log_q [S], log_prior [S]) as the kernels form them: fp32 terms and partial sums, exact exp2 / log2 rounded to fp32
    (`flush`: denormal results and arguments as zero), the combine of bbb_layer_scalars_kernel in double."""
    S = eps_w.shape[0]
    mu = np.concatenate([np.asarray(w_mu, f32).ravel(), np.asarray(b_mu, f32)])
    rho = np.concatenate([np.asarray(w_rho, f32).ravel(), np.asarray(b_rho, f32)])
    eps = np.concatenate([np.asarray(eps_w, f32).reshape(S, -1), np.asarray(eps_b, f32).reshape(S, -1)], 1)
    n = mu.size
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sg = emu_softplus(rho, flush, residue=variant != "softplus_no_residue")
        sg_l = _bf16(sg) if variant == "logq_sigma_bf16" else sg
        ls = _seq(_log2(sg_l, flush) * LN2_F)
        e2 = _seq(eps * eps)
        log_q = n * C0 - ls - 0.5 * e2
        w = _fma(sg[None], eps, mu[None])
        if pr.mixture:
            c, iv = [], []
            for s in (pr.sigma1, pr.sigma2):
                c.append(f32(C0 - (0.0 if variant == "mix_no_inv_sigma" else math.log(s))))
                iv.append(f32(1.0 / (2.0 * s * s)))
            w2 = w * w
            p1 = _exp2(_fma(-w2, iv[0], c[0]) * LOG2E_F, flush)
            p2 = _exp2(_fma(-w2, iv[1], c[1]) * LOG2E_F, flush)
            narrow = 1 if pr.sigma2 <= pr.sigma1 else 0
            if variant == "mix_drop_narrow":
                p1, p2 = (p1, np.zeros_like(p2)) if narrow == 1 else (np.zeros_like(p1), p2)
            mix = _fma(np.full_like(p1, f32(pr.pi)), p1, (f32(1) - f32(pr.pi)) * p2)
            log_p = _seq(_log2(mix, flush) * LN2_F)
        else:
            a = _seq(w * w)
            log_p = n * (C0 - math.log(pr.sigma_p)) - a / (2.0 * pr.sigma_p * pr.sigma_p)
    return log_q, log_p


def emu_kl(mu, rho, sigma_p, flush=False, variant=None):
    """(kl, ls, s2, m2) as gauss_kl / the LR layers form them: fp32 sums, the combine in double."""
    mu, rho = np.asarray(mu, f32).ravel(), np.asarray(rho, f32).ravel()
    n = mu.size
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sg = emu_softplus(rho, flush, residue=variant != "softplus_no_residue")
        ls = _seq(_log2(_bf16(sg) if variant == "logq_sigma_bf16" else sg, flush) * LN2_F)
        sq = sg * sg
        s2 = _seq(_bf16(sq) if variant == "kl_sigma2_bf16" else sq)
        m2 = _seq(mu * mu)
        if variant == "kl_fp32_combine":
            sp, cnt = f32(sigma_p), f32(n)
            kl = float(f32(0.5) * ((f32(2) * cnt * f32(math.log(sigma_p)) - f32(2) * f32(ls)) - cnt + (f32(s2) + f32(m2)) / (sp * sp)))
        else:
            kl = 0.5 * (2.0 * n * math.log(sigma_p) - 2.0 * ls - n + (s2 + m2) / (sigma_p * sigma_p))
    return kl, ls, s2, m2


# -------------------------------------------------------------------------------------------- judging a launch's results
def share(got, ref, bound):
    """Largest |got - ref| / bound (0 / 0 counts as 0; a NaN, or an error over a zero bound, as inf)."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        sh = np.where(err == 0, 0.0, err / bound)
    sh = np.where(np.isnan(sh), np.inf, sh)
    return float(sh.max()) if sh.size else 0.0


def prior_sample_tags(pr, m):
    """Per sample: 'regular' | 'band' | 'beyond' | 'open' for the log prior, from m = max |w_s| / sigma1."""
    if not pr.mixture:
        return ["regular"] * len(m)
    return ["regular" if v <= REG_M else "band" if v <= BAND_M else "beyond" if v >= EDGE_M else "open" for v in m]


# ------------------------------------------------------------------------------------------------- measuring the constants
def softplus_probe_points():
    """rho at which E_SP is measured: 4096 evenly spaced in [-20, 80], the levels and the ends of their 2 % neighbourhoods."""
    pts = [np.linspace(-20.0, 80.0, 4096)]
    for r in RHO_LEVELS:
        h = max(0.02 * abs(r), 0.02)
        pts.append(np.array([r - h, r, r + h]))
    return np.clip(np.concatenate(pts), -20.4, 81.6).astype(f32)


def softplus_rest_in_u(got, rho):
    """Largest |got - log1p(exp(rho))| / (u sigma) - A_RHO |rho|."""
    want = softplus64(rho)
    return float(np.max(np.abs(got.astype(F64) - want) / (U * want) - A_RHO * np.abs(rho.astype(F64))))


def exp_probe_points():
    return np.linspace(-87.0, -17.5, 4096).astype(f32)


def exp_error_in_u(got, rho):
    """got = ops.softplus(rho) at rho <= -17.5: exp2(p) with p = fl(rho * log2 e); relative error against 2^p, in u."""
    p = (rho.astype(f32) * LOG2E_F).astype(F64)
    want = np.exp2(p)
    return float(np.max(np.abs(got.astype(F64) - want) / (U * want)))


def log_probe_points():
    """rho whose sigma spans [2e-9, 80], densely around sigma = 1 (rho = log(e - 1)), where log2 sigma passes through 0."""
    r1 = math.log(math.e - 1.0)
    return np.concatenate([np.linspace(-20.0, 80.0, 160), r1 + np.linspace(-0.05, 0.05, 64), r1 + np.linspace(-1e-4, 1e-4, 32)]).astype(f32)


def log_error_in_u(got, sigma):
    """got = fast_log(sigma) on the device for the fp32 sigma given; error against log(sigma) in u max(|log sigma|, 1)."""
    want = np.log(sigma.astype(F64))
    return float(np.max(np.abs(got.astype(F64) - want) / (U * np.maximum(np.abs(want), 1.0))))
