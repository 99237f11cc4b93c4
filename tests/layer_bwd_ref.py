"""TEST INFRASTRUCTURE: fp64 restatement of the layer backward (bnn_bbb_linear_bwd, bnn_lr_linear_bwd; SURVEY Appendix
A.5 and the header comments of csrc/bbb_bwd.hip, csrc/lr_bwd.hip) with a derived error bound for EVERY output element, the
shared table of cases and inputs, and the seeded wrong variants the bound has to reject.  torch-CPU only: imports
without a GPU.  tests/tensor_op_grads.py stays the fp32-on-device cross-check; this module is the independent reference.

What is restated
----------------
BBB ([out, in] weights), per MC sample s with gz_s = gy_s * (y_s > 0), w_s = mu + sigma * eps_s, sigma = softplus(rho):
    t_s   = gz_s^T x_s + glp_s * dlogp(w_s)
    g_mu  = sum_s t_s                 g_rho = (sum_s t_s eps_s - (sum_s glq_s) / sigma) * sigmoid(rho)
    g_x_s = gz_s w_s  [* (x_s > 0)]   (bias: column sums of gz_s in place of gz_s^T x_s)
LR ([in, out] weights), h_s = gz_s eps_act_s / (2 sqrt(v_s)) (0 where v == 0) or gz_s * hfac_s:
    g_M   = sum_s x_s^T gz_s + c_w M / sp^2          g_sigma = 2 sigma sum_s (x_s^2)^T h_s + c_w (sigma / sp^2 - 1 / sigma)
    g_rho = g_sigma * sigmoid(rho)                   g_x_s   = gz_s M^T + 2 x_s (h_s (sigma^2)^T)  [* (x_s > 0)]
y, v and hfac are INPUTS: no mask and no variance depends on a forward run, so no element is ever excluded.
bf16 math (`bf16=True`) applies the kernels' rounding points to the input gradient only: BBB rounds gz and w_s (the
w_sampled tensor as passed, or bf16(fl32(mu + sigma eps)) on the generator path); LR rounds gz, M, h, sigma^2.  Products of
two bf16 numbers are exact in fp32 and accumulation is fp32, so the sums stay in fp64 here.

The bound
---------
u = 2^-24 is the unit roundoff of fp32 round-to-nearest.  An output element the kernel forms as a sum of n fp32 terms
t_i followed by a few elementwise operations obeys (Higham, Accuracy and Stability, 3.1, to first order in u, ANY
summation order -- which is why the MFMA tile order, the LDS exchanges and the K split do not matter)

    |got - ref| <= (n + C_TAIL) * u * sum_i |t_i|  +  P.

  * sum |t_i| is the same formula on absolute values, in fp64.  n = S B + S (BBB weights: S B products, S prior terms),
    S B (+ S) (bias), N (BBB g_x), S B + 1 (LR weights), 2 N (LR g_x).
  * C_TAIL = 16 covers the elementwise tail: rounding of the host constants (1 / sigma_p^2, a_i, ...), of c_q and c_w
    (sums of <= 3 upstream scalars), the fma / multiply / subtract of the epilogue, x^2, 2 sigma: fewer than 16 roundings
    in every kernel, each relative to a term that is in sum |t_i|.
  * P is the first-order propagation |d term / d q| * delta_q of every quantity q the kernel RE-CREATES on chip:
      sigma = softplus(rho)   delta = (E_T + |rho|) u sigma.  exp2(rho * log2 e): forming the product costs up to one ulp OF
                              THE ARGUMENT, i.e. |rho| ulp of the result (d exp(a) = exp(a) da); E_T is the measured rest
                              (exp2, log2, the compensated sum).
      sigmoid(rho)            the same relative figure (the argument error of exp(-rho) is damped by 1 - sigmoid <= 1).
      1 / sigma               (E_T + |rho| + 1) u / sigma   (v_rcp_f32: one ulp).
      w_s = fma(sigma, eps, mu)   delta_w = |eps| delta_sigma + u |w|.   eps itself is exact: bit-pinned to the device.
      dlogp(w)                Gaussian -w / sp^2: delta_w / sp^2.  Mixture g(w) = -w r(w), r = p1 / s1^2 + p2 / s2^2 with the
                              responsibilities p_i = n_i / (n1 + n2), n_i = a_i exp(-A_i), A_i = w^2 / (2 s_i^2):
                                |g'(w)| delta_w,  g' = -r + w^2 (1/s1^2 - 1/s2^2)^2 p1 p2   (the curvature: 1 / s2^2 = 1.6e5
                                near w = 0) plus the evaluation error: a relative error d_i of n_i moves r by
                                (1/s1^2 - 1/s2^2) p1 p2 (d_1 - d_2), and d_i = (5 A_i + E_T + 2) u (five roundings on the
                                way to the exponent's argument -- w^2, 1 / 2 s^2, the product, log2 e, its product -- each
                                worth A_i u; the exp2 unit; a_i and its product).
      LR's h                  three roundings (product, sqrt, quotient; division and square root are correctly rounded):
                              3 u |h|; one (the product gz * hfac) from the saved factor.
      LR's sigma^2            (2 (E_T + |rho|) + 1) u sigma^2.
  * bf16 math: a re-created operand q (w_s on the generator path, LR's h and sigma^2) is rounded to bf16 AFTER its fp32
    error delta_q.  If bf16(q - delta_q) == bf16(q + delta_q) the kernel's operand is that value exactly and the rounding
    adds nothing; otherwise q lies within delta_q of a rounding tie, either neighbour is legitimate, and the element's
    bound grows by |other operand| * |bf16(q + delta_q) - bf16(q - delta_q)| (one bf16 ulp) -- for exactly those
    operands and no others.  `info["tie_share"]` is their share; the CPU test holds it below 1 %.  Inputs that are
    rounded (gz, M, a passed w_sampled) are exact.

E_T is the one measured constant: the largest relative error of ops.softplus on the MI355X against fp64 log1p(exp(rho))
in units of u, over 4096 evenly spaced rho in [-12, 2] and the fp32 neighbours of the cases' rho end points.  The
constant is twice the measured figure rounded up to a power of two; the factor two covers sigmoid and dlogp, which use the
same one-ulp-class units (v_rcp, v_exp) but are not sampled directly.  tests/test_gpu_layer_bwd.py repeats the
measurement and asserts measured <= E_T / 2.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

from oracle import bnn_oracle as O

U = 2.0 ** -24
E_T_MEASURED = 14.953    # MI355X, largest |softplus - log1p(exp)| / (u * log1p(exp)) over softplus_probe_points()
E_T = 32.0              # 2 * E_T_MEASURED rounded up to a power of two
C_TAIL = 16.0
H_ROUNDINGS = 3.0       # product, sqrt, quotient
F64 = torch.float64

Prior = collections.namedtuple("Prior", "mixture sigma_p pi sigma1 sigma2")
MIX = Prior(True, 1.0, 0.5, 1.0, math.exp(-6.0))
GAUSS = Prior(False, 0.8, 0.5, 1.0, 1.0)
RHO_RANGES = {"cfg": (-5.0, -4.0), "wide": (-12.0, 2.0)}
SEED, LAYER_ID, SAMPLE_OFFSET = 0x1234ABCD5678EF01, 2, 40

Result = collections.namedtuple("Result", "grads bounds info")     # grads / bounds: (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x)
NAMES = ("g_w_mu", "g_w_rho", "g_b_mu", "g_b_rho", "g_x")


# ------------------------------------------------------------------------------------------------------------ pieces
def _t(a, dt):
    if a is None:
        return None
    a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return a.detach().cpu().to(dt)


def softplus(rho):
    return torch.log1p(torch.exp(rho))


def bf16r(t):
    """fp32 -> bf16 round-to-nearest-even of fl32(t), as (__bf16)float on the device."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def bf16_tie(q, delta):
    """bf16(q) and the slack |bf16(q + delta) - bf16(q - delta)|: zero unless q is within delta of a rounding tie."""
    return bf16r(q), (bf16r(q + delta) - bf16r(q - delta)).abs()


def rel_sigma(rho):
    return (E_T + rho.abs()) * U


def _mix(w, pr, swap=False):
    a1, a2 = pr.pi / pr.sigma1, (1.0 - pr.pi) / pr.sigma2
    if swap:
        a1, a2 = a2, a1
    iv1, iv2 = 1.0 / pr.sigma1 ** 2, 1.0 / pr.sigma2 ** 2
    A1, A2 = w * w * (0.5 * iv1), w * w * (0.5 * iv2)
    d = (math.log(a2) - A2) - (math.log(a1) - A1)
    p2 = torch.sigmoid(d)
    p1 = torch.sigmoid(-d)
    return iv1, iv2, A1, A2, p1, p2


def dlogp(w, pr, swap=False):
    if not pr.mixture:
        return -w / pr.sigma_p ** 2
    iv1, iv2, _, _, p1, p2 = _mix(w, pr, swap)
    return -w * (p1 * iv1 + p2 * iv2)


def dlogp_err(w, dw, pr):
    """delta of dlogp(w) beyond the roundings C_TAIL counts: propagation of delta_w and the mixture's evaluation."""
    if not pr.mixture:
        return dw / pr.sigma_p ** 2
    iv1, iv2, A1, A2, p1, p2 = _mix(w, pr)
    gp = (p1 * iv1 + p2 * iv2) + w * w * (iv1 - iv2) ** 2 * p1 * p2
    ev = w.abs() * abs(iv1 - iv2) * p1 * p2 * ((5 * A1 + E_T + 2) + (5 * A2 + E_T + 2)) * U
    return gp * dw + ev


def _x3(x, S):
    return x if x.dim() == 3 else x.unsqueeze(0).expand(S, -1, -1)


def _mask(gy, y, relu, variant):
    if not relu:
        return gy
    return gy * ((y >= 0) if variant == "mask_ge" else (y > 0)).to(gy.dtype)


def _clamped_outputs(g, variant, w_out_axis):
    """Seeded output variants: the last k column / last feature computed from its clamped neighbour's data."""
    g = [t.clone() for t in g]
    w_in_axis = 1 - w_out_axis
    if variant == "clamp_last_k":
        for t in g[:2]:
            t.select(w_in_axis, -1).copy_(t.select(w_in_axis, -2).clone())
        g[4][..., -1] = g[4][..., -2]
    elif variant == "clamp_last_feature":
        for t in g[:2]:
            t.select(w_out_axis, -1).copy_(t.select(w_out_axis, -2).clone())
        g[2][-1], g[3][-1] = g[2][-2].clone(), g[3][-2].clone()
    return tuple(g)


# ------------------------------------------------------------------------------------------------------------ BBB
def bbb_ref(x, gy, y, w_mu, w_rho, b_mu, b_rho, *, prior, relu, eps_w, eps_b, g_log_prior=None, g_log_q=None,
            gx_relu_mask=False, w_sampled=None, bf16=False, dtype=F64, variant=None, want_bound=True):
    """Gradients (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x[S, B, K]) of one bnn_bbb_linear_bwd launch and their bounds.
    eps_w [S, N, K], eps_b [S, N]: the epsilon of the launch's samples (philox_eps_bbb, or the BNN_EPS_MEMORY arrays)."""
    dt = dtype
    x, gy, y, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, glp, glq, w_sampled = (
        _t(a, dt) for a in (x, gy, y, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, g_log_prior, g_log_q, w_sampled))
    S, B, N = gy.shape
    x3 = _x3(x, S)
    gz = _mask(gy, y, relu, variant)
    if variant == "drop_last_row":
        gz = gz.clone()
        gz[:, -1] = 0
    zS = torch.zeros(S, dtype=dt)
    glp_ = glp if glp is not None else zS
    glq_ = glq if glq is not None else zS
    sw, sb = softplus(w_rho), softplus(b_rho)
    W, bv = w_mu + sw * eps_w, b_mu + sb * eps_b                                   # [S, N, K], [S, N]
    swap = variant == "mix_swapped"
    dW = dlogp(w_mu.expand_as(W) if variant == "prior_at_mu" else W, prior, swap)
    db = dlogp(b_mu.expand_as(bv) if variant == "prior_at_mu" else bv, prior, swap)
    tW = torch.einsum("sbn,sbk->snk", gz, x3) + glp_.view(S, 1, 1) * dW
    tb = gz.sum(1) + glp_.view(S, 1) * db
    cq = glq_.sum()
    sig_w, sig_b = torch.sigmoid(w_rho), torch.sigmoid(b_rho)
    g_wmu, g_bmu = tW.sum(0), tb.sum(0)
    g_wrho = ((tW * eps_w).sum(0) - cq / sw) * sig_w
    g_brho = ((tb * eps_b).sum(0) - (0.0 if variant == "bias_no_q" else cq) / sb) * sig_b
    # ---- input gradient
    if bf16:
        gzr = gz if variant == "gz_not_rounded" else bf16r(gz)
        Wr = w_sampled if w_sampled is not None else bf16r(W)
    else:
        gzr, Wr = gz, W
    gxm = (x3 > 0).to(dt) if gx_relu_mask else torch.ones((), dtype=dt)
    g_x = torch.einsum("sbn,snk->sbk", gzr, Wr) * gxm
    grads = _clamped_outputs((g_wmu, g_wrho, g_bmu, g_brho, g_x), variant, 0)
    if not want_bound:
        return Result(grads, None, {})

    def param_bounds(absdata, rho, sg, sig, mu, eps, g_rho, nterms):
        """absdata [S, ...]: sum_b |x| |gz| (or |gz|) per sample; returns the bounds of (g_mu, g_rho)."""
        rs = rel_sigma(rho)
        w = mu + sg * eps
        dw = eps.abs() * rs * sg + U * w.abs()
        dg = dlogp_err(w, dw, prior)
        shp = (S,) + (1,) * (w.dim() - 1)
        a_lp = glp_.abs().view(shp)
        at = absdata + a_lp * dlogp(w, prior).abs()
        b_mu_ = (nterms + C_TAIL) * U * at.sum(0) + (a_lp * dg).sum(0)
        A = sig * ((at * eps.abs()).sum(0) + glq_.abs().sum() / sg)
        P = sig * ((a_lp * dg * eps.abs()).sum(0) + cq.abs() * (rs + U) / sg) + rs * g_rho.abs()
        return b_mu_, (nterms + C_TAIL) * U * A + P

    agz = gz.abs()
    bw_mu, bw_rho = param_bounds(torch.einsum("sbn,sbk->snk", agz, x3.abs()), w_rho, sw, sig_w, w_mu, eps_w, g_wrho, S * B + S)
    bb_mu, bb_rho = param_bounds(agz.sum(1), b_rho, sb, sig_b, b_mu, eps_b, g_brho, S * B + S)
    info = {"tie_share": 0.0, "inside_3sigma2": float((W.abs() < 3 * prior.sigma2).double().mean()) if prior.mixture else 0.0}
    dWs = eps_w.abs() * rel_sigma(w_rho) * sw + U * W.abs()
    if bf16:
        slack = torch.zeros_like(W)
        if w_sampled is None:
            _, slack = bf16_tie(W, dWs)
            info["tie_share"] = float((slack > 0).double().mean())
        b_x = (N + C_TAIL) * U * torch.einsum("sbn,snk->sbk", gzr.abs(), Wr.abs()) + torch.einsum("sbn,snk->sbk", gzr.abs(), slack)
    else:
        b_x = (N + C_TAIL) * U * torch.einsum("sbn,snk->sbk", agz, W.abs()) + torch.einsum("sbn,snk->sbk", agz, dWs)
    return Result(grads, (bw_mu, bw_rho, bb_mu, bb_rho, b_x * gxm), info)


# ------------------------------------------------------------------------------------------------------------ LR
def lr_ref(x, gy, y, v, w_mu, w_rho, b_mu, b_rho, *, sigma_p, relu, eps_act, eps_b, g_kl=None, hfac=None, gx_relu_mask=False,
           bf16=False, dtype=F64, variant=None, want_bound=True):
    """Gradients (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x[S, B, K]) of one bnn_lr_linear_bwd launch and their bounds.
    `v` or (`hfac` with relu False: the launch without preparation); eps_act [S, B, N] (unused with hfac), eps_b [S, N]."""
    dt = dtype
    x, gy, y, v, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b, gkl, hfac = (
        _t(a, dt) for a in (x, gy, y, v, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b, g_kl, hfac))
    S, B, N = gy.shape
    x3 = _x3(x, S)
    gz = _mask(gy, y, relu, variant)
    if variant == "drop_last_row":
        gz = gz.clone()
        gz[:, -1] = 0
    factor = hfac is not None and not relu
    if factor:
        h, h_rel = gz * hfac, U
    else:
        sd = torch.sqrt(v)
        raw = gz * eps_act / (2 * sd)
        h = raw if variant == "h_unguarded" else torch.where(sd > 0, raw, torch.zeros_like(raw))
        h_rel = H_ROUNDINGS * U
    sw, sb = softplus(w_rho), softplus(b_rho)
    s2 = sw * sw
    xsq = x3 * x3
    sp2 = sigma_p ** 2
    cw = (gkl[0] + gkl[1]) if gkl is not None else torch.zeros((), dtype=dt)
    cb = (gkl[0] + gkl[2]) if gkl is not None else torch.zeros((), dtype=dt)
    gS = torch.einsum("sbk,sbn->kn", xsq, h)
    two = 1.0 if variant == "no_factor_2" else 2.0
    sig_w, sig_b = torch.sigmoid(w_rho), torch.sigmoid(b_rho)
    g_wmu = torch.einsum("sbk,sbn->kn", x3, gz) + cw * w_mu / sp2
    g_wrho = (two * sw * gS + cw * (sw / sp2 - 1 / sw)) * sig_w
    gsum = gz.sum(1)                                                               # [S, N]
    g_bmu = gsum.sum(0) + cb * b_mu / sp2
    g_brho = ((gsum * eps_b).sum(0) + cb * (sb / sp2 - (0.0 if variant == "bias_no_q" else 1.0) / sb)) * sig_b
    # ---- input gradient
    if bf16:
        gzr = gz if variant == "gz_not_rounded" else bf16r(gz)
        Mr, hr, s2r = bf16r(w_mu), bf16r(h), bf16r(s2)
    else:
        gzr, Mr, hr, s2r = gz, w_mu, h, s2
    gxm = (x3 > 0).to(dt) if gx_relu_mask else torch.ones((), dtype=dt)
    g_x = (torch.einsum("sbn,kn->sbk", gzr, Mr) + 2 * x3 * torch.einsum("sbn,kn->sbk", hr, s2r)) * gxm
    grads = _clamped_outputs((g_wmu, g_wrho, g_bmu, g_brho, g_x), variant, 1)
    if not want_bound:
        return Result(grads, None, {})

    n = S * B + 1
    agz, ah = gz.abs(), h.abs()
    bw_mu = (n + C_TAIL) * U * (torch.einsum("sbk,sbn->kn", x3.abs(), agz) + cw.abs() * w_mu.abs() / sp2)
    aS = torch.einsum("sbk,sbn->kn", xsq, ah)
    rs = rel_sigma(w_rho)
    A = 2 * sw * aS + cw.abs() * (sw / sp2 + 1 / sw)
    P = 2 * sw * aS * (h_rel + U) + 2 * rs * sw * gS.abs() + cw.abs() * (rs * sw / sp2 + (rs + U) / sw)
    bw_rho = sig_w * ((n + C_TAIL) * U * A + P) + rs * g_wrho.abs()
    bb_mu = (n + C_TAIL) * U * (agz.sum((0, 1)) + cb.abs() * b_mu.abs() / sp2)
    rsb = rel_sigma(b_rho)
    Ab = (agz.sum(1) * eps_b.abs()).sum(0) + cb.abs() * (sb / sp2 + 1 / sb)
    bb_rho = sig_b * ((n + C_TAIL) * U * Ab + cb.abs() * (rsb * sb / sp2 + (rsb + U) / sb)) + rsb * g_brho.abs()
    ds2 = s2 * (2 * rs + U)
    dh = ah * h_rel
    ax = x3.abs()
    info = {"tie_share": 0.0}
    if bf16:
        _, slack_h = bf16_tie(h, dh)
        _, slack_s = bf16_tie(s2, ds2)
        info["tie_share"] = max(float((slack_h > 0).double().mean()), float((slack_s > 0).double().mean()))
        Ax = torch.einsum("sbn,kn->sbk", gzr.abs(), Mr.abs()) + 2 * ax * torch.einsum("sbn,kn->sbk", hr.abs(), s2r)
        Px = 2 * ax * (torch.einsum("sbn,kn->sbk", slack_h, s2r + slack_s) + torch.einsum("sbn,kn->sbk", hr.abs(), slack_s))
    else:
        Ax = torch.einsum("sbn,kn->sbk", agz, w_mu.abs()) + 2 * ax * torch.einsum("sbn,kn->sbk", ah, s2)
        Px = 2 * ax * (torch.einsum("sbn,kn->sbk", dh, s2) + torch.einsum("sbn,kn->sbk", ah, ds2))
    b_x = ((2 * N + C_TAIL) * U * Ax + Px) * gxm
    return Result(grads, (bw_mu, bw_rho, bb_mu, bb_rho, b_x), info)


def lr_gx_bf16(math_bf16, N, B, narrow_ok):
    """Where bnn_lr_linear_bwd rounds the input gradient's operands (the dispatch at the end of csrc/lr_bwd.hip): bf16 math with
    N % 8 == 0, and not the narrow output launch (N <= 16, B <= 128, Philox epsilon, v given), which is plain fp32."""
    return bool(math_bf16 and N % 8 == 0 and not (narrow_ok and N <= 16 and B <= 128))


# ------------------------------------------------------------------------------------------------------------ epsilon
def philox_eps(kind, sample0, S, rows, cols, seed=SEED, layer_id=LAYER_ID):
    """float32 [S, rows, cols]: the device's epsilon of tensor 4 * layer_id + kind (0 weights, 1 bias, 2 LR activations)
    for the global samples sample0 .. sample0 + S - 1 (oracle.bnn_oracle.philox_normal, bit-pinned to the device)."""
    return np.stack([O.philox_normal(seed, 4 * layer_id + kind, sample0 + s, rows, cols) for s in range(S)])


def softplus_probe_points():
    """The rho at which E_T is measured: 4096 evenly spaced in [-12, 2] and the fp32 neighbours of the ranges' end points."""
    pts = [np.linspace(-12.0, 2.0, 4096).astype(np.float32)]
    for lo, hi in list(RHO_RANGES.values()) + [(-8.0, -6.0)]:
        for e in (lo, hi):
            e = np.float32(e)
            pts.append(np.array([np.nextafter(e, np.float32(-np.inf)), e, np.nextafter(e, np.float32(np.inf))], np.float32))
    return np.concatenate(pts)


def softplus_error_in_u(got, rho):
    """Largest |got - log1p(exp(rho))| / (u * log1p(exp(rho))), fp64."""
    want = np.log1p(np.exp(rho.astype(np.float64)))
    return float(np.max(np.abs(got.astype(np.float64) - want) / (U * want)))


# ------------------------------------------------------------------------------------------------------------ cases
def _c(S, B, K, N, **kw):
    d = dict(S=S, B=B, K=K, N=N, eps="philox", math="f32", rho="cfg", relu=True, x3=True, mask=False, counter=0, prior="mix",
             wsrc=None, gy16=False, gx16=False, mode="v")
    d.update(kw)
    return d


# (S, B, K, N).  BBB: [out = N, in = K]; weights kernel <VEC = K % 4 == 0, MEM = eps from memory>
BBB_CASES = {
    "w-vec-philox":      _c(3, 20, 72, 37, mask=True),
    "w-vec-mem":         _c(3, 20, 72, 37, eps="memory", rho="wide", x3=False),
    "w-novec-philox":    _c(1, 5, 33, 65, rho="wide", relu=False),
    "w-novec-mem":       _c(1, 5, 33, 65, eps="memory", mask=True),
    "w-grid15of16":      _c(2, 130, 264, 72, rho="wide", x3=False, math="bf16", mask=True, gx16=True),   # 15 work items on a grid of 16
    "w-grid15of16-f32":  _c(2, 130, 264, 72, counter=7),
    "w-n1-gauss":        _c(3, 17, 50, 1, eps="memory", prior="gauss", relu=False),
    "w-n1":              _c(3, 17, 50, 1, rho="wide"),
    "w-b1":              _c(1, 1, 64, 32, math="bf16"),
    "w-s5":              _c(5, 33, 200, 40, rho="wide", counter=3, mask=True),
    "w-s5-gauss":        _c(5, 33, 200, 40, prior="gauss", math="bf16", x3=False),
    # input gradient over the forward's sampled weights: the gather, the transposed matmul (with and without the bf16 gy)
    "x-gather":          _c(5, 33, 200, 40, math="bf16", wsrc="w", mask=True, gx16=True),
    "x-gather-odd":      _c(3, 20, 72, 37, math="bf16", wsrc="w", rho="wide", x3=False),
    "x-wt-gy16":         _c(3, 20, 72, 40, math="bf16", wsrc="wt", gy16=True, relu=False, mask=True, gx16=True),
    "x-wt-relu":         _c(2, 130, 264, 72, math="bf16", wsrc="wt", rho="wide", gx16=True),
    # narrow output layer (bf16 math, w_sampled, N <= 16, B <= 256, K % 8 == 0); PAIR: 112 < B <= 128 and S > 1
    "out-b112":          _c(2, 112, 40, 10, math="bf16", wsrc="w", relu=False, mask=True),
    "out-b113":          _c(2, 113, 40, 10, math="bf16", wsrc="w", relu=False, rho="wide", gx16=True),
    "out-b128":          _c(2, 128, 40, 10, math="bf16", wsrc="w", relu=False, mask=True, gx16=True, counter=5),
    "out-b129":          _c(2, 129, 40, 10, math="bf16", wsrc="w", relu=False, x3=False),
    "out-b256":          _c(2, 256, 40, 10, math="bf16", wsrc="w", relu=True, rho="wide", mask=True),
    "out-b257":          _c(2, 257, 40, 10, math="bf16", wsrc="w", relu=False, mask=True),               # general kernels
    "out-n16":           _c(3, 128, 40, 16, math="bf16", wsrc="w", relu=False, rho="wide", mask=True),
    "out-n17":           _c(2, 128, 40, 17, math="bf16", wsrc="w", relu=False, mask=True),               # general kernels
    "out-k44":           _c(2, 128, 44, 10, math="bf16", wsrc="w", relu=False, mask=True),               # general kernels
    "out-s1":            _c(1, 128, 40, 10, math="bf16", wsrc="w", relu=False, rho="wide", mask=True),   # not PAIR
}
BBB_FULL = _c(1, 16, 1200, 1200, mask=True)       # 722 blocks: the XCD work-item mapping (GPU file only, eps from the device)

# LR: [in = K, out = N]; prep vec N % 4 == 0; weights <VEC = (K | N) even>; input <N % 4 == 0, bf16 math and N % 8 == 0>
LR_CASES = {
    "lr-38":             _c(3, 20, 72, 38, mask=True),
    "lr-38-mem":         _c(3, 20, 72, 38, eps="memory", rho="wide", x3=False),
    "lr-odd":            _c(2, 9, 31, 21, rho="wide", mask=True),
    "lr-odd-hfac":       _c(2, 9, 31, 21, mode="hfac", relu=False, counter=9),
    "lr-k1":             _c(1, 7, 1, 50, eps="memory", mask=True),
    "lr-k1-philox":      _c(1, 7, 1, 50, rho="wide", math="bf16"),
    "lr-72-bf16":        _c(2, 130, 264, 72, math="bf16", mask=True, counter=4),
    "lr-72-bf16-wide":   _c(2, 130, 264, 72, math="bf16", rho="wide", x3=False),
    "lr-72-f32":         _c(2, 130, 264, 72, rho="wide", mask=True),
    "lr-72-hfac-bf16":   _c(2, 130, 264, 72, math="bf16", mode="hfac", relu=False, mask=True),
    "lr-36-bf16":        _c(3, 20, 72, 36, math="bf16", mask=True),                                      # N % 4 == 0 only: fp32 input kernel
    "lr-40-hfac":        _c(3, 20, 72, 40, mode="hfac", relu=False, rho="wide", x3=False),
    # narrow output layer (N <= 16, B <= 128, Philox epsilon, v given): one launch
    "lr-out-n3":         _c(5, 20, 33, 3, mask=True),
    "lr-out-n3-mem":     _c(5, 20, 33, 3, eps="memory", rho="wide", mask=True),                          # general kernels
    "lr-out-b128":       _c(2, 128, 40, 10, relu=False, math="bf16", mask=True, counter=2),
    "lr-out-b128-wide":  _c(2, 128, 40, 10, rho="wide", x3=False),
    "lr-out-b129":       _c(2, 129, 40, 10, relu=False, mask=True),                                      # general kernels
    "lr-out-n16":        _c(2, 128, 40, 16, relu=False, rho="wide", math="bf16", mask=True),
    "lr-out-n17":        _c(2, 128, 40, 17, relu=False, mask=True),                                      # general kernels
}

KL_MODES = ("kl", "data")       # with upstream KL gradients; with g_log_prior = g_log_q = g_kl = None (the data term alone)


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _common(c, rs, lr):
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    lo, hi = RHO_RANGES[c["rho"]]
    wshape = (K, N) if lr else (N, K)
    w_mu, w_rho = rs.uniform(-0.3, 0.3, wshape), rs.uniform(lo, hi, wshape)
    b_mu, b_rho = rs.uniform(-0.3, 0.3, N), rs.uniform(lo, hi, N)
    if not lr and c["prior"] == "mix":
        # a quarter of the weights sit where the narrow component's d log p / dw matters: |mu| <= 2 sigma2, rho in [-8, -6]
        s2 = MIX.sigma2
        for mu, rho in ((w_mu, w_rho), (b_mu, b_rho)):
            near = rs.uniform(size=mu.shape) < 0.25
            mu[near] = rs.uniform(-2 * s2, 2 * s2, int(near.sum()))
            rho[near] = rs.uniform(-8.0, -6.0, int(near.sum()))
    # the end points of the range themselves
    w_rho.flat[0], w_rho.flat[-1] = lo, hi
    x = rs.uniform(-1, 1, (S, B, K) if c["x3"] else (B, K))
    x[rs.uniform(size=x.shape) < 0.05] = 0.0                  # exact zeros under gx_relu_mask
    gy = rs.uniform(-1, 1, (S, B, N))
    if S * B > 1:
        gy[0, 0] = 0.0                                        # one all-zero row
    y = None
    if c["relu"]:
        y = rs.uniform(-1, 1, (S, B, N))
        z = rs.uniform(size=y.shape)
        y[z < 0.025] = 0.0
        y[(z >= 0.025) & (z < 0.05)] = -0.0
        y[-1, -1, 0] = 0.0                                    # at least one of each, in rows where gy is not zero
        if N > 1:
            y[-1, -1, -1] = -0.0
        else:
            y[-1, -2, 0] = -0.0
    d = dict(x=f(x), gy=f(gy), y=None if y is None else f(y), w_mu=f(w_mu), w_rho=f(w_rho), b_mu=f(b_mu), b_rho=f(b_rho))
    d["sample0"] = SAMPLE_OFFSET + c["counter"]
    return d, f


@functools.lru_cache(maxsize=None)
def bbb_inputs(name):
    """numpy fp32 inputs of a BBB case.  eps_w / eps_b carry S + 1 samples (the seeded variant `eps_next_sample`)."""
    c = BBB_CASES[name]
    rs = _rs(name)
    d, f = _common(c, rs, False)
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    if c["eps"] == "memory":
        d["eps_w"], d["eps_b"] = f(rs.standard_normal((S + 1, N, K))), f(rs.standard_normal((S + 1, N)))
    else:
        d["eps_w"] = philox_eps(0, d["sample0"], S + 1, N, K)
        d["eps_b"] = philox_eps(1, d["sample0"], S + 1, 1, N).reshape(S + 1, N)
    d["glp"], d["glq"] = f(rs.uniform(-0.5, 0.5, S)), f(rs.uniform(-0.5, 0.5, S))
    d["w_sampled"] = None
    if c["wsrc"]:
        w = d["w_mu"][None] + 0.01 * rs.standard_normal((S, N, K))
        d["w_sampled"] = torch.from_numpy(f(w)).to(torch.bfloat16)
    d["prior"] = MIX if c["prior"] == "mix" else GAUSS
    return d


@functools.lru_cache(maxsize=None)
def lr_inputs(name):
    """numpy fp32 inputs of an LR case: two all-zero rows of x with v = 0 there; v = fl32(x^2 sigma^2), hfac = fl32(eps /
    (2 sqrt(v))) (0 where v == 0) -- inputs like any other."""
    c = LR_CASES[name]
    rs = _rs(name)
    d, f = _common(c, rs, True)
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    d["x"][..., 1, :] = 0.0
    d["x"][..., 2, :] = 0.0
    if c["eps"] == "memory":
        d["eps_act"], d["eps_b"] = f(rs.standard_normal((S + 1, B, N))), f(rs.standard_normal((S + 1, N)))
    else:
        d["eps_act"] = philox_eps(2, d["sample0"], S + 1, B, N)
        d["eps_b"] = philox_eps(1, d["sample0"], S + 1, 1, N).reshape(S + 1, N)
    x3 = d["x"].astype(np.float64) if c["x3"] else np.broadcast_to(d["x"].astype(np.float64), (S, B, K))
    s2 = np.log1p(np.exp(d["w_rho"].astype(np.float64))) ** 2
    d["v"] = f(np.einsum("sbk,kn->sbn", x3 * x3, s2))
    zero_row = np.broadcast_to((x3 == 0).all(axis=2)[:, :, None], d["v"].shape)
    assert zero_row[:, 1:3].all() and ((d["v"] == 0) == zero_row).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        hf = d["eps_act"][:S].astype(np.float64) / (2 * np.sqrt(d["v"].astype(np.float64)))
    d["hfac"] = f(np.where(d["v"] > 0, hf, 0.0))
    d["gkl"] = f(rs.uniform(0.1, 0.5, 3))
    d["sigma_p"] = 0.8
    return d


def _eps_variant(e, S, variant):
    """The launch's epsilon from the S + 1 stored samples, or a seeded wrong one."""
    if variant == "eps_next_sample":
        return e[1:S + 1]
    e = e[:S]
    if variant == "eps_shift_group":                           # one Philox group of four along the contiguous dimension
        flat = e.reshape(S, -1)
        return np.roll(flat, -4, axis=1).reshape(e.shape)
    return e


def bbb_run(name, kl, dtype=F64, variant=None, want_bound=True, inputs=None):
    """bbb_ref on the inputs of case `name`; kl in KL_MODES."""
    c = BBB_CASES.get(name, BBB_FULL)
    d = inputs if inputs is not None else bbb_inputs(name)
    S = c["S"]
    with_kl = kl == "kl"
    return bbb_ref(d["x"], d["gy"], d["y"], d["w_mu"], d["w_rho"], d["b_mu"], d["b_rho"], prior=d["prior"], relu=c["relu"],
                   eps_w=_eps_variant(d["eps_w"], S, variant), eps_b=_eps_variant(d["eps_b"], S, variant),
                   g_log_prior=d["glp"] if with_kl else None, g_log_q=d["glq"] if with_kl else None, gx_relu_mask=c["mask"],
                   w_sampled=d["w_sampled"], bf16=c["math"] == "bf16", dtype=dtype, variant=variant, want_bound=want_bound)


def lr_run(name, kl, dtype=F64, variant=None, want_bound=True):
    c = LR_CASES[name]
    d = lr_inputs(name)
    S = c["S"]
    factor = c["mode"] == "hfac"
    narrow_ok = c["eps"] == "philox" and not factor
    return lr_ref(d["x"], d["gy"], d["y"], None if factor else d["v"], d["w_mu"], d["w_rho"], d["b_mu"], d["b_rho"],
                  sigma_p=d["sigma_p"], relu=c["relu"], eps_act=_eps_variant(d["eps_act"], S, variant),
                  eps_b=_eps_variant(d["eps_b"], S, variant), g_kl=d["gkl"] if kl == "kl" else None,
                  hfac=d["hfac"] if factor else None, gx_relu_mask=c["mask"],
                  bf16=lr_gx_bf16(c["math"] == "bf16", c["N"], c["B"], narrow_ok), dtype=dtype, variant=variant,
                  want_bound=want_bound)


def shares(got, res):
    """Per tensor: the largest |got - ref| / bound (0 / 0 counts as 0; a NaN, or an error over a zero bound, as inf)."""
    out = []
    for g, r, b in zip(got, res.grads, res.bounds):
        err = (_t(g, F64) - r).abs()
        sh = torch.where(err == 0, torch.zeros_like(err), err / b)         # (x / 0 = inf; NaN stays NaN)
        sh = torch.where(torch.isnan(sh), torch.full_like(sh, float("inf")), sh)
        out.append(float(sh.max()) if sh.numel() else 0.0)
    return out
