"""TEST INFRASTRUCTURE: fp64 restatement of the local-reparameterisation layer FORWARD (bnn_lr_linear_fwd, bnn_lr_final_fwd;
csrc/lr_linear.hip) -- y, the saved variance v, the backward factor hfac and the eval mean path -- with a derived error
bound for EVERY output element, per math mode, on the regime cells of tests/fwd_stats_ref.py (lr_cells, cell_params(lr=True):
that module's docstring describes them), the input kinds of x, an fp32 emulation of the kernels' operation order and the
seeded wrong variants the bound has to reject.  numpy / torch-CPU only: imports without a GPU.  tests/layer_bwd_ref.py takes
y, v and hfac as inputs; this module is what checks them.

What is restated (float64, from the fp32 or bf16 inputs as given), per MC sample s
--------------------------------------------------------------------------------
    sigma = log1p(exp(rho))         m = x . M           v = x^2 . sigma^2          b = b_mu + sigma_b eps_b
    y     = m + sqrt(v) eps_act + b  [-> ReLU]          hfac = eps_act / (2 sqrt(v)), 0 where v == 0 (lr_epilogue_item)
    eval  : y = x . M + b_mu         (BNN_EPS_ZERO, the module's sample=False: fma(sqrt(v), 0, m) + fma(sigma_b, 0, b_mu))
Rounding points per math mode (read from the kernels; oracle/bnn_oracle.py states the same in network_forward_bf16[x3]):
  f32     none.
  bf16    x16 = bf16(x) (or x given as bf16); x^2 = bf16(x16^2) -- the square of the ROUNDED activation, rounded, whoever forms it
          (K3a, K3s and K3r square the fragment they loaded; K3b reads the x_sq stream as passed) --; bf16(M); sigma^2 formed in
          fp32 and then rounded to bf16.  Products of two bf16 numbers are exact in fp32 and accumulation is fp32: the sums stay
          in fp64 here.
  bf16x3  (K3b over bnn_lr_prepare_x3 fragments) the planes x, x_lo, x_sq are INPUTS; M_hi = bf16(M), M_lo = bf16(M - M_hi)
          (M - M_hi is exact in fp32); the kernel multiplies exactly three plane pairs per k-step,
              m = sum x M_hi + x M_lo + x_lo M_hi,
          each product exact, so the restated mean is that sum of 3 K exact terms; the variance as in bf16 math on x_sq as passed.

The bound (first order in u = 2^-24, any summation order; Higham 3.1, as in the two sibling modules)
---------------------------------------------------------------------------------------------------
  m          (n_m + C_TAIL) u sum |x| |M|, n_m = K (3 K in bf16x3: three exact products per k), + 2^-126 per product that
             underflows in fp32.
  sigma^2    delta = (2 rel_sigma(rho) + u) sigma^2                                     (fwd_stats_ref.rel_sigma: E_SP, A_RHO)
  v          (K + C_TAIL) u v + sum x^2 delta(sigma^2)  + 2^-126 (sigma^2 [x^2 underflows] + x^2 [sigma^2 underflows] + [the
             product underflows]) per term: fp32 has no 1e-42.  (f32 math: x^2 and the product round once each, inside C_TAIL.)
             bf16 math: sigma^2 is rounded to bf16 AFTER its fp32 error.  If bf16(q - delta) == bf16(q + delta) the operand is
             that value exactly; otherwise q lies within delta of a rounding tie, either neighbour is legitimate and the
             element's bound grows by x^2 times one bf16 ulp -- for those operands only (layer_bwd_ref.bf16_tie, used as is).
             info["tie_share"] is their share; tests/test_lr_fwd_cpu.py holds it below 1 %.
  sqrt(v)    min(dv / (2 sqrt(v)), sqrt(dv)) + E_SQRT u sqrt(v); the second form where v is tiny or zero.
  b          |eps_b| rel_sigma(b_rho) sigma_b + u |b|                                   (one fma)
  y          dm + |eps| d sqrt(v) + db + C_TAIL u (|m| + sqrt(v) |eps| + |b|).  ReLU is 1-Lipschitz: the same bound after it; no
             element is excluded for sitting near zero.  bf16 y: + 2^-8 (|y| + bound): half an ulp of bf16's 8 significant bits.
             bf16x3, bf16 y: the planes' sum y + y_lo carries 2^-16 (|y| + bound) instead (lo = bf16(v - hi): 2^-8 of 2^-8 |v|).
  hfac       |eps| / 2 (1 / sqrt(v - dv) - 1 / sqrt(v)) + H_ROUNDINGS u |hfac| (layer_bwd_ref: product, sqrt, quotient; this
             square root is the correctly rounded one); exactly 0 where v == 0 with dv == 0 (a zero row); unbounded (inf: nothing
             is asserted) where dv >= v, i.e. where fp32 cannot tell v from 0.
  eval       dm + C_TAIL u (|m| + |b_mu|).

The one new hardware constant, measured on an MI355X against fp64 (tests/test_gpu_lr_fwd.py re-measures it and asserts
measured <= constant / 2; the constant is twice the measured figure rounded up to a power of two, the project's rule):
  E_SQRT   the raw v_sqrt_f32 (__builtin_amdgcn_sqrtf) of y's epilogue: lr_linear_fwd on a 1 x 1 layer with M = 0, b = 0,
           sigma_b eps_b = 0 and eps_act = 1 returns y = sqrt(v) of the v it saves (want_v) bit for bit; largest
           |y - sqrt(v)| / (u sqrt(v)) over sqrt_probe_x():                              measured 1.3331, E_SQRT = 4
Nothing else is tuned on device figures.

Cells: lr_cells("lr-1") (sigma_p does not enter y): 12 rho levels x 8 |mu| levels + the cancellation cell = 97 regular,
the rho = -100 band, the edges rho = 89 (sigma = +inf) and rho = -200 (sigma = 0).  Epsilon as in cell_eps: sample s is
uniform in +-EPS_SCALES[(s + shift) % 4], so sample 0 is the mean path and the |mu| = 0 cells show sqrt(v) by itself; on
the generator paths whatever O.philox_normal gives.  Input kinds of x: (a) signed uniform(-1, 1) = cell_x; (b) ReLU-like:
non-negative, half zeros, row 1 and column 2 all zero (v = 0, hfac = 0, y = b on the zero row); (c) (a) scaled by 2^-70: x^2
underflows, v is 0 on the device where fp64 has 1e-42 -- the sqrt(dv) branch and the 2^-126 terms are what covers it.
"""
import collections
import functools

import numpy as np
import torch

import fwd_stats_ref as R
import layer_bwd_ref as LB

U, C_TAIL, MIN_NORMAL = R.U, R.C_TAIL, R.MIN_NORMAL
H_ROUNDINGS = LB.H_ROUNDINGS
E_SQRT_MEASURED, E_SQRT = 1.3331, 4.0        # MI355X; twice the measured figure rounded up to a power of two
HALF_BF16 = 2.0 ** -8                         # half an ulp of bf16 (8 significant bits), relative
F64, f32 = np.float64, np.float32
MATHS = ("f32", "bf16", "bf16x3")
CELLS = "lr-1"
SIDE_MU_INDEX = 3                             # |mu| = 0.05: the level the reduced grid (rho levels at one |mu|) runs on

LrRef = collections.namedtuple("LrRef", "y v hfac m bias b_y b_v b_hfac y_mean b_y_mean info")


def cells(grid="full"):
    """lr_cells("lr-1"), or (`rho`) its rho levels at |mu| = 0.05 with the cancellation, band and edge cells."""
    cs = R.lr_cells(CELLS)
    if grid == "full":
        return cs
    return tuple(c for c in cs if c.tag != "regular" or c.name.endswith(f"/mu{SIDE_MU_INDEX}") or c.name.endswith("/cancel"))


def lr_eps(S, B, N, shift=0):
    """Injected epsilon: (eps_act [S, B, N], eps_b [S, N]) fp32, sample s uniform in +-EPS_SCALES[(s + shift) % 4]."""
    rs = R._rs(f"lr-eps/{S}/{B}x{N}/{shift}")
    sc = np.array([R.EPS_SCALES[(s + shift) % 4] for s in range(S)])
    return (np.ascontiguousarray(sc[:, None, None] * rs.uniform(-1, 1, (S, B, N)), f32),
            np.ascontiguousarray(sc[:, None] * rs.uniform(-1, 1, (S, N)), f32))


def philox_eps(seed, layer_id, sample0, S, B, N):
    """The generator's (eps_act [S, B, N], eps_b [S, N]) of samples sample0 .. (layer_bwd_ref.philox_eps: kinds 2 and 1)."""
    return (LB.philox_eps(2, sample0, S, B, N, seed=seed, layer_id=layer_id),
            LB.philox_eps(1, sample0, S, 1, N, seed=seed, layer_id=layer_id).reshape(S, N))


@functools.lru_cache(maxsize=None)
def kind_x(kind, B, K, S=0):
    """x of input kind 'a' | 'b' | 'c' (module docstring), fp32 [B, K] or [S, B, K]."""
    x = R.cell_x(B, K, S)
    if kind == "a":
        return x
    if kind == "c":
        return np.ascontiguousarray(x * f32(2.0 ** -70), f32)
    assert kind == "b" and B >= 2 and K >= 3
    x = np.maximum(x, 0).astype(f32)
    x[..., 1, :] = 0
    x[..., :, 2] = 0
    return np.ascontiguousarray(x)


# ------------------------------------------------------------------------------------------------------ fp64 restatement
def _np64(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().float().numpy()
    return np.asarray(a, F64)


def bf16(v):
    """fp64 -> fl32 -> bf16 (RNE), as (__bf16)float on the device."""
    return R._bf16(np.asarray(v, f32)).astype(F64)


def bf16_tie(q, delta):
    a, s = LB.bf16_tie(torch.from_numpy(np.ascontiguousarray(q, F64)), torch.from_numpy(np.ascontiguousarray(delta, F64)))
    return a.numpy(), s.numpy()


def _small(a):
    return (a > 0) & (a < MIN_NORMAL)


def _underflows(a, b):
    """Per output element: how many products a[.., k] b[k, n] are non-zero and below 2^-126."""
    a, b = np.abs(a), np.abs(b)
    na, nb = a[a > 0], b[b > 0]
    if na.size == 0 or nb.size == 0 or na.min() * nb.min() >= MIN_NORMAL:
        return 0.0
    return _small(a[..., :, None] * b).sum(-2).astype(F64)


def lr_ref(x, w_mu, w_rho, b_mu, b_rho, eps_act=None, eps_b=None, *, math="f32", relu=False, x_sq=None, x_lo=None,
           y_bf16=False, n_samples=None):
    """fp64 outputs of one launch and their bounds.  x [B, K] or [S, B, K] (fp32 numpy, or the bf16 tensor passed); weights
    [K, N]; eps_act [S, B, N], eps_b [S, N], or None for BNN_EPS_ZERO.  bf16 math: `x_sq` as passed (K3b) or None (squared by the
    kernel); bf16x3: x is the high plane, with `x_lo` and `x_sq`.  Every returned array is [S, B, N] (bias: [S, N])."""
    assert math in MATHS
    x, M, rho, bmu, brho = _np64(x), _np64(w_mu), _np64(w_rho), _np64(b_mu), _np64(b_rho)
    K, N = M.shape
    S = eps_act.shape[0] if eps_act is not None else (n_samples or (x.shape[0] if x.ndim == 3 else 1))
    ea = _np64(eps_act) if eps_act is not None else np.zeros((S,) + x.shape[-2:-1] + (N,))
    eb = _np64(eps_b) if eps_b is not None else np.zeros((S, N))
    sg = R.softplus64(rho)
    s2 = sg * sg
    ds2 = (2 * R.rel_sigma(rho) + U) * s2
    info = {"tie_share": 0.0}
    planes = None
    if math == "f32":
        xm, Mm, s2m, P = x, M, s2, ds2
        xq = x * x
    else:
        xm = bf16(x) if math == "bf16" else x
        xq = _np64(x_sq) if x_sq is not None else bf16(xm * xm)
        Mm = bf16(M)
        s2m, P = bf16_tie(s2, ds2)
        info["tie_share"] = float((P > 0).mean())
        if math == "bf16x3":
            planes = ((xm, bf16(M - Mm)), (_np64(x_lo), Mm))
    m, am = xm @ Mm, np.abs(xm) @ np.abs(Mm)
    uf_m = _underflows(xm, Mm)
    n_m = K
    for a, b in planes or ():
        m, am, uf_m, n_m = m + a @ b, am + np.abs(a) @ np.abs(b), uf_m + _underflows(a, b), n_m + K
    dm = (n_m + C_TAIL) * U * am + MIN_NORMAL * uf_m
    v = xq @ s2m
    x2 = xm * xm if x_sq is None else np.zeros_like(xq)         # (a passed x_sq is an input: no square is formed)
    uf_v = _small(x2).astype(F64) @ s2m + xq @ _small(s2).astype(F64) + _underflows(xq, s2m)
    dv = (K + C_TAIL) * U * v + xq @ P + MIN_NORMAL * uf_v
    sd = np.sqrt(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsd = np.where(v > 0, np.minimum(dv / (2 * sd), np.sqrt(dv)), np.sqrt(dv)) + E_SQRT * U * sd
    sgb = R.softplus64(brho)
    bias = bmu + sgb * eb
    db = np.abs(eb) * R.rel_sigma(brho) * sgb + U * np.abs(bias)
    act = lambda t: np.maximum(t, 0) if relu else t
    y_lin = m + sd * ea + bias[:, None, :]
    b_y = dm + np.abs(ea) * dsd + db[:, None, :] + C_TAIL * U * (np.abs(m) + sd * np.abs(ea) + np.abs(bias)[:, None, :])
    y = act(y_lin)
    y_mean = act(np.broadcast_to(m + bmu, y.shape))
    b_y_mean = np.broadcast_to(dm + C_TAIL * U * (np.abs(m) + np.abs(bmu)), y.shape)
    if y_bf16:
        b_y = b_y + HALF_BF16 * (np.abs(y) + b_y)
        b_y_mean = b_y_mean + HALF_BF16 * (np.abs(y_mean) + b_y_mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        hfac = np.where(v > 0, ea / (2 * sd), 0.0)
        b_h = np.where(dv < v, 0.5 * np.abs(ea) * (1 / np.sqrt(np.maximum(v - dv, 0)) - 1 / sd) + H_ROUNDINGS * U * np.abs(hfac),
                       np.where((v == 0) & (dv == 0), 0.0, np.inf))
    bc = lambda t: np.broadcast_to(t, y.shape)
    return LrRef(y, bc(v), bc(hfac), bc(m), bias, b_y, bc(dv), bc(b_h), y_mean, b_y_mean, info)


# ----------------------------------------------------------------- fp32 emulation of the kernels' arithmetic, and variants
VARIANTS = ("v_drop_last_k", "v_tail_twice", "s2_bf16_in_f32", "x2_not_rerounded", "sd_bf16", "bias_noise_dropped",
            "relu_before_bias", "hfac_sqrt_eps")


def _chain(a, b):
    """sum_k a[.., k] b[k, n]: rounded products, left-to-right fp32 accumulation in k order."""
    t = (a[..., :, None].astype(f32) * b.astype(f32)).astype(f32)
    return np.cumsum(t, axis=-2, dtype=f32)[..., -1, :]


def emu_lr(x, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b, *, math="f32", relu=False, variant=None):
    """(y, v, hfac) fp32 [S, B, N] in the kernels' operation order: softplus as bnn::softplus (fwd_stats_ref.emu_softplus),
    sigma^2 = fl(sigma sigma), x^2 = fl(x x) (bf16 math: of the rounded x, re-rounded), fp32 k-ordered chains, y = fl(fma(sqrt(v),
    eps, m) + fma(sigma_b, eps_b, b_mu)), hfac = eps / (2 sqrt(v)).  `variant`: one of VARIANTS -- each a plausible kernel slip."""
    x, M = np.asarray(x, f32), np.asarray(w_mu, f32)
    ea, eb = np.asarray(eps_act, f32), np.asarray(eps_b, f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        sg, sgb = R.emu_softplus(np.asarray(w_rho, f32)), R.emu_softplus(np.asarray(b_rho, f32))
        s2 = (sg * sg).astype(f32)
        if math == "bf16":
            xb = R._bf16(x)
            xq = R._bf16((x * x).astype(f32) if variant == "x2_not_rerounded" else (xb * xb).astype(f32))
            x, M, s2 = xb, R._bf16(M), R._bf16(s2)
        else:
            xq = (x * x).astype(f32)
            if variant == "s2_bf16_in_f32":
                s2 = R._bf16(s2)
        m = _chain(x, M)
        if variant == "v_drop_last_k":
            v = _chain(xq[..., :-1], s2[:-1])
        elif variant == "v_tail_twice":
            v = _chain(np.concatenate([xq, xq[..., -1:]], -1), np.concatenate([s2, s2[-1:]], 0))
        else:
            v = _chain(xq, s2)
        sd = np.sqrt(v).astype(f32)
        sdy = R._bf16(sd) if variant == "sd_bf16" else sd
        bias = R._fma(sgb[None], eb, np.asarray(b_mu, f32)[None]) if variant != "bias_noise_dropped" else np.broadcast_to(np.asarray(b_mu, f32), eb.shape)
        y = R._fma(np.broadcast_to(sdy, ea.shape), ea, np.broadcast_to(m, ea.shape))
        if variant == "relu_before_bias":
            y = (np.maximum(y, 0) + bias[:, None, :]).astype(f32)
        else:
            y = (y + bias[:, None, :]).astype(f32)
            if relu:
                y = np.maximum(y, 0)
        sdh = np.sqrt((v + f32(1e-8)).astype(f32)) if variant == "hfac_sqrt_eps" else sd
        hfac = np.where(sdh > 0, ea / (f32(2) * sdh), f32(0)).astype(f32)
    return y, np.broadcast_to(v, ea.shape), hfac


# ------------------------------------------------------------------------------------------------- measuring the constant
def sqrt_probe_x():
    """x of the E_SQRT probe: 4096 points log-uniform over [2^-20, 2^20] (v = fl(x^2) fl(sigma^2) walks every mantissa and both
    exponent parities) and 256 around 1."""
    rs = R._rs("sqrt-probe")
    return np.concatenate([np.exp2(rs.uniform(-20, 20, 4096)), 1 + rs.uniform(-0.5, 1.0, 256)]).astype(f32)


def sqrt_error_in_u(y, v):
    """Largest |y - sqrt(v)| / (u sqrt(v)) over the probe, fp64."""
    want = np.sqrt(np.asarray(v, F64))
    return float(np.max(np.abs(np.asarray(y, F64) - want) / (U * want)))
