"""TEST INFRASTRUCTURE: float64 restatement of one launch of the grouped bandit kernels (include/bnn_hip.h F6
bnn_mlp_group_*, F7 bnn_bbb_group_*; csrc/mlp_group.hip, csrc/bbb_group.hip), the cases the CPU and GPU tests share, the
fp32 restatement whose distance from the float64 one sets the bound (d_ref), and the bound itself.

The float64 side knows none of the kernels' hand-derived formulas: the forward and the loss are written as include/bnn_hip.h
states them and differentiated by CPU torch float64 autograd; Adam is torch.optim.Adam's _single_tensor_adam (weight decay
added to the gradient, t given).  F7's epsilon is an argument: the oracle's restatement of the stream here, the device's own
materialised stream (ops.philox_normal, widened) in the GPU tests.  Nothing here imports the product.

The fp32 side (step32 / forward32) is numpy float32 with the gradients in closed form and numpy's own `@` / sum order, which is
not the kernels' k-ascending fma chain: its deviation from the float64 side, per tensor class and relative to the tensor's
max |.|, is d_ref.  A kernel is allowed bound(d_ref, n) = min(max(4 d_ref, n 2^-23), 2e-4): two independent orderings on either
side of the comparison times a factor 2 (the margin of tests/test_gpu_bnn_bandit_group.py), never more than F6's standing 2e-4
of scale, and never less than n roundings of the longest path of that quantity (FLOOR_OPS below)."""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import bnn_oracle as O

F32, F64 = np.float32, np.float64
C0 = -0.9189385332046727                 # -log sqrt(2 pi)
ULP = 2.0 ** -23
CAP = 2e-4                               # F6's standing bound (tests/test_gpu_greedy_bandit.py _close)
CLASSES = ("params", "exp_avg", "exp_avg_sq", "outputs")

# The floor's n: rounded operations on the longest path from the launch's inputs to one element of the class, counted in
# csrc/mlp_group.hip / csrc/bbb_group.hip / csrc/mlp_group_common.h at 1-1-1, batch 1, S 1 (every chain one fma long; at that
# shape d_ref can be a few ULP or zero by luck).  An operation correctly rounded is off by 2^-24 of its result and the hardware
# exp / log / rcp by at most 2^-23, so n 2^-23 is twice the first-order worst case of n such operations.
#   F6 outputs      6: three layers of (one fma, + bias).
#   F6 gradient    10: outputs 6; z - y (2 (z - y) is exact) 7; dz w3 8; the dh1 fma 9; the dW1 fma 10.
#   F6 exp_avg     14: gradient 10; fma(wd, p, g) 11; gg - m 12; * omb1 13; m + 14.
#   F6 exp_avg_sq  15: fma(wd, p, g) 11; omb2 gg 12; * gg 13; (v beta2f beside it) + 15.
#   F6 params      21: exp_avg_sq 15; sqrt 16; / sqrt_bc2 17; + eps 18; m / denom 19; * step_size 20; p - 21.
#   F7 outputs     10: softplus = log(1 + exp(rho)) 3; fma(sigma, eps, mu) 4; then F6's 6.
#   F7 gradient    19: outputs 10; z - y 11; * 1/S 12; dz w3 13; dh1 14; dW1 15; G += 16 (the prior's share joins at 13);
#                      fma(v, eps, H) 17; H - beta rcp(sigma) 18; * sigmoid(rho) 19.
#   F7 exp_avg 23, exp_avg_sq 24, params 30: F6's 4, 5 and 11 further operations after the gradient.
FLOOR_OPS = dict(f6=dict(params=21, exp_avg=14, exp_avg_sq=15, outputs=6),
                 f7=dict(params=30, exp_avg=23, exp_avg_sq=24, outputs=10))

PERTURBATIONS = ("no_weight_decay", "t_minus_one", "betas_swapped", "no_inv_s", "no_sigmoid", "no_beta_over_sigma",
                 "eps_of_previous_sample", "beta_of_previous_batch", "accumulators_kept")


def bound(d_ref: float, n_ops: int) -> float:
    return min(max(4.0 * d_ref, n_ops * ULP), CAP)


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    kind: str                              # "f6" | "f7"
    I: int
    H: int
    B: int                                 # batch (a step) or n_rows (a forward)
    nb: int = 1
    S: int = 1
    prior_init: Tuple[float, ...] = (1.0,)
    mixture: bool = False
    betas: Tuple[float, float] = (0.8, 0.95)
    eps: float = 1e-6
    wd: float = 1e-2
    lr: float = 1e-3
    step0: int = 7
    kl: Tuple[float, ...] = (0.37, 0.11)   # KL weights, none a power of two
    seed: int = 0
    eps_seed: int = 4242
    counter: int = 7
    zero_eps: bool = False                 # a forward under EPS_ZERO
    gapped: bool = False                   # inputs whose gates are far from zero by construction (inputs())

    @property
    def id(self):
        tail = "" if self.kind == "f6" else f"-S{self.S}-{'mix' if self.mixture else 'gauss'}{'-mean' if self.zero_eps else ''}"
        adam = "-default" if self.betas == (0.9, 0.999) else ""
        return f"{self.kind}-{self.I}-{self.H}-b{self.B}-nb{self.nb}{tail}{adam}"

    def applies(self, perturbation: str) -> bool:
        f7 = self.kind == "f7"
        return {"no_weight_decay": self.wd != 0, "t_minus_one": True, "betas_swapped": True, "no_inv_s": f7 and self.S > 1,
                "no_sigmoid": f7, "no_beta_over_sigma": f7, "eps_of_previous_sample": f7,
                "beta_of_previous_batch": f7 and self.nb > 1, "accumulators_kept": f7 and self.nb > 1}[perturbation]


DEFAULT_ADAM = dict(betas=(0.9, 0.999), eps=1e-8, wd=0.0)
MIX = dict(prior_init=(0.5, 0.0, -6.0), mixture=True)

# The seeds are those whose float64 pre-activations all keep the margin of gate_margin_ok from zero (tests/test_group_ref_cpu.py
# asserts it), so that fp32 and float64 take the same ReLU branches everywhere and no element has to be left out.
STEP_CASES = (
    Case("f6", 1, 1, 1, seed=1),
    Case("f6", 5, 7, 3, seed=0),
    Case("f6", 37, 19, 8, seed=0),
    Case("f6", 37, 19, 8, seed=0, **DEFAULT_ADAM),
    Case("f6", 128, 128, 64, seed=65),
    Case("f7", 1, 1, 1, nb=1, S=1, seed=1),
    Case("f7", 5, 7, 3, nb=2, S=8, seed=0, **MIX),
    Case("f7", 37, 19, 8, nb=2, S=2, seed=0),
    Case("f7", 37, 19, 8, nb=1, S=2, seed=0, **MIX, **DEFAULT_ADAM),
    Case("f7", 128, 128, 64, nb=1, S=2, seed=64, **MIX),
)

_FWD_SHAPES = tuple((I, H, A) for (I, H) in ((1, 1), (37, 19), (128, 128)) for A in (1, 5, 64))
_FWD_SEEDS = {("f6", 128, 128, 64, 1, False): 65, ("f7", 37, 19, 64, 8, False): 9, ("f7", 128, 128, 5, 8, False): 4,
              ("f7", 128, 128, 64, 1, False): 64, ("f7", 128, 128, 64, 1, True): 13}      # every other forward case: seed 0
FWD_CASES = tuple(Case("f6", I, H, A, seed=_FWD_SEEDS.get(("f6", I, H, A, 1, False), 0)) for (I, H, A) in _FWD_SHAPES) + \
    tuple(Case("f7", I, H, A, S=S, seed=_FWD_SEEDS.get(("f7", I, H, A, S, z), 0), zero_eps=z, gapped=(I, A, S) == (128, 64, 8))
          for (I, H, A) in _FWD_SHAPES for (S, z) in ((1, False), (8, False), (1, True)))


def with_seed(case: Case, seed: int) -> Case:
    return replace(case, seed=seed)


# ---------------------------------------------------------------------------------------------------------------- inputs
def shapes(case):
    """The parameter shapes in the agent block's order (F6: w1 b1 w2 b2 w3 b3; F7: (w_mu, w_rho, b_mu, b_rho) x 3)."""
    I, H = case.I, case.H
    lin = [(H, I), (H,), (H, H), (H,), (1, H), (1,)]
    return lin if case.kind == "f6" else [s for k in range(3) for s in (lin[2 * k], lin[2 * k], lin[2 * k + 1], lin[2 * k + 1])]


def oracle_eps(case):
    """eps(layer, kind, first, S, rows, cols) -> float64 [S, rows, cols] from the oracle's restatement of the device stream."""
    def f(layer, kind, first, S, rows, cols):
        return np.stack([O.philox_normal(case.eps_seed, O.tensor_id(layer, kind), (first + s) & 0xFFFFFFFF, rows, cols)
                         for s in range(S)]).astype(F64)
    return f


def inputs(case: Case, train: bool = True):
    """float32 inputs of one launch: params, slab [nb, B, I] / targets [nb, B] (a step) or rows [B, I] (a forward), and for a
    step the loaded Adam state: exp_avg = 0.5 rms(g) N(0, 1) and exp_avg_sq = (1 - beta2^20) rms(g)^2 U(0.5, 1.5), g the
    float64 gradient of the first minibatch at the start point (per tensor): what twenty steps of such gradients leave."""
    rs = np.random.RandomState(1000 * case.seed + 17 * case.I + case.H + (0 if case.kind == "f6" else 500))
    I, H, B = case.I, case.H, case.B
    ps = []
    if case.kind == "f6":
        for shp in shapes(case):
            k = 1.0 / np.sqrt(shp[1] if len(shp) == 2 else (I if len(ps) == 1 else H))      # nn.Linear's range
            ps.append(rs.uniform(-k, k, shp).astype(F32))
    else:
        for q, shp in enumerate(shapes(case)):
            ps.append((rs.uniform(-5, -4, shp) if q & 1 else rs.uniform(-0.2, 0.2, shp)).astype(F32))
    if case.gapped:
        # 128-128 with 64 rows and 8 draws has 131072 pre-activations per layer: about 25 of them lie within 100 d_ref of zero
        # whatever the seed.  Weights a tenth as wide and hidden biases of +-U(0.5, 1) keep every gate five deviations from
        # zero; about half the units are on, and the rows and draws still move every output.
        for q in (0, 4):
            ps[q] = (0.1 * ps[q]).astype(F32)
        for q in (2, 6):
            ps[q] = (np.sign(ps[q]) * rs.uniform(0.5, 1.0, ps[q].shape)).astype(F32)
    if case.I == 1 and case.H == 1:
        # the one-unit net: a live path (positive weights and biases), or no gradient reaches layer 1
        ps = [np.abs(p) if (case.kind == "f6" or q % 2 == 0) else p for q, p in enumerate(ps)]
    out = dict(params=ps)
    if not train:
        out["rows"] = rs.uniform(0, 1, (B, I)).astype(F32)
        return out
    out["slab"] = rs.uniform(0, 1, (case.nb, B, I)).astype(F32)
    out["targets"] = (rs.standard_normal((case.nb, B)) * 5).astype(F32)
    g = _gradients64(case, [torch.from_numpy(p.astype(F64)) for p in ps], out["slab"][0], out["targets"][0], case.kl[0],
                     None if case.kind == "f6" else _eps_lists(case, oracle_eps(case), case.counter))[0]
    out["exp_avg"], out["exp_avg_sq"] = [], []
    for p, gt in zip(ps, g):
        rms = max(float(np.sqrt(np.mean(gt.numpy() ** 2))), 1e-3)
        out["exp_avg"].append((0.5 * rms * rs.standard_normal(p.shape)).astype(F32))
        out["exp_avg_sq"].append(((1 - case.betas[1] ** 20) * rms * rms * rs.uniform(0.5, 1.5, p.shape)).astype(F32))
    return out


def _eps_lists(case, eps_fn, first):
    """Six float64 arrays [S, *shape] (w1 b1 w2 b2 w3 b3) of draws first .. first + S - 1; biases drawn as [1, out]."""
    I, H = case.I, case.H
    dims = [(H, I), (H, H), (1, H)]
    out = []
    for layer, (n, k) in enumerate(dims):
        out.append(eps_fn(layer, 0, first, case.S, n, k))
        out.append(eps_fn(layer, 1, first, case.S, 1, n).reshape(case.S, n))
    return out


# ---------------------------------------------------------------------------------------------------------------- Adam
def adam(p, m, v, g, t, lr, betas, eps, wd, T=F64):
    """torch.optim.Adam's _single_tensor_adam on numpy arrays of dtype T: (p', m', v').  The scalars are formed in fp64 and
    rounded once to T, as torch forms them on the host and the kernels receive them."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step_size, sqrt_bc2 = T(lr / bc1), T(np.sqrt(bc2))
    if wd != 0:
        g = g + T(wd) * p
    m = m + (g - m) * T(1.0 - b1)
    v = v * T(b2) + T(1.0 - b2) * g * g
    denom = np.sqrt(v) / sqrt_bc2 + T(eps)
    return (p - step_size * (m / denom)).astype(T), m.astype(T), v.astype(T)


# ---------------------------------------------------------------------------------------------------------------- float64
def _mlp64(x, w1, b1, w2, b2, w3, b3):
    a1 = x @ w1.T + b1
    a2 = torch.relu(a1) @ w2.T + b2
    return (torch.relu(a2) @ w3.T + b3).squeeze(-1), a1, a2


def _log_prior64(case, w):
    if not case.mixture:
        sp = case.prior_init[0]
        return (C0 - np.log(sp) - w * w / (2 * sp * sp)).sum()
    pi, s1, s2 = case.prior_init[0], np.exp(case.prior_init[1]), np.exp(case.prior_init[2])
    l1 = np.log(pi) + C0 - np.log(s1) - w * w / (2 * s1 * s1)
    l2 = np.log(1 - pi) + C0 - np.log(s2) - w * w / (2 * s2 * s2)
    return torch.logaddexp(l1, l2).sum()


def _gradients64(case, ps, x, y, beta, eps, perturb=None):
    """Autograd through the loss as include/bnn_hip.h states it.  ps: float64 tensors; eps: six lists of S arrays (F7).
    Returns (gradients, info): info = dict(loss | loss_info, z [S, B], pre1, pre2 [S, B, H], abs_q, abs_p)."""
    ps = [p.clone().requires_grad_(True) for p in ps]
    x, y = torch.from_numpy(np.asarray(x, F64)), torch.from_numpy(np.asarray(y, F64))
    if case.kind == "f6":
        z, a1, a2 = _mlp64(x, *ps)
        loss = torch.nn.functional.mse_loss(z, y, reduction="sum")
        loss.backward()
        return [p.grad for p in ps], dict(loss=float(loss.detach()), z=z.detach().numpy()[None], pre1=a1.detach().numpy()[None],
                                          pre2=a2.detach().numpy()[None])
    S = case.S
    lq = lp = nll = 0.0
    abs_q = abs_p = 0.0
    zs, a1s, a2s = [], [], []
    for s in range(S):
        ws = []
        for q in range(6):
            mu, rho = ps[2 * q], ps[2 * q + 1]
            e = torch.from_numpy(np.asarray(eps[q][s], F64)).reshape(mu.shape)
            sigma = torch.log1p(torch.exp(rho))
            w = mu + sigma * e
            log_sigma = torch.log(sigma.detach() if perturb == "no_beta_over_sigma" else sigma)
            tq = C0 - log_sigma - (w - mu) ** 2 / (2 * sigma ** 2)
            lq = lq + tq.sum()
            lp = lp + _log_prior64(case, w)
            abs_q += float(tq.detach().abs().sum())
            abs_p += float(_abs_prior_terms(case, w.detach()))
            ws.append(w)
        z, a1, a2 = _mlp64(x, *ws)
        nll = nll + (0.5 * (z - y) ** 2 - C0).sum()
        zs.append(z.detach().numpy()), a1s.append(a1.detach().numpy()), a2s.append(a2.detach().numpy())
    m_lq, m_lp = lq / S, lp / S
    m_nll = nll if perturb == "no_inv_s" else nll / S
    loss = beta * (m_lq - m_lp) + m_nll
    loss.backward()
    grads = [p.grad for p in ps]
    if perturb == "no_sigmoid":
        grads = [g / torch.sigmoid(ps[i].detach()) if i & 1 else g for i, g in enumerate(grads)]
    info = dict(loss_info=np.array([float(t.detach()) for t in (loss, m_lp, m_lq, nll / S)]), z=np.stack(zs), pre1=np.stack(a1s),
                pre2=np.stack(a2s), abs_q=abs_q / S, abs_p=abs_p / S, abs_r=float(np.abs(np.stack(zs) - y.numpy()).sum()) / S)
    return grads, info


def _abs_prior_terms(case, w):
    if not case.mixture:
        sp = case.prior_init[0]
        return (C0 - np.log(sp) - w * w / (2 * sp * sp)).abs().sum()
    pi, s1, s2 = case.prior_init[0], np.exp(case.prior_init[1]), np.exp(case.prior_init[2])
    l1 = np.log(pi) + C0 - np.log(s1) - w * w / (2 * s1 * s1)
    l2 = np.log(1 - pi) + C0 - np.log(s2) - w * w / (2 * s2 * s2)
    return torch.logaddexp(l1, l2).abs().sum()


def step64(case: Case, inp, eps_fn=None, perturb: Optional[str] = None):
    """The launch in float64: nb minibatches from the loaded state.  Returns dict(params, exp_avg, exp_avg_sq (lists of float64
    arrays), step, counter, loss | loss_info, z [nb, S, B], pre1, pre2 [nb, S, B, H], and the last minibatch's abs_* sums)."""
    assert perturb is None or perturb in PERTURBATIONS
    f7 = case.kind == "f7"
    eps_fn = eps_fn or (oracle_eps(case) if f7 else None)
    lr = float(F32(case.lr))                                       # the device word
    betas = case.betas[::-1] if perturb == "betas_swapped" else case.betas
    wd = 0.0 if perturb == "no_weight_decay" else case.wd
    p = [a.astype(F64) for a in inp["params"]]
    m = [a.astype(F64) for a in inp["exp_avg"]]
    v = [a.astype(F64) for a in inp["exp_avg_sq"]]
    kl = [float(F32(b)) for b in case.kl]                          # the table is fp32
    zs, p1, p2, info, kept = [], [], [], None, None
    for j in range(case.nb):
        eps = None
        if f7:
            first = case.counter + j * case.S - (1 if perturb == "eps_of_previous_sample" else 0)
            eps = _eps_lists(case, eps_fn, first)
        beta = kl[j - 1] if (perturb == "beta_of_previous_batch" and j > 0) else kl[j]
        g, info = _gradients64(case, [torch.from_numpy(a) for a in p], inp["slab"][j], inp["targets"][j], beta, eps, perturb)
        g = [a.numpy() for a in g]
        if f7 and perturb == "accumulators_kept":
            # G and H of this minibatch as the launch holds them before Adam: G = g_mu, H = g_rho / sigmoid(rho) + beta / sigma
            acc = []
            for q in range(6):
                rho = p[2 * q + 1]
                sig, sgm = np.log1p(np.exp(rho)), 1.0 / (1.0 + np.exp(-rho))
                acc.append((g[2 * q], g[2 * q + 1] / sgm + beta / sig))
            if kept is not None:
                for q in range(6):
                    rho = p[2 * q + 1]
                    sig, sgm = np.log1p(np.exp(rho)), 1.0 / (1.0 + np.exp(-rho))
                    acc[q] = (acc[q][0] + kept[q][0], acc[q][1] + kept[q][1])
                    g[2 * q], g[2 * q + 1] = acc[q][0], (acc[q][1] - beta / sig) * sgm
            kept = acc
        t = case.step0 + j + (0 if perturb == "t_minus_one" else 1)
        for i in range(len(p)):
            p[i], m[i], v[i] = adam(p[i], m[i], v[i], g[i], t, lr, betas, case.eps, wd)
        zs.append(info["z"]), p1.append(info["pre1"]), p2.append(info["pre2"])
    out = dict(params=p, exp_avg=m, exp_avg_sq=v, step=case.step0 + case.nb, counter=case.counter + case.nb * case.S,
               z=np.stack(zs), pre1=np.stack(p1), pre2=np.stack(p2))
    out.update({k: info[k] for k in info if k not in ("z", "pre1", "pre2")})
    return out


def forward64(case: Case, inp, eps_fn=None):
    """The decision forward in float64: dict(z [S, A] ([1, A] under EPS_ZERO), pre1, pre2)."""
    ps = [torch.from_numpy(a.astype(F64)) for a in inp["params"]]
    x = torch.from_numpy(inp["rows"].astype(F64))
    if case.kind == "f6":
        z, a1, a2 = _mlp64(x, *ps)
        return dict(z=z.numpy()[None], pre1=a1.numpy()[None], pre2=a2.numpy()[None])
    if case.zero_eps:
        z, a1, a2 = _mlp64(x, *ps[0::2])
        return dict(z=z.numpy()[None], pre1=a1.numpy()[None], pre2=a2.numpy()[None])
    eps = _eps_lists(case, eps_fn or oracle_eps(case), case.counter)
    zs, a1s, a2s = [], [], []
    for s in range(case.S):
        ws = [ps[2 * q] + torch.log1p(torch.exp(ps[2 * q + 1])) * torch.from_numpy(eps[q][s]).reshape(ps[2 * q].shape)
              for q in range(6)]
        z, a1, a2 = _mlp64(x, *ws)
        zs.append(z.numpy()), a1s.append(a1.numpy()), a2s.append(a2.numpy())
    return dict(z=np.stack(zs), pre1=np.stack(a1s), pre2=np.stack(a2s))


# ---------------------------------------------------------------------------------------------------------------- closed form
def _sigmoid(r, T):
    return (T(1) / (T(1) + np.exp(-r))).astype(T)


def _dlogp(case, w, T):
    if not case.mixture:
        return (-w * T(1.0 / case.prior_init[0] ** 2)).astype(T)
    pi, s1, s2 = case.prior_init[0], np.exp(case.prior_init[1]), np.exp(case.prior_init[2])
    w2 = w * w
    # the narrow component's share, scaled by the wide one's: exp of a difference, safe from 0 / 0 in fp32
    r = (T((1 - pi) / s2 / (pi / s1)) * np.exp(-w2 * T(1 / (2 * s2 * s2) - 1 / (2 * s1 * s1)))).astype(T)
    return (-w * (T(1 / (s1 * s1)) + r * T(1 / (s2 * s2))) / (T(1) + r)).astype(T)


def _logp_terms(case, w, T):
    if not case.mixture:
        sp = case.prior_init[0]
        return (T(C0 - np.log(sp)) - w * w * T(1 / (2 * sp * sp))).astype(T)
    pi, s1, s2 = case.prior_init[0], np.exp(case.prior_init[1]), np.exp(case.prior_init[2])
    l1 = T(np.log(pi) + C0 - np.log(s1)) - w * w * T(1 / (2 * s1 * s1))
    l2 = T(np.log(1 - pi) + C0 - np.log(s2)) - w * w * T(1 / (2 * s2 * s2))
    return np.logaddexp(l1, l2).astype(T)


def _mlp_np(x, w1, b1, w2, b2, w3, b3):
    a1 = x @ w1.T + b1
    h1 = np.maximum(a1, 0)
    a2 = h1 @ w2.T + b2
    h2 = np.maximum(a2, 0)
    return (h2 @ w3.T + b3)[:, 0], a1, a2, h1, h2


def _backward_np(x, dz, a1, a2, h1, h2, w2, w3):
    """The six gradients of sum_b dz_b z_b's loss through Linear-ReLU-Linear-ReLU-Linear (numpy's own summation order)."""
    g3, gb3 = dz[None, :] @ h2, dz.sum(keepdims=True)
    dh2 = np.where(a2 > 0, dz[:, None] * w3, 0).astype(x.dtype)
    g2, gb2 = dh2.T @ h1, dh2.sum(0)
    dh1 = np.where(a1 > 0, dh2 @ w2, 0).astype(x.dtype)
    return [dh1.T @ x, dh1.sum(0), g2, gb2, g3, gb3]


def gradients_closed(case, ps, x, y, beta, eps, T):
    """The gradients by hand in dtype T (F7: the header's closed form g_mu = sum t_s, g_rho = (sum t_s eps_s - beta / sigma)
    sigmoid(rho)): what the float64 autograd side is checked against, and the fp32 restatement's gradients."""
    x, y = np.asarray(x, T), np.asarray(y, T)
    if case.kind == "f6":
        z, a1, a2, h1, h2 = _mlp_np(x, *ps)
        r = z - y
        return _backward_np(x, T(2) * r, a1, a2, h1, h2, ps[2], ps[4]), dict(loss=(r * r).sum(), z=z[None])
    S = case.S
    inv_s, beta = T(1.0 / S), T(beta)
    sig = [np.log1p(np.exp(ps[2 * q + 1])).astype(T) for q in range(6)]
    G = [np.zeros_like(ps[2 * q]) for q in range(6)]
    Hh = [np.zeros_like(ps[2 * q]) for q in range(6)]
    lq = lp = nll = T(0)
    zs = []
    for s in range(S):
        es = [np.asarray(eps[q][s], T).reshape(ps[2 * q].shape) for q in range(6)]
        ws = [(ps[2 * q] + sig[q] * es[q]).astype(T) for q in range(6)]
        z, a1, a2, h1, h2 = _mlp_np(x, *ws)
        r = z - y
        gl = _backward_np(x, r * inv_s, a1, a2, h1, h2, ws[2], ws[4])
        for q in range(6):
            t = (gl[q].reshape(ws[q].shape) - beta * inv_s * _dlogp(case, ws[q], T)).astype(T)
            G[q] = G[q] + t
            Hh[q] = Hh[q] + t * es[q]
            lq = lq + (T(C0) - np.log(sig[q]) - T(0.5) * es[q] * es[q]).sum(dtype=T)
            lp = lp + _logp_terms(case, ws[q], T).sum(dtype=T)
        nll = nll + (T(0.5) * r * r - T(C0)).sum(dtype=T)
        zs.append(z)
    g = []
    for q in range(6):
        g.append(G[q])
        g.append(((Hh[q] - beta / sig[q]) * _sigmoid(ps[2 * q + 1], T)).astype(T))
    m_lq, m_lp, m_nll = lq * inv_s, lp * inv_s, nll * inv_s
    return g, dict(loss_info=np.array([beta * m_lq - beta * m_lp + m_nll, m_lp, m_lq, m_nll], T), z=np.stack(zs))


def step32(case: Case, inp, eps_fn=None):
    """The launch restated in numpy float32 (closed-form gradients, numpy's summation order, the kernels' fp32 scalars)."""
    f7 = case.kind == "f7"
    eps_fn = eps_fn or (oracle_eps(case) if f7 else None)
    p, m, v = list(inp["params"]), list(inp["exp_avg"]), list(inp["exp_avg_sq"])
    zs, info = [], None
    for j in range(case.nb):
        eps = _eps_lists(case, eps_fn, case.counter + j * case.S) if f7 else None
        g, info = gradients_closed(case, p, inp["slab"][j], inp["targets"][j], F32(case.kl[j]), eps, F32)
        assert all(a.dtype == F32 for a in g)
        for i in range(len(p)):
            p[i], m[i], v[i] = adam(p[i], m[i], v[i], g[i].reshape(p[i].shape), case.step0 + j + 1, float(F32(case.lr)),
                                    case.betas, case.eps, case.wd, F32)
        zs.append(info["z"])
    out = dict(params=p, exp_avg=m, exp_avg_sq=v, z=np.stack(zs))
    out.update({k: info[k] for k in info if k != "z"})
    return out


def forward32(case: Case, inp, eps_fn=None):
    ps, x = inp["params"], inp["rows"]
    if case.kind == "f6":
        return dict(z=_mlp_np(x, *ps)[0][None])
    if case.zero_eps:
        return dict(z=_mlp_np(x, *ps[0::2])[0][None])
    eps = _eps_lists(case, eps_fn or oracle_eps(case), case.counter)
    zs = []
    for s in range(case.S):
        ws = [(ps[2 * q] + np.log1p(np.exp(ps[2 * q + 1])) * eps[q][s].astype(F32).reshape(ps[2 * q].shape)).astype(F32)
              for q in range(6)]
        zs.append(_mlp_np(x, *ws)[0])
    return dict(z=np.stack(zs))


# ---------------------------------------------------------------------------------------------------------------- bounds
def rel_dev(got, want):
    """max |got - want| relative to max |want| (float64)."""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64).reshape(want.shape) - want).max()) / max(float(np.abs(want).max()), 1e-30)


def deviations(got, ref, classes=CLASSES):
    """Per class, the largest rel_dev over the class's tensors: got / ref as step64 / step32 / forward* return them."""
    out = {}
    for c in classes:
        if c == "outputs":
            out[c] = rel_dev(got["z"], ref["z"])
        elif c in got:
            out[c] = max(rel_dev(a, b) for a, b in zip(got[c], ref[c]))
    return out


def d_ref(case: Case, inp, ref=None, eps_fn=None, train=True):
    """The fp32 restatement's deviation from the float64 reference, per class: computed from the reference side alone."""
    if train:
        ref = ref if ref is not None else step64(case, inp, eps_fn)
        return deviations(step32(case, inp, eps_fn), ref)
    ref = ref if ref is not None else forward64(case, inp, eps_fn)
    return deviations(forward32(case, inp, eps_fn), ref, ("outputs",))


def bounds(case: Case, dref):
    return {c: bound(d, FLOOR_OPS[case.kind][c]) for c, d in dref.items()}


def gate_margin(ref):
    """Per hidden layer, the smallest |pre-activation| over every step, draw and row, relative to the layer's max |.|."""
    return tuple(float(np.abs(ref[k]).min()) / float(np.abs(ref[k]).max()) for k in ("pre1", "pre2"))


def gate_margin_ok(ref, d_ref_outputs):
    return all(g > 100.0 * d_ref_outputs for g in gate_margin(ref))


# The scalar words.  They are sums over the outputs (and F7's over the parameters), so their bounds follow from the classes':
#   F6 loss = sum r^2, r = z - y: an output deviation dz moves it by at most 2 sum |r| dz, and the kernel's own B + 1 roundings
#     (the subtraction, an fma chain of B) by (B + 1) 2^-23 loss.
#   F7 nll = mean_s sum (r^2 / 2 - c0): sum |r| dz from the outputs (abs_r: the mean over s of sum |r|), B + 3 roundings of sum |term|.
#   F7 log_q, log_p: sums over the six tensors' elements; a thread adds 4 ceil(groups / 512) terms of each tensor (groups: its
#     Philox groups of four), then 6 + 8 tree levels and the S draws, each term 4 roundings (softplus, the log, the fma):
#     (depth + 4) 2^-23 sum |term|; from the second minibatch on the parameters differ
#     by their class's bound, which moves every term by about that fraction of it (tests/test_gpu_bnn_bandit_group.py).
def loss_tolerance(case: Case, inp, ref, bnds):
    dz = bnds["outputs"] * float(np.abs(ref["z"][-1]).max())
    B = case.B
    if case.kind == "f6":
        r = ref["z"][-1, 0] - inp["targets"][-1].astype(F64)
        return 2 * float(np.abs(r).sum()) * dz + (B + 1) * ULP * abs(ref["loss"])
    groups = [(s[0] if len(s) == 2 else 1) * -(-s[-1] // 4) for s in shapes(case)[0::2]]
    depth = sum(4 * -(-g // 512) for g in groups) + 14 + case.S
    carried = bnds["params"] if case.nb > 1 else 0.0
    tq, tp = (((depth + 4) * ULP + carried) * ref[k] for k in ("abs_q", "abs_p"))
    nll_terms = float(ref["loss_info"][3])                         # every term is positive
    tn = ref["abs_r"] * dz + (B + 3) * ULP * nll_terms
    beta = float(F32(case.kl[case.nb - 1]))
    return np.array([beta * (tq + tp) + tn, tp, tq, tn])
