"""numpy fp64 restatement of the Flipout estimator (include/bnn_hip.h F16): the sign stream, the layer forward, the ELBO terms
at the base draw and the backward closed forms.  tests/test_flipout_cpu.py checks the restatement against the per-row dense
form and torch's CPU autograd of it; tests/test_gpu_flipout.py checks the kernels against the restatement."""
import math

import numpy as np

from oracle import bnn_oracle as O

C0 = -0.5 * math.log(2.0 * math.pi)


def signs(seed, layer_id, kind, gsample, rows, cols, row_offset=0):
    """int8 [rows, cols] of +1 / -1: group = (row_offset + row) * ceil(cols / 128) + (col >> 7), counter word 3 = 2,
    bit (b & 31) of word b >> 5, b = col & 127."""
    gpr = (cols + 127) // 128
    row = np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(row_offset)
    grp = ((row * np.uint64(gpr) + np.arange(gpr, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w = O.philox4x32(grp, np.uint32(gsample & 0xFFFFFFFF), np.uint32(4 * layer_id + kind), np.uint32(2),
                     seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1)                                   # [rows, gpr, 4]
    col = np.arange(cols)
    b = col & 127
    word = words[:, col >> 7, b >> 5]                              # [rows, cols]
    bit = (word >> (b & 31).astype(np.uint32)[None, :]) & np.uint32(1)
    return np.where(bit == 1, -1, 1).astype(np.int8)


def sign_block(seed, layer_id, kind, first_sample, n_samples, rows, cols, row_offset=0):
    return np.stack([signs(seed, layer_id, kind, first_sample + i, rows, cols, row_offset) for i in range(n_samples)])


def softplus(rho):
    return np.log1p(np.exp(np.asarray(rho, np.float64)))


def forward(x, mu, delta, b, r, s, relu):
    """y[s, n, o] = act(sum_k x mu + s * sum_k (x r) Delta_d + b_d);  x [B, K] or [S, B, K], delta [D, N, K], b [D, N],
    r [S, B, K], s [S, B, N].  Returns (y, pre-activation)."""
    x, mu, delta, b = (np.asarray(t, np.float64) for t in (x, mu, delta, b))
    S, D = r.shape[0], delta.shape[0]
    xs = np.broadcast_to(x, (S,) + x.shape[-2:])
    pre = np.empty((S, xs.shape[1], mu.shape[0]))
    for i in range(S):
        d = i // (S // D)
        pre[i] = xs[i] @ mu.T + s[i] * ((xs[i] * r[i]) @ delta[d].T) + b[d]
    return (np.maximum(pre, 0.0) if relu else pre), pre


def forward_dense(x, mu, delta, b, r, s, relu):
    """The definition, row by row: y_n = x_n (mu + Delta o (s_n r_n^T))^T + b."""
    x, mu, delta, b = (np.asarray(t, np.float64) for t in (x, mu, delta, b))
    S, D = r.shape[0], delta.shape[0]
    xs = np.broadcast_to(x, (S,) + x.shape[-2:])
    y = np.empty((S, xs.shape[1], mu.shape[0]))
    for i in range(S):
        d = i // (S // D)
        for n in range(xs.shape[1]):
            w = mu + delta[d] * np.outer(s[i, n], r[i, n])
            y[i, n] = w @ xs[i, n] + b[d]
    return np.maximum(y, 0.0) if relu else y


def bound(x, mu, delta, b, S, K):
    """(K + 8) 2^-24 (|x||mu|^T + |x||Delta_d|^T + |b_d|): any fp32 fma summation order stays inside it.  [S, B, N]."""
    x, mu, delta, b = (np.abs(np.asarray(t, np.float64)) for t in (x, mu, delta, b))
    D = delta.shape[0]
    xs = np.broadcast_to(x, (S,) + x.shape[-2:])
    return np.stack([(K + 8) * 2.0 ** -24 * (xs[i] @ mu.T + xs[i] @ delta[i // (S // D)].T + b[i // (S // D)]) for i in range(S)])


def log_q(eps_w, eps_b, sigma_w, sigma_b):
    n = eps_w.size + eps_b.size
    return n * C0 - np.log(sigma_w).sum() - np.log(sigma_b).sum() - 0.5 * ((eps_w ** 2).sum() + (eps_b ** 2).sum())


def _log_normal(w, sd):
    return C0 - math.log(sd) - w ** 2 / (2.0 * sd * sd)


def log_prior(w, b, prior):
    """prior: ("gauss", sigma_p) or ("mixture", pi, sigma1, sigma2)."""
    if prior[0] == "gauss":
        return _log_normal(w, prior[1]).sum() + _log_normal(b, prior[1]).sum()
    _, pi, s1, s2 = prior
    f = lambda t: np.log(pi * np.exp(_log_normal(t, s1)) + (1.0 - pi) * np.exp(_log_normal(t, s2))).sum()
    return f(w) + f(b)


def dlogp(w, prior):
    if prior[0] == "gauss":
        return -w / prior[1] ** 2
    _, pi, s1, s2 = prior
    p1, p2 = pi * np.exp(_log_normal(w, s1)), (1.0 - pi) * np.exp(_log_normal(w, s2))
    return -w * (p1 / s1 ** 2 + p2 / s2 ** 2) / (p1 + p2)


def elbo_terms(mu, rho, b_mu, b_rho, eps_w, eps_b, prior):
    """(log_prior[D], log_q[D]) at the base draws; fp64 throughout."""
    mu, rho, b_mu, b_rho, eps_w, eps_b = (np.asarray(t, np.float64) for t in (mu, rho, b_mu, b_rho, eps_w, eps_b))
    sw, sb = softplus(rho), softplus(b_rho)
    lp = np.array([log_prior(mu + sw * eps_w[d], b_mu + sb * eps_b[d], prior) for d in range(eps_w.shape[0])])
    lq = np.array([log_q(eps_w[d], eps_b[d], sw, sb) for d in range(eps_w.shape[0])])
    return lp, lq


def backward(x, gy, y, mu, rho, b_mu, b_rho, eps_w, eps_b, r, s, prior, relu, glp=None, glq=None):
    """The closed forms of include/bnn_hip.h F16: (g_mu, g_rho, g_b_mu, g_b_rho, g_x [S, B, K])."""
    x, gy, mu, rho, b_mu, b_rho, eps_w, eps_b = (np.asarray(t, np.float64) for t in (x, gy, mu, rho, b_mu, b_rho, eps_w, eps_b))
    S, D = r.shape[0], eps_w.shape[0]
    spd = S // D
    glp = np.zeros(D) if glp is None else np.asarray(glp, np.float64)
    glq = np.zeros(D) if glq is None else np.asarray(glq, np.float64)
    sw, sb = softplus(rho), softplus(b_rho)
    xs = np.broadcast_to(x, (S,) + x.shape[-2:])
    gz = gy * (np.asarray(y) > 0) if relu else gy
    G = sum(gz[i].T @ xs[i] for i in range(S))
    g_mu, racc = G.copy(), np.zeros_like(mu)
    g_bmu, bracc = np.zeros_like(b_mu), np.zeros_like(b_mu)
    gx = np.empty((S,) + xs.shape[1:])
    for d in range(D):
        delta = sw * eps_w[d]
        H = sum((gz[i] * s[i]).T @ (xs[i] * r[i]) for i in range(d * spd, (d + 1) * spd))
        pr = glp[d] * dlogp(mu + delta, prior)
        g_mu += pr
        racc += (H + pr) * eps_w[d]
        t = sum(gz[i].sum(0) for i in range(d * spd, (d + 1) * spd)) + glp[d] * dlogp(b_mu + sb * eps_b[d], prior)
        g_bmu += t
        bracc += t * eps_b[d]
        for i in range(d * spd, (d + 1) * spd):
            gx[i] = gz[i] @ mu + ((gz[i] * s[i]) @ delta) * r[i]
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    g_rho = (racc - glq.sum() / sw) * sig(rho)
    g_brho = (bracc - glq.sum() / sb) * sig(b_rho)
    return g_mu, g_rho, g_bmu, g_brho, gx


# ---------------------------------------------------------------------------------------------- three-layer network
def nll_and_grad(logits, target, mode, sigma=1.0):
    """(nll[S], d sum_s nll_s / d logits) in fp64: cross-entropy summed over the batch, or the Gaussian NLL of the reference."""
    logits = np.asarray(logits, np.float64)
    if mode == "classification":
        z = logits - logits.max(-1, keepdims=True)
        lse = np.log(np.exp(z).sum(-1, keepdims=True))
        logp = z - lse
        t = np.asarray(target).astype(np.int64)
        onehot = np.eye(logits.shape[-1])[t]
        return -(logp * onehot[None]).sum((1, 2)), np.exp(logp) - onehot[None]
    t = np.asarray(target, np.float64).reshape(logits.shape[1:])
    diff = logits - t[None]
    const = -C0 + math.log(sigma)
    return (diff ** 2 / (2.0 * sigma ** 2) + const).sum((1, 2)), diff / sigma ** 2


def network(params, x, eps, seed, first_sample, S, D, prior, mode, target, beta, sigma=1.0, round_bf16=None):
    """Forward + ELBO + backward of the three-layer net.  params: [(mu, rho, b_mu, b_rho)] per layer (fp32 arrays); eps:
    [(eps_w [D, N, K], eps_b [D, N])].  Returns dict(logits, loss, log_prior, log_q, nll, grads [4 per layer], g_x).
    round_bf16: optional callable applied to every matmul operand (x / hidden activations, mu, Delta) -- the bf16 math."""
    rb = round_bf16 if round_bf16 is not None else (lambda t: t)
    B = x.shape[0]
    h, saved = np.asarray(x, np.float64), []
    lp, lq = np.zeros(D), np.zeros(D)
    for li, ((mu, rho, bm, br), (ew, eb)) in enumerate(zip(params, eps)):
        N, K = mu.shape
        r = sign_block(seed, li, 0, first_sample, S, B, K)
        s = sign_block(seed, li, 1, first_sample, S, B, N)
        sw32 = softplus(rho).astype(np.float32)
        delta = (sw32 * np.asarray(ew, np.float32)).astype(np.float32) if round_bf16 is not None else softplus(rho) * np.asarray(ew, np.float64)
        b = np.asarray(bm, np.float64) + softplus(br) * np.asarray(eb, np.float64)
        relu = li < len(params) - 1
        y, _ = forward(rb(h), rb(mu), rb(delta), b, r, s, relu)
        a, c = elbo_terms(mu, rho, bm, br, ew, eb, prior)
        lp, lq = lp + a, lq + c
        saved.append((h, y, r, s))
        h = y
    nll, g = nll_and_grad(h, target, mode, sigma)
    out = dict(logits=h, log_prior=lp.mean(), log_q=lq.mean(), nll=nll.mean())
    out["loss"] = beta * out["log_q"] - beta * out["log_prior"] + out["nll"]
    g = g / S
    grads = [None] * len(params)
    for li in reversed(range(len(params))):
        mu, rho, bm, br = params[li]
        ew, eb = eps[li]
        hin, y, r, s = saved[li]
        relu = li < len(params) - 1
        res = backward(hin, g, y, mu, rho, bm, br, ew, eb, r, s, prior, relu, glp=np.full(D, -beta / D), glq=np.full(D, beta / D))
        grads[li] = res[:4]
        g = res[4]
    out["grads"] = grads
    out["g_x"] = g.sum(0)
    return out
