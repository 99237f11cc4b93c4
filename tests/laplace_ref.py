"""fp64 restatement of the diagonal Laplace stages (include/bnn_hip.h F17; csrc/laplace.hip) in numpy, stage by stage as the
kernels cut the work, plus an INDEPENDENT formulation (per-row Jacobians by torch.autograd.functional.jacobian, the GGN from
diag(p) - p p^T itself, the evidence from slogdet of the dense diagonal precision) that tests/test_laplace_cpu.py holds the
restatement against.  The GPU tests compare each kernel with the restated stage computed from the kernel's own inputs."""
import math

import numpy as np
import torch

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------ the four stages
def seed(z, target, mode, curvature, sigma=1.0):
    """(gy [R, C], log-likelihood sum or None): virtual row r = c * B + n under 'ggn' (R = B * C), r = n under 'empirical'.
    A label outside [0, C) makes its row's deltas and the log-likelihood NaN."""
    z = np.asarray(z, dtype=np.float64)
    B, C = z.shape
    ll = None
    if mode == "classification":
        p = softmax(z)
        ok = None
        if target is not None:
            t = np.asarray(target).astype(np.int64)
            ok = (t >= 0) & (t < C)
            lse = z.max(axis=1) + np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1))
            ll = np.where(ok, z[np.arange(B), np.where(ok, t, 0)] - lse, np.nan).sum()
        if curvature == "ggn":
            gy = np.empty((C, B, C))
            for c in range(C):
                e = np.zeros(C)
                e[c] = 1.0
                gy[c] = np.sqrt(p[:, c])[:, None] * (e[None, :] - p)
        else:
            onehot = np.zeros((B, C))
            onehot[np.arange(B), np.where(ok, t, 0)] = 1.0
            gy = (p - onehot)[None]
        if ok is not None:
            gy[:, ~ok, :] = np.nan
        return gy.reshape(-1, C), ll
    y = None if target is None else np.asarray(target, dtype=np.float64).reshape(B, C)
    if y is not None:
        ll = (-0.5 * ((z - y) / sigma) ** 2 - math.log(sigma) - HALF_LOG_2PI).sum()
    if curvature == "ggn":
        gy = np.zeros((C, B, C))
        for c in range(C):
            gy[c, :, c] = 1.0 / sigma
        return gy.reshape(-1, C), ll
    return (z - y) / sigma ** 2, ll


def layer(x, gy, y_saved, w, gx_mask=False, want_gx=True):
    """One Linear -> [ReLU] group: (S [B, out], dF_w [out, in], dF_b [out], g_x [R, in] | None).  gz = gy where the saved
    output of data row r mod B is positive (y_saved None: everywhere); S sums gz^2 over the virtual rows of a data row."""
    x, gy, w = (np.asarray(a, dtype=np.float64) for a in (x, gy, w))
    B = x.shape[0]
    R, out = gy.shape
    C = R // B
    gz = gy.reshape(C, B, out)
    if y_saved is not None:
        gz = np.where((np.asarray(y_saved) > 0)[None], gz, 0.0)
    S = (gz ** 2).sum(axis=0)
    gx = None
    if want_gx:
        gx = gz.reshape(R, out) @ w
        if gx_mask:
            gx = np.where(np.tile(x > 0, (C, 1)), gx, 0.0)
    return S, S.T @ (x ** 2), S.sum(axis=0), gx


def evidence(params, curvs, taus, loglik):
    """log_evidence[g] = loglik - tau |w|^2 / 2 + P log(tau) / 2 - sum log(F + tau) / 2."""
    w = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])
    f = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in curvs])
    taus = np.asarray(taus, dtype=np.float64)
    return np.array([loglik - 0.5 * t * (w ** 2).sum() + 0.5 * w.size * math.log(t) - 0.5 * np.log(f + t).sum() for t in taus])


def best_precision(log_ev):
    """(index of the maximum, relative gap to the runner-up): the caller asserts the gap before trusting the index."""
    order = np.argsort(-log_ev, kind="stable")
    gap = (log_ev[order[0]] - log_ev[order[1]]) / abs(log_ev[order[0]]) if len(order) > 1 else np.inf
    return int(order[0]), gap


def posterior_sigma(f, tau):
    return (np.asarray(f, dtype=np.float64) + tau) ** -0.5


def softplus(rho):
    rho = np.asarray(rho, dtype=np.float64)
    return np.maximum(rho, 0.0) + np.log1p(np.exp(-np.abs(rho)))


def inv_softplus(s):
    s = np.asarray(s, dtype=np.float64)
    return np.where(s > 40.0, s, np.log(np.expm1(np.minimum(s, 40.0))))


# ------------------------------------------------------------------------------------------------------------ the chain
def forward(weights, x):
    """(activations after each group, the last one the logits) of an MLP given as [(W [out, in], b [out]), ...] with ReLU
    between the layers."""
    h, acts = np.asarray(x, dtype=np.float64), []
    for i, (w, b) in enumerate(weights):
        h = h @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if i + 1 < len(weights):
            h = np.maximum(h, 0.0)
        acts.append(h)
    return acts


def accumulate(weights, x, target, mode, curvature, sigma=1.0):
    """One minibatch through the restated stages: ([dF_w0, dF_b0, dF_w1, ...], log-likelihood)."""
    x = np.asarray(x, dtype=np.float64)
    acts = forward(weights, x)
    g, ll = seed(acts[-1], target, mode, curvature, sigma)
    out = [None] * (2 * len(weights))
    for i in range(len(weights) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        relu = i + 1 < len(weights)
        _, fw, fb, gx = layer(xin, g, acts[i] if relu else None, weights[i][0], gx_mask=i > 0, want_gx=i > 0)
        out[2 * i], out[2 * i + 1] = fw, fb
        g = gx
    return out, ll


# ------------------------------------------------------------------------------------------------------------ independent form
def _torch_net(weights, dtype):
    ws = [(torch.tensor(np.asarray(w), dtype=dtype), torch.tensor(np.asarray(b), dtype=dtype)) for w, b in weights]

    def f(flat, xrow):
        h, at = xrow, 0
        for i, (w, b) in enumerate(ws):
            W = flat[at:at + w.numel()].view(w.shape)
            at += w.numel()
            bb = flat[at:at + b.numel()]
            at += b.numel()
            h = W @ h + bb
            if i + 1 < len(ws):
                h = torch.relu(h)
        return h
    flat = torch.cat([t.reshape(-1) for w, b in ws for t in (w, b)])
    return f, flat


def jacobian_curvature(weights, x, target, mode, curvature, sigma=1.0, dtype=torch.float64):
    """The same diagonal from per-row Jacobians J_n = d logits / d theta (autograd) and the output Hessian itself:
    'ggn': diag(sum_n J_n^T H_n J_n) with H_n = diag(p) - p p^T (classification) or I / sigma^2 (regression);
    'empirical': sum_n (J_n^T d_n)^2 with d_n the gradient of the row's negative log-likelihood in the logits.
    Returns the flat diagonal in parameter order (W0, b0, W1, b1, ...)."""
    f, flat = _torch_net(weights, dtype)
    xs = torch.tensor(np.asarray(x), dtype=dtype)
    diag = torch.zeros_like(flat)
    for n in range(xs.shape[0]):
        J = torch.autograd.functional.jacobian(lambda th: f(th, xs[n]), flat)           # [C, P]
        z = f(flat, xs[n])
        if mode == "classification":
            p = torch.softmax(z, dim=0)
            H = torch.diag(p) - torch.outer(p, p)
            d = p.clone()
            if curvature == "empirical":
                d[int(target[n])] -= 1.0
        else:
            H = torch.eye(z.numel(), dtype=dtype) / sigma ** 2
            d = None if curvature != "empirical" else (z - torch.tensor(np.asarray(target, dtype=np.float64).reshape(xs.shape[0], -1)[n], dtype=dtype)) / sigma ** 2
        if curvature == "ggn":
            diag += torch.einsum("cp,cd,dp->p", J, H, J)
        else:
            diag += (J.T @ d) ** 2
    return diag.numpy()


def dense_evidence(params, curvs, tau, loglik):
    """The Laplace evidence from the dense form: log p(D | w) + log N(w; 0, I / tau) + P/2 log 2 pi - 1/2 log det(diag(F) + tau I)."""
    w = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in params])
    f = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1) for c in curvs])
    P = w.size
    log_prior = -0.5 * tau * (w ** 2).sum() + 0.5 * P * math.log(tau) - P * HALF_LOG_2PI
    sign, logdet = np.linalg.slogdet(np.diag(f + tau))
    assert sign > 0
    return loglik + log_prior + P * HALF_LOG_2PI - 0.5 * logdet


def fp32_chain_error(weights, x_batches, y_batches, mode, curvature, sigma=1.0):
    """Max-norm error (relative to the largest fp64 entry, per tensor; the maximum over the tensors) of a plain fp32 CPU torch
    evaluation of the restated chain against fp64, on the same inputs: what the end-to-end device check scales its bound by."""
    ref = None
    for x, y in zip(x_batches, y_batches):
        inc, _ = accumulate(weights, x, y, mode, curvature, sigma)
        ref = inc if ref is None else [a + b for a, b in zip(ref, inc)]
    got = None
    for x, y in zip(x_batches, y_batches):
        inc = accumulate_torch32(weights, x, y, mode, curvature, sigma)
        got = inc if got is None else [a + b for a, b in zip(got, inc)]
    return max(float(np.abs(g.double().numpy() - r).max() / np.abs(r).max()) for g, r in zip(got, ref)), ref


def accumulate_torch32(weights, x, target, mode, curvature, sigma=1.0):
    """The chain of accumulate() in fp32 torch CPU ops."""
    T = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    ws = [(T(w), T(b)) for w, b in weights]
    x = T(x)
    B = x.shape[0]
    h, acts = x, []
    for i, (w, b) in enumerate(ws):
        h = h @ w.T + b
        if i + 1 < len(ws):
            h = torch.relu(h)
        acts.append(h)
    z = acts[-1]
    C = z.shape[1]
    if mode == "classification":
        p = torch.softmax(z, dim=1)
        if curvature == "ggn":
            g = torch.stack([p[:, c].sqrt()[:, None] * (torch.eye(C)[c][None, :] - p) for c in range(C)]).reshape(-1, C)
        else:
            g = p - torch.eye(C)[torch.as_tensor(np.asarray(target)).long()]
    elif curvature == "ggn":
        g = torch.stack([torch.eye(C)[c][None, :].expand(B, C) / sigma for c in range(C)]).reshape(-1, C)
    else:
        g = (z - T(target).reshape(B, C)) / sigma ** 2
    out = [None] * (2 * len(ws))
    for i in range(len(ws) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        gz = g.reshape(-1, B, g.shape[1])
        if i + 1 < len(ws):
            gz = torch.where((acts[i] > 0)[None], gz, torch.zeros(()))
        S = (gz ** 2).sum(0)
        out[2 * i], out[2 * i + 1] = S.T @ xin ** 2, S.sum(0)
        if i > 0:
            g = gz.reshape(-1, gz.shape[2]) @ ws[i][0]
            g = torch.where((xin > 0).repeat(gz.shape[0], 1), g, torch.zeros(()))
    return out
