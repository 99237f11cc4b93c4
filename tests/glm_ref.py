"""fp64 restatement of the linearised (GLM) predictive of the diagonal Laplace posterior (include/bnn_hip.h F18;
csrc/laplace.hip) in numpy, stage by stage as the kernels cut the work -- V, the tile partials and their sum, the finish
(covariance, Cholesky factor, probit, quantiles), the logit sampler on the Philox stream (5, 1) -- plus an INDEPENDENT form,
J diag(s^2) J^T from per-row autograd Jacobians, that tests/test_glm_cpu.py holds the restatement against."""
import math
import statistics

import numpy as np
import torch

import laplace_ref as R
from oracle import bnn_oracle as O

TILE = 64
MAX_CLASSES = 16
STREAM = (5, 1)                                                # counter words 2 and 3 of the sampler's stream


def variance(f, tau):
    """s^2 = 1 / (F + tau)."""
    return 1.0 / (np.asarray(f, dtype=np.float64) + float(tau))


def pairs(C):
    """[(c, c')] with c <= c' in the kernels' order: pair = c' (c' + 1) / 2 + c."""
    return [(c, cb) for cb in range(C) for c in range(cb + 1)]


def v_of(x, f_w, f_b, tau):
    """V [B, out] = x^2 . (s^2_w)^T + s^2_b."""
    x = np.asarray(x, dtype=np.float64)
    return x ** 2 @ variance(f_w, tau).T + variance(f_b, tau)[None, :]


def gz_of(gy, y_saved, B):
    """(gz [C, B, out], active [B, out]): the deltas of virtual row c B + n, and where the saved output lets them through."""
    gy = np.asarray(gy, dtype=np.float64)
    Rr, out = gy.shape
    gz = gy.reshape(Rr // B, B, out)
    active = np.ones((B, out), dtype=bool) if y_saved is None else np.asarray(y_saved) > 0
    return gz, active


def layer_parts(gy, y_saved, V, B):
    """cov_part [ceil(out / 64), B, pairs]: per 64-column tile, sum over its ACTIVE columns of gz_c gz_c' V (an inactive
    column is left out, not multiplied by zero: a non-finite V[n, o] reaches only the rows whose unit o is active)."""
    gz, active = gz_of(gy, y_saved, B)
    C, _, out = gz.shape
    V = np.asarray(V, dtype=np.float64)
    tiles = (out + TILE - 1) // TILE
    part = np.zeros((tiles, B, len(pairs(C))))
    for t in range(tiles):
        sl = slice(t * TILE, min(out, (t + 1) * TILE))
        for p, (c, cb) in enumerate(pairs(C)):
            term = np.where(active[:, sl], gz[c][:, sl] * gz[cb][:, sl] * V[:, sl], 0.0)
            part[t, :, p] = term.sum(axis=1)
    return part


def sum_parts(parts):
    """a [B, pairs]: every layer's partials, every tile."""
    return sum(np.asarray(p, dtype=np.float64).sum(axis=0) for p in parts)


def unpack(a, C):
    """cov [B, C, C] from the lower-triangle pairs."""
    B = a.shape[0]
    cov = np.zeros((B, C, C))
    for p, (c, cb) in enumerate(pairs(C)):
        cov[:, cb, c] = a[:, p]
        cov[:, c, cb] = a[:, p]
    return cov


def cholesky(cov):
    """The lower factor per row; a row that is not positive definite (or not finite) is all NaN below and on the diagonal."""
    out = np.zeros_like(cov)
    for n, m in enumerate(cov):
        try:
            if not np.isfinite(m).all():
                raise np.linalg.LinAlgError
            out[n] = np.linalg.cholesky(m)
        except np.linalg.LinAlgError:
            out[n] = np.where(np.tri(m.shape[0], dtype=bool), np.nan, 0.0)
    return out


def probit(mean, var):
    """(probs, preds, entropy) of MacKay's approximation softmax(mean / sqrt(1 + pi / 8 var))."""
    t = np.asarray(mean, dtype=np.float64) / np.sqrt(1.0 + math.pi / 8.0 * np.asarray(var, dtype=np.float64))
    p = R.softmax(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(p == 0.0, 0.0, p * np.log(p)).sum(axis=1)
    return p, np.argmax(p, axis=1), h


def normal_z(levels):
    nd = statistics.NormalDist()
    return np.array([-math.inf if q == 0.0 else math.inf if q == 1.0 else nd.inv_cdf(q) for q in levels], dtype=np.float64)


def finish(parts, mean, mode, sigma=1.0, levels=()):
    """dict(cov, var, chol, and probs / preds / entropy or predictive_variance / quantiles [Q, B, C])."""
    mean = np.asarray(mean, dtype=np.float64)
    C = mean.shape[1]
    cov = unpack(sum_parts(parts), C)
    var = np.einsum("ncc->nc", cov).copy()
    out = dict(cov=cov, var=var, chol=cholesky(cov))
    if mode == "classification":
        out["probs"], out["preds"], out["entropy"] = probit(mean, var)
    else:
        out["predictive_variance"] = var + sigma ** 2
        with np.errstate(invalid="ignore"):
            out["quantiles"] = mean[None] + normal_z(levels)[:, None, None] * np.sqrt(var)[None]
    return out


# ------------------------------------------------------------------------------------------------------------ the sampler
def glm_eps(seed, g, B, C):
    """eps [B, C] (float32) of global sample g: element (n, j) in group n * ceil(C / 4) + (j >> 2), slot j & 3, counter
    (group, g, 5, 1) -- oracle.bnn_oracle.philox_normal's map with the sampler's counter words."""
    gpr = (C + 3) // 4
    grp = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(gpr) + np.arange(gpr, dtype=np.uint64)[None, :]).astype(np.uint32)
    r0, r1, r2, r3 = O.philox4x32(grp, np.uint32(int(g) & 0xFFFFFFFF), np.uint32(STREAM[0]), np.uint32(STREAM[1]),
                                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    n0, n1 = O.box_muller(r0, r1)
    n2, n3 = O.box_muller(r2, r3)
    return np.ascontiguousarray(np.stack([n0, n1, n2, n3], axis=-1).reshape(B, gpr * 4)[:, :C])


def sample(mean, chol, seed, first, S):
    """(f [S, B, C], mag [S, B, C]) in fp64: f = mean + chol . eps over the global samples first ... first + S - 1, and
    mag = |mean| + sum_j |chol_cj| |eps_j|, what a rounding-error bound of the fmaf chain scales with."""
    mean, chol = np.asarray(mean, dtype=np.float64), np.asarray(chol, dtype=np.float64)
    B, C = mean.shape
    eps = np.stack([glm_eps(seed, first + s, B, C) for s in range(S)]).astype(np.float64)
    f = mean[None] + np.einsum("ncj,snj->snc", chol, eps)
    mag = np.abs(mean)[None] + np.einsum("ncj,snj->snc", np.abs(chol), np.abs(eps))
    return f, mag


# ------------------------------------------------------------------------------------------------------------ the chain
def chain(weights, curv, tau, x, dtype=np.float64):
    """(mean [B, C], cov [B, C, C], parts per layer) of the layer-wise form: the forward, the seed gy[c B + n, k] = delta_kc,
    then top down V, the partials and g_x = gz . W masked by the layer's input.  curv: [F_w0, F_b0, F_w1, ...]."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    acts = R.forward(weights, x)
    C = acts[-1].shape[1]
    g = np.zeros((C, B, C))
    for c in range(C):
        g[c, :, c] = 1.0
    g = g.reshape(C * B, C)
    parts = [None] * len(weights)
    for i in range(len(weights) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        saved = acts[i] if i + 1 < len(weights) else None
        parts[i] = layer_parts(g, saved, v_of(xin, curv[2 * i], curv[2 * i + 1], tau), B)
        if i > 0:
            gz, active = gz_of(g, saved, B)
            g = np.where(active[None], gz, 0.0).reshape(C * B, -1) @ np.asarray(weights[i][0], dtype=np.float64)
            g = np.where(np.tile(xin > 0, (C, 1)), g, 0.0)
    return acts[-1], unpack(sum_parts(parts), C), parts


def chain_torch32(weights, curv, tau, x):
    """The same layer-wise formula in plain fp32 torch CPU ops: cov [B, C, C] (float32)."""
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
    C = acts[-1].shape[1]
    g = torch.eye(C)[:, None, :].expand(C, B, C).reshape(C * B, C)
    cov = torch.zeros((B, C, C))
    for i in range(len(ws) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        V = xin ** 2 @ (1.0 / (T(curv[2 * i]) + tau)).T + 1.0 / (T(curv[2 * i + 1]) + tau)
        gz = g.reshape(C, B, -1)
        if i + 1 < len(ws):
            gz = torch.where((acts[i] > 0)[None], gz, torch.zeros(()))
        cov += torch.einsum("cno,dno,no->ncd", gz, gz, V)
        if i > 0:
            g = gz.reshape(C * B, -1) @ ws[i][0]
            g = torch.where((xin > 0).repeat(C, 1), g, torch.zeros(()))
    return cov


def jacobian_cov(weights, curv, tau, x, dtype=torch.float64):
    """(mean, cov) from per-row Jacobians J_n = d f(x_n) / d theta by autograd: cov_n = J_n diag(1 / (F + tau)) J_n^T."""
    f, flat = R._torch_net(weights, dtype)
    s2 = torch.tensor(np.concatenate([variance(c, tau).reshape(-1) for c in curv]), dtype=dtype)
    xs = torch.tensor(np.asarray(x), dtype=dtype)
    mean, cov = [], []
    for n in range(xs.shape[0]):
        J = torch.autograd.functional.jacobian(lambda th: f(th, xs[n]), flat)           # [C, P]
        mean.append(f(flat, xs[n]).numpy())
        cov.append(((J * s2[None, :]) @ J.T).numpy())
    return np.stack(mean), np.stack(cov)
