"""fp64 restatement of the Kronecker-factored Laplace stages (include/bnn_hip.h F20; csrc/kfac.hip) in numpy, cut as the
kernels cut the work, plus an INDEPENDENT formulation -- per-row Jacobians by torch.autograd, the dense per-layer precision
kron(G, Abar) / N + tau I (Wbar = [W | b] flattened row by row, so element (j, i) has index j (in + 1) + i), its slogdet, its
solve, and M M^T = P^-1 for the sampling map M = (Q_G (x) Q_A) diag(Sigma) -- that tests/test_kfac_cpu.py holds the
restatement against.  The GPU tests compare each kernel with the restated stage computed from the kernel's own inputs."""
import math

import numpy as np
import torch

import laplace_ref as R
from oracle import bnn_oracle as O

NOISE_WORD3 = 4


# ------------------------------------------------------------------------------------------------------------ the stages
def layer(x, gy, y_saved, w, gx_mask=False, want_gx=True):
    """One Linear -> [ReLU] group: (dA [in, in], ds [in], dG [out, out], g_x [R, in] | None)."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    B = x.shape[0]
    Rr, out = gy.shape
    gz = gy.reshape(Rr // B, B, out)
    if y_saved is not None:
        gz = np.where((np.asarray(y_saved) > 0)[None], gz, 0.0)
    gz = gz.reshape(Rr, out)
    gx = R.layer(x, gy, y_saved, w, gx_mask=gx_mask, want_gx=True)[3] if want_gx else None
    return x.T @ x, x.sum(axis=0), gz.T @ gz, gx


def accumulate(weights, x, target, mode, curvature, sigma=1.0):
    """One minibatch through the restated stages: ([(dA, ds, dG) per layer], log-likelihood)."""
    x = np.asarray(x, dtype=np.float64)
    acts = R.forward(weights, x)
    g, ll = R.seed(acts[-1], target, mode, curvature, sigma)
    out = [None] * len(weights)
    for i in range(len(weights) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        relu = i + 1 < len(weights)
        a, s, G, gx = layer(xin, g, acts[i] if relu else None, weights[i][0], gx_mask=i > 0, want_gx=i > 0)
        out[i] = (a, s, G)
        g = gx
    return out, ll


def add(total, inc):
    return inc if total is None else [tuple(a + b for a, b in zip(t, i)) for t, i in zip(total, inc)]


def abar_of(A, s, N):
    A, s = np.asarray(A, dtype=np.float64), np.asarray(s, dtype=np.float64)
    n = A.shape[0]
    m = np.empty((n + 1, n + 1))
    m[:n, :n], m[:n, n], m[n, :n], m[n, n] = A, s, s, N
    return m


def decompose(A, s, G, N):
    """(Q_A, lA, Q_G, lG): Abar / N = Q_A diag(lA) Q_A^T, G = Q_G diag(lG) Q_G^T, eigenvalues below 0 set to 0."""
    lA, QA = np.linalg.eigh(abar_of(A, s, N) / N)
    lG, QG = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    return QA, np.maximum(lA, 0.0), QG, np.maximum(lG, 0.0)


def evidence(weights, eigs, taus, loglik):
    """log_evidence[g] = loglik - tau |w|^2 / 2 + P log(tau) / 2 - 1/2 sum_l sum_ji log(lG_j lA_i + tau);
    eigs: (lA, lG) per layer."""
    w2 = sum((np.asarray(w, dtype=np.float64) ** 2).sum() + (np.asarray(b, dtype=np.float64) ** 2).sum() for w, b in weights)
    P = sum(np.asarray(w).size + np.asarray(b).size for w, b in weights)
    out = []
    for t in np.asarray(taus, dtype=np.float64):
        ld = sum(np.log(np.outer(lG, lA) + t).sum() for lA, lG in eigs)
        out.append(loglik - 0.5 * t * w2 + 0.5 * P * math.log(t) - 0.5 * ld)
    return np.array(out)


def glm_layer(x, gy, y_saved, QA, lA, QG, lG, tau):
    """(at [B, in + 1], gt [R, out], V [B, out], cov [B, C, C]) of one layer: at = [x | 1] Q_A, gt = gz Q_G,
    V = at^2 . D^T with D_ji = 1 / (lG_j lA_i + tau), cov[n, c, c'] = sum_j gt_cj gt_c'j V_nj."""
    x, gy = np.asarray(x, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    B = x.shape[0]
    Rr, out = gy.shape
    C = Rr // B
    gz = gy.reshape(C, B, out)
    if y_saved is not None:
        gz = np.where((np.asarray(y_saved) > 0)[None], gz, 0.0)
    at = np.concatenate([x, np.ones((B, 1))], axis=1) @ QA
    gt = gz.reshape(Rr, out) @ QG
    D = 1.0 / (np.outer(lG, lA) + tau)
    V = at ** 2 @ D.T
    g3 = gt.reshape(C, B, out)
    return at, gt, V, np.einsum("cnj,dnj,nj->ncd", g3, g3, V)


def glm_cov(weights, x, decs, tau):
    """(mean [B, C], cov [B, C, C]) of the linearised predictive: the chain of glm_layer top down, the deltas seeded with
    the identity (gy[c B + n, k] = delta_kc) as F18 does.  decs: decompose()'s tuple per layer."""
    x = np.asarray(x, dtype=np.float64)
    acts = R.forward(weights, x)
    B, C = acts[-1].shape
    g = np.zeros((C, B, C))
    for c in range(C):
        g[c, :, c] = 1.0
    g = g.reshape(C * B, C)
    cov = np.zeros((B, C, C))
    for i in range(len(weights) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        relu = i + 1 < len(weights)
        cov += glm_layer(xin, g, acts[i] if relu else None, *decs[i], tau)[3]
        if i > 0:
            g = R.layer(xin, g, acts[i] if relu else None, weights[i][0], gx_mask=True, want_gx=True)[3]
    return acts[-1], cov


def glm_cov_torch32(weights, x, decs, tau):
    """glm_cov()'s chain in fp32 torch CPU ops (eigenvectors and eigenvalues rounded to fp32 first): cov [B, C, C]."""
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
        QA, lA, QG, lG = (T(t) for t in decs[i])
        gz = g.reshape(C, B, -1)
        if i + 1 < len(ws):
            gz = torch.where((acts[i] > 0)[None], gz, torch.zeros(()))
        at = torch.cat([xin, torch.ones((B, 1))], dim=1) @ QA
        gt = (gz.reshape(C * B, -1) @ QG).reshape(C, B, -1)
        V = at ** 2 @ (1.0 / (torch.outer(lG, lA) + tau)).T
        cov += torch.einsum("cnj,dnj,nj->ncd", gt, gt, V)
        if i > 0:
            g = torch.where((xin > 0).repeat(C, 1), gz.reshape(C * B, -1) @ ws[i][0], torch.zeros(()))
    return cov


def noise(seed, sample, layer_index, out, in1):
    """E [out, in + 1] of one draw: element e = j (in + 1) + i from the Philox counter (e >> 2, sample, layer, 4), slot e & 3,
    through the oracle's Box-Muller."""
    n = out * in1
    groups = np.arange((n + 3) // 4, dtype=np.uint32)
    r0, r1, r2, r3 = O.philox4x32(groups, np.uint32(sample & 0xFFFFFFFF), np.uint32(layer_index), np.uint32(NOISE_WORD3),
                                  seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    n0, n1 = O.box_muller(r0, r1)
    n2, n3 = O.box_muller(r2, r3)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(-1)[:n].reshape(out, in1).astype(np.float64)


def sample(w, b, QA, lA, QG, lG, tau, E):
    """Wbar_s = Wbar + Q_G (E o Sigma) Q_A^T, Sigma_ji = (lG_j lA_i + tau)^-1/2 -> (W_s [out, in], b_s [out])."""
    wbar = np.concatenate([np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)[:, None]], axis=1)
    sig = (np.outer(lG, lA) + tau) ** -0.5
    ws = wbar + QG @ (np.asarray(E, dtype=np.float64) * sig) @ QA.T
    return ws[:, :-1], ws[:, -1]


def accumulate_torch32(weights, x, target, mode, curvature, sigma=1.0):
    """The chain of accumulate() in fp32 torch CPU ops: [(dA, ds, dG) per layer]."""
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
    out = [None] * len(ws)
    for i in range(len(ws) - 1, -1, -1):
        xin = x if i == 0 else acts[i - 1]
        gz = g.reshape(-1, B, g.shape[1])
        if i + 1 < len(ws):
            gz = torch.where((acts[i] > 0)[None], gz, torch.zeros(()))
        gz = gz.reshape(-1, gz.shape[2])
        out[i] = (xin.T @ xin, xin.sum(0), gz.T @ gz)
        if i > 0:
            g = torch.where((xin > 0).repeat(gz.shape[0] // B, 1), gz @ ws[i][0], torch.zeros(()))
    return out


def fp32_chain_error(weights, x_batches, y_batches, mode, curvature, sigma=1.0):
    """(max-norm error, relative to each tensor's largest fp64 entry, the maximum over the tensors, of the chain in plain fp32
    torch on the CPU against fp64; the fp64 factors): what the end-to-end device check scales its bound by."""
    ref = got = None
    for x, y in zip(x_batches, y_batches):
        ref = add(ref, accumulate(weights, x, y, mode, curvature, sigma)[0])
        got = add(got, accumulate_torch32(weights, x, y, mode, curvature, sigma))
    err = max(float(np.abs(g.double().numpy() - r).max() / np.abs(r).max()) for gl, rl in zip(got, ref) for g, r in zip(gl, rl))
    return err, ref


# ------------------------------------------------------------------------------------------------------------ independent form
def _layer_slices(weights):
    """Per layer the (weight, bias) column ranges of the flat parameter vector (W0, b0, W1, b1, ...)."""
    out, at = [], 0
    for w, b in weights:
        nw, nb = np.asarray(w).size, np.asarray(b).size
        out.append((slice(at, at + nw), slice(at + nw, at + nw + nb)))
        at += nw + nb
    return out


def row_jacobians(weights, x, dtype=torch.float64):
    """[(logits z_n [C], J_n [C, P]) per data row] by torch.autograd."""
    f, flat = R._torch_net(weights, dtype)
    xs = torch.tensor(np.asarray(x), dtype=dtype)
    return [(f(flat, xs[n]).numpy(), torch.autograd.functional.jacobian(lambda th: f(th, xs[n]), flat).numpy())
            for n in range(xs.shape[0])]


def wbar_jacobian(weights, J):
    """Per layer J_l [C, out (in + 1)]: the Jacobian in Wbar = [W | b], flattened row by row."""
    out = []
    for (w, b), (sw, sb) in zip(weights, _layer_slices(weights)):
        o, i = np.asarray(w).shape
        Jw, Jb = J[:, sw].reshape(-1, o, i), J[:, sb].reshape(-1, o, 1)
        out.append(np.concatenate([Jw, Jb], axis=2).reshape(J.shape[0], o * (i + 1)))
    return out


def output_hessian(z, mode, sigma):
    if mode == "classification":
        p = np.exp(z - z.max())
        p /= p.sum()
        return np.diag(p) - np.outer(p, p), p
    return np.eye(z.size) / sigma ** 2, None


def jacobian_factors(weights, x, target, mode, curvature, sigma=1.0):
    """[(A, s, G) per layer] without the restated back-propagation: the Jacobian in a layer's bias IS the Jacobian in its
    pre-activation, so G = sum_n Jb_n^T H_n Jb_n ('ggn') or sum_n (Jb_n^T d_n)(Jb_n^T d_n)^T ('empirical'); the layer's input
    comes from a torch forward."""
    x = np.asarray(x, dtype=np.float64)
    ws = [(torch.tensor(np.asarray(w), dtype=torch.float64), torch.tensor(np.asarray(b), dtype=torch.float64)) for w, b in weights]
    h, ins = torch.tensor(x), []
    for i, (w, b) in enumerate(ws):
        ins.append(h.numpy())
        h = h @ w.T + b
        if i + 1 < len(ws):
            h = torch.relu(h)
    tgt = None if target is None else np.asarray(target)
    out = [[a.T @ a, a.sum(axis=0), 0.0] for a in ins]
    for n, (z, J) in enumerate(row_jacobians(weights, x)):
        H, p = output_hessian(z, mode, sigma)
        if curvature == "empirical":
            if mode == "classification":
                d = p.copy()
                d[int(tgt[n])] -= 1.0
            else:
                d = (z - tgt.reshape(x.shape[0], -1)[n]) / sigma ** 2
        for l, (_, sb) in enumerate(_layer_slices(weights)):
            Jb = J[:, sb]
            if curvature == "ggn":
                out[l][2] = out[l][2] + Jb.T @ H @ Jb
            else:
                v = Jb.T @ d
                out[l][2] = out[l][2] + np.outer(v, v)
    return [tuple(t) for t in out]


def dense_precision(A, s, G, N, tau):
    """kron(G, Abar) / N + tau I: the per-layer posterior precision in Wbar flattened row by row."""
    k = np.kron(np.asarray(G, dtype=np.float64), abar_of(A, s, N)) / N
    return k + tau * np.eye(k.shape[0])


def dense_evidence(weights, factors, N, tau, loglik):
    w2 = sum((np.asarray(w, dtype=np.float64) ** 2).sum() + (np.asarray(b, dtype=np.float64) ** 2).sum() for w, b in weights)
    P = sum(np.asarray(w).size + np.asarray(b).size for w, b in weights)
    ld = 0.0
    for A, s, G in factors:
        sign, v = np.linalg.slogdet(dense_precision(A, s, G, N, tau))
        assert sign > 0
        ld += v
    return loglik - 0.5 * tau * w2 + 0.5 * P * math.log(tau) - 0.5 * ld


def psd(m):
    """The nearest positive semi-definite matrix: the symmetric m with its negative eigenvalues set to 0 (the projection is
    unique, whatever basis a degenerate eigenvalue is given)."""
    lam, q = np.linalg.eigh(np.asarray(m, dtype=np.float64))
    return (q * np.maximum(lam, 0.0)) @ q.T


def dense_glm_cov(weights, x, factors, N, tau, device=None, clamp=False):
    """cov [B, C, C] = sum_l J_l P_l^-1 J_l^T from the autograd Jacobians and a dense solve: basis-invariant.  `clamp`: the
    posterior as F20 defines it for factors that carry rounding-sized negative eigenvalues (fp32 accumulation): G and Abar / N
    projected onto the positive semi-definite matrices first.  `device`: where the fp64 solve runs (torch.linalg.solve, one LU
    per layer for every row's right-hand sides: a 12 000 x 12 000 precision is a second there and a minute in numpy); by
    default numpy on the host."""
    rows = [wbar_jacobian(weights, J) for _, J in row_jacobians(weights, x)]
    B, C = len(rows), rows[0][0].shape[0]
    cov = np.zeros((B, C, C))
    for l, (A, s, G) in enumerate(factors):
        Jl = np.concatenate([r[l] for r in rows])                                     # [B C, P_l]
        Gm, Am = np.asarray(G, dtype=np.float64), abar_of(A, s, N) / N
        if clamp:
            Gm, Am = psd(Gm), psd(Am)
        if device is None:
            X = np.linalg.solve(np.kron(Gm, Am) + tau * np.eye(Gm.shape[0] * Am.shape[0]), Jl.T)
        else:
            D = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=device)   # noqa: E731
            P = torch.kron(D(Gm), D(Am))
            P.diagonal().add_(tau)
            X = torch.linalg.solve(P, D(Jl.T)).cpu().numpy()
            del P
        full = Jl @ X                                                                 # [B C, B C]: the rows' diagonal blocks
        for n in range(B):
            cov[n] += full[n * C:(n + 1) * C, n * C:(n + 1) * C]
    return cov


def sampling_map(QA, lA, QG, lG, tau):
    """M with vec(Wbar_s - Wbar) = M vec(E) (row-by-row vec): (Q_G (x) Q_A) diag(Sigma)."""
    return np.kron(QG, QA) * ((np.outer(lG, lA) + tau) ** -0.5).reshape(-1)[None, :]


def ggn_block(weights, x, mode, sigma=1.0):
    """Per layer the FULL GGN block sum_n J_nl^T H_n J_nl in Wbar (what kron(G, Abar) / N approximates; equal for N = 1)."""
    out = None
    for z, J in row_jacobians(weights, x):
        H, _ = output_hessian(z, mode, sigma)
        inc = [Jl.T @ H @ Jl for Jl in wbar_jacobian(weights, J)]
        out = inc if out is None else [a + b for a, b in zip(out, inc)]
    return out
