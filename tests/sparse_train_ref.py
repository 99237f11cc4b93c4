"""The restatement of the F14 sparse training step (include/bnn_hip.h F14; bnn_hip/sparse_train.py), on the CPU.

A CASE is a dict: layers (per layer row_ptr, col, rows -- the row of every entry --, mu_val, rho_val, sigma_val, b_mu, b_rho,
b_sigma, b_keep, fin, fout, layer_id, all numpy), x [rows, fin], y, mode, S, first (the global MC-sample index of sample 0),
seed, beta, prior (dict: mixture, sigma_p, pi, sigma1, sigma2), nll_sigma.

  autograd_ref   fp64 torch autograd over DENSE masked weights W = scatter(mu + sigma * eps), epsilon from
                 oracle.bnn_oracle.philox_normal on the dense [out, in] map at the step's sample indices, sigma taken from the
                 given values (so d/d rho = d/d sigma * sigmoid(rho)).  Returns (out4, the twelve gradients at the CSR positions).
  closed_ref     the closed forms of the issue / header in numpy, in a chosen dtype: float64 (checked against autograd_ref by
                 tests/test_sparse_train_cpu.py) and float32 with numpy's own summation orders (BLAS matmuls, pairwise sums):
                 a second, independent fp32 ordering of the same arithmetic.
  ref32_of       REF32 of a case: the largest deviation of closed_ref(float32) from closed_ref(float64) over the twelve
                 gradient tensors and out4, relative to each tensor's max |.|.
  build_case     a case from a synth network, pruned by the restatement of tests/test_prune_sweep_cpu.py (no device).
"""
import math

import numpy as np
import torch

from oracle import bnn_oracle as O

C0 = -0.5 * math.log(2.0 * math.pi)
GRAD_NAMES = tuple(f"l{i}.{n}" for i in (1, 2, 3) for n in ("weight_mu", "weight_rho", "bias_mu", "bias_rho"))
_eps_cache = {}


def dense_eps(seed, layer_id, g, fout, fin):
    """(eps_w [out, in], eps_b [out]) of global sample g: the dense weight-space map (kind 0) and the bias map (kind 1)."""
    key = (seed, layer_id, g, fout, fin)
    if key not in _eps_cache:
        _eps_cache[key] = (np.asarray(O.philox_normal(seed, 4 * layer_id, g, fout, fin), dtype=np.float64),
                           np.asarray(O.philox_normal(seed, 4 * layer_id + 1, g, 1, fout), dtype=np.float64)[0])
    return _eps_cache[key]


def case_eps(case, s):
    """Per layer (eps at the CSR entries [nnz], eps_b [out]) of the step's sample s, float64."""
    out = []
    for l in case["layers"]:
        ew, eb = dense_eps(case["seed"], l["layer_id"], case["first"] + s, l["fout"], l["fin"])
        out.append((ew[l["rows"], l["col"]], eb))
    return out


# ------------------------------------------------------------------------------------------------- fp64 autograd
def _log_prior_t(w, pr):
    if pr["mixture"]:
        n1 = torch.exp(-w ** 2 / (2 * pr["sigma1"] ** 2) - math.log(pr["sigma1"]) + C0)
        n2 = torch.exp(-w ** 2 / (2 * pr["sigma2"] ** 2) - math.log(pr["sigma2"]) + C0)
        return torch.log(pr["pi"] * n1 + (1 - pr["pi"]) * n2).sum()
    return (-w ** 2 / (2 * pr["sigma_p"] ** 2) - math.log(pr["sigma_p"]) + C0).sum()


def _nll_t(out, y, mode, sigma):
    if mode == "classification":
        return torch.nn.functional.cross_entropy(out, y, reduction="sum")
    return -(-((y - out) ** 2) / (2 * sigma ** 2) - math.log(sigma) + C0).sum()


def autograd_ref(case):
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    leaves = [(t64(l["mu_val"]), t64(l["sigma_val"]), t64(l["b_mu"]), t64(l["b_sigma"])) for l in case["layers"]]
    x = torch.tensor(np.asarray(case["x"], dtype=np.float64).reshape(len(case["x"]), -1))
    y = torch.as_tensor(case["y"]) if case["mode"] == "classification" else \
        torch.tensor(np.asarray(case["y"], dtype=np.float64).reshape(len(case["x"]), -1))
    S, pr = case["S"], case["prior"]
    lps, lqs, nlls = [], [], []
    for s in range(S):
        h, lp, lq = x, 0.0, 0.0
        for i, (l, (mu, sg, bmu, bsg), (ew, eb)) in enumerate(zip(case["layers"], leaves, case_eps(case, s))):
            ew, eb = torch.tensor(ew), torch.tensor(eb)
            keep = torch.tensor(np.asarray(l["b_keep"], dtype=bool))
            w = mu + sg * ew
            W = torch.zeros((l["fout"], l["fin"]), dtype=torch.float64).index_put(
                (torch.as_tensor(l["rows"]), torch.as_tensor(l["col"])), w)
            b = torch.where(keep, bmu + bsg * eb, torch.zeros_like(bmu))
            h = h @ W.t() + b
            if i < 2:
                h = torch.relu(h)
            bk, bsk, ebk = b[keep], bsg[keep], eb[keep]
            lq = lq + (C0 - torch.log(sg) - ew ** 2 / 2).sum() + (C0 - torch.log(bsk) - ebk ** 2 / 2).sum()
            lp = lp + _log_prior_t(w, pr) + _log_prior_t(bk, pr)
        lps.append(lp)
        lqs.append(lq)
        nlls.append(_nll_t(h, y, case["mode"], case["nll_sigma"]))
    mlp, mlq, mnll = sum(lps) / S, sum(lqs) / S, sum(nlls) / S
    loss = case["beta"] * (mlq - mlp) + mnll
    loss.backward()
    grads = []
    for l, (mu, sg, bmu, bsg) in zip(case["layers"], leaves):
        sig = lambda r: 1.0 / (1.0 + np.exp(-np.asarray(r, dtype=np.float64)))
        grads += [mu.grad.numpy(), sg.grad.numpy() * sig(l["rho_val"]), bmu.grad.numpy(), bsg.grad.numpy() * sig(l["b_rho"]) * l["b_keep"]]
    return np.array([loss.item(), mlp.item(), mlq.item(), mnll.item()]), grads


# ------------------------------------------------------------------------------------------------- the closed forms
def _dlogp(w, pr, dt):
    if not pr["mixture"]:
        return -w / dt(pr["sigma_p"] ** 2)
    s1, s2, pi = pr["sigma1"], pr["sigma2"], pr["pi"]
    n1 = dt(pi / s1) * np.exp(-w * w * dt(1 / (2 * s1 * s1)))
    n2 = dt((1 - pi) / s2) * np.exp(-w * w * dt(1 / (2 * s2 * s2)))
    return -w * (n1 * dt(1 / (s1 * s1)) + n2 * dt(1 / (s2 * s2))) / (n1 + n2)


def _log_prior_np(w, pr, dt):
    if not pr["mixture"]:
        return (dt(C0 - math.log(pr["sigma_p"])) - w * w * dt(1 / (2 * pr["sigma_p"] ** 2))).sum(dtype=dt)
    n1 = np.exp(dt(C0 - math.log(pr["sigma1"])) - w * w * dt(1 / (2 * pr["sigma1"] ** 2)))
    n2 = np.exp(dt(C0 - math.log(pr["sigma2"])) - w * w * dt(1 / (2 * pr["sigma2"] ** 2)))
    return np.log(dt(pr["pi"]) * n1 + dt(1 - pr["pi"]) * n2).sum(dtype=dt)


def closed_ref(case, dtype=np.float64):
    """(out4, the twelve gradients) by the closed forms, every array and every sum in `dtype`."""
    dt = np.dtype(dtype).type
    A = lambda a: np.asarray(a, dtype=dt)
    S, pr, beta, mode = case["S"], case["prior"], dt(case["beta"]), case["mode"]
    L = case["layers"]
    x = A(case["x"]).reshape(len(case["x"]), -1)
    B = x.shape[0]
    y = np.asarray(case["y"]) if mode == "classification" else A(case["y"]).reshape(B, -1)
    g_lp, g_lq = -beta / dt(S), beta / dt(S)
    acc = [dict(t=np.zeros(len(l["col"]), dt), te=np.zeros(len(l["col"]), dt), bt=np.zeros(l["fout"], dt), bte=np.zeros(l["fout"], dt))
           for l in L]
    lps, lqs, nlls = [], [], []
    for s in range(S):
        eps = [(A(ew), A(eb)) for ew, eb in case_eps(case, s)]
        hs, ws, bs = [x], [], []
        lp, lq = dt(0), dt(0)
        for i, (l, (ew, eb)) in enumerate(zip(L, eps)):
            keep = np.asarray(l["b_keep"], dtype=bool)
            w = A(l["mu_val"]) + A(l["sigma_val"]) * ew
            b = np.where(keep, A(l["b_mu"]) + A(l["b_sigma"]) * eb, dt(0))
            W = np.zeros((l["fout"], l["fin"]), dt)
            W[l["rows"], l["col"]] = w
            z = hs[-1] @ W.T + b
            hs.append(np.maximum(z, dt(0)) if i < 2 else z)
            ws.append((w, W))
            bs.append(b)
            cnt = dt(len(w) + keep.sum())
            lq = lq + (cnt * dt(C0) - np.log(A(l["sigma_val"])).sum(dtype=dt) - np.log(A(l["b_sigma"])[keep]).sum(dtype=dt)
                       - dt(0.5) * ((ew * ew).sum(dtype=dt) + (eb[keep] * eb[keep]).sum(dtype=dt)))
            lp = lp + _log_prior_np(w, pr, dt) + _log_prior_np(b[keep], pr, dt)
        out = hs[-1]
        if mode == "classification":
            m = out.max(1, keepdims=True)
            lse = np.log(np.exp(out - m).sum(1, keepdims=True, dtype=dt)) + m
            nll = (lse[:, 0] - out[np.arange(B), y]).sum(dtype=dt)
            gz = np.exp(out - lse)
            gz[np.arange(B), y] -= dt(1)
        else:
            sg = dt(case["nll_sigma"])
            d = out - y
            nll = ((d * d) * dt(1 / (2 * float(sg) ** 2)) + dt(math.log(float(sg)) - C0)).sum(dtype=dt)
            gz = d * dt(1 / float(sg) ** 2)
        gz = gz / dt(S)
        lps.append(lp)
        lqs.append(lq)
        nlls.append(nll)
        for i in (2, 1, 0):
            l, (ew, eb), (w, W) = L[i], eps[i], ws[i]
            keep = np.asarray(l["b_keep"], dtype=bool)
            G = (gz.T @ hs[i])[l["rows"], l["col"]]
            t = G + g_lp * _dlogp(w, pr, dt)
            acc[i]["t"] += t
            acc[i]["te"] += t * ew
            tb = np.where(keep, gz.sum(0, dtype=dt) + g_lp * _dlogp(bs[i], pr, dt), dt(0))
            acc[i]["bt"] += tb
            acc[i]["bte"] += tb * eb
            if i > 0:
                gz = (gz @ W) * (hs[i] > 0)
    lps, lqs, nlls = A(lps), A(lqs), A(nlls)
    mlp, mlq, mnll = lps.mean(dtype=dt), lqs.mean(dtype=dt), nlls.mean(dtype=dt)
    out4 = np.array([beta * (mlq - mlp) + mnll, mlp, mlq, mnll], dtype=dt)
    sig = lambda r: dt(1) / (dt(1) + np.exp(-A(r)))
    grads = []
    for l, a in zip(L, acc):
        keep = np.asarray(l["b_keep"], dtype=bool)
        cq = dt(S) * g_lq
        safe = np.where(keep, A(l["b_sigma"]), dt(1))
        grads += [a["t"], (a["te"] - cq / A(l["sigma_val"])) * sig(l["rho_val"]), a["bt"],
                  np.where(keep, (a["bte"] - cq / safe) * sig(l["b_rho"]), dt(0))]
    return out4, grads


def rel_dev(got, want):
    """max |got - want| / max |want| of one tensor (0 for an empty one; the absolute deviation when want is all zero)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0))


def ref32_of(case, ref64=None):
    """REF32: the fp32 restatement against the fp64 one, the worst tensor (the twelve gradients and out4)."""
    o64, g64 = closed_ref(case, np.float64) if ref64 is None else ref64
    o32, g32 = closed_ref(case, np.float32)
    return max([rel_dev(o32, o64)] + [rel_dev(a, b) for a, b in zip(g32, g64)])


# ------------------------------------------------------------------------------------------------- cases without a device
def softplus32(rho):
    return torch.log1p(torch.exp(torch.as_tensor(np.asarray(rho, dtype=np.float32)))).numpy()


def layers_from_dense(params, keep_w, keep_b, sigma=None):
    """CSR layers from canonical dense parameters: params = [(W_mu, W_rho [out, in], b_mu, b_rho)], keep_* boolean masks;
    sigma: None (fp32 softplus of rho) or a function rho -> sigma."""
    sp = softplus32 if sigma is None else sigma
    out = []
    for i, ((wm, wr, bm, br), kw, kb) in enumerate(zip(params, keep_w, keep_b)):
        r, c = np.nonzero(kw)
        rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=wm.shape[0]))]).astype(np.int32)
        z = np.zeros_like(bm)
        out.append(dict(row_ptr=rp, col=c.astype(np.int64), rows=r.astype(np.int64), mu_val=wm[r, c], rho_val=wr[r, c],
                        sigma_val=sp(wr[r, c]), b_mu=np.where(kb, bm, z), b_rho=np.where(kb, br, z),
                        b_sigma=np.where(kb, sp(br), z), b_keep=kb.astype(np.uint8), fin=wm.shape[1], fout=wm.shape[0], layer_id=i))
    return out


def build_case(dims, mode, lr, level, rows, S, mixture=False, seed=2026, first=0, beta=0.3, data_seed=5, sigma=None):
    """A synth network (bnn_hip.synth) pruned at `level` by the restatement of tests/test_prune_sweep_cpu.py."""
    from bnn_hip import synth
    from test_prune_sweep_cpu import snr32_torch, thresholds_ref
    sd = synth.synth_state_dict(*dims, lr)
    params = []
    for n in ("l1", "l2", "l3"):
        wm, wr = sd[f"{n}.weight_mu"], sd[f"{n}.weight_rho"]
        params.append(((wm.T.copy(), wr.T.copy()) if lr else (wm, wr)) + (sd[f"{n}.bias_mu"], sd[f"{n}.bias_rho"]))
    snrs = [snr32_torch(a, b) for p in params for a, b in ((p[0], p[1]), (p[2], p[3]))]
    thr = np.float32(thresholds_ref(np.concatenate([s.ravel() for s in snrs]), [level])[0])
    with np.errstate(invalid="ignore"):
        keep_w = [snrs[2 * i] > thr for i in range(3)]
        keep_b = [snrs[2 * i + 1] > thr for i in range(3)]
    x, y = synth.synth_batch(mode, rows, dims[0], dims[2], seed=data_seed)
    prior = dict(mixture=bool(mixture), sigma_p=1.0, pi=0.5, sigma1=math.exp(0.0), sigma2=math.exp(-6.0))
    return dict(layers=layers_from_dense(params, keep_w, keep_b, sigma), x=x.reshape(rows, -1), y=y, mode=mode, S=S, first=first,
                seed=seed, beta=beta, prior=prior, nll_sigma=1.0)


# (dims, mode, local_reparam, drop level, batch rows, MC samples, mixture prior): the cases of tests/test_gpu_sparse_train.py.
# Rows 37 (less than a wave, odd) and 300 (crosses the forward's 256-row batch block); a 1-column layer, empty rows and
# columns at .98, survivors sharing and not sharing a Philox group, a 10-wide row-major gy; both source layer types.
CASES = (
    ((1, 48, 1), "regression", False, 0., 37, 1, False),
    ((1, 48, 1), "regression", True, .5, 300, 3, False),
    ((1, 48, 1), "regression", False, .98, 37, 3, True),
    ((70, 130, 10), "classification", False, 0., 300, 3, False),
    ((70, 130, 10), "classification", False, .5, 37, 3, True),
    ((70, 130, 10), "classification", True, .98, 300, 1, False),
    ((70, 130, 10), "classification", True, .5, 37, 1, False),
    ((119, 100, 1), "regression", False, .98, 300, 3, False),
    ((119, 100, 1), "regression", True, 0., 37, 3, False),
    ((119, 100, 1), "regression", False, .5, 300, 1, True),
)
