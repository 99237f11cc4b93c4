#!/usr/bin/env python3
"""F20: the times of the Kronecker-factored Laplace posterior (bnn_hip.KronLaplace) at ClassConfig (784-1200-1200-10, batch 128)
and at RegConfig (1-400-400-1, batch 400), exact-fp32 math:
  fit                    KronLaplace.fit over `--rows` synthetic rows (the captured chain per minibatch)
  decompose              the fp64 eigendecompositions of every layer's two factors (once per fit)
  fit_prior_precision    33 candidates, ending in the read of the chosen precision
  glm_probit / glm_mc100 glm_predictive_graph(...).replay() of one minibatch
  sample_bank_30         30 matrix-normal weight draws into a WeightBank
beside two baselines in the same process:
  torch_*                a torch loop on the same device that does the same products with torch.matmul / einsum from C backward
                         passes (fit: A += x^T x, s += colsum x, G += gz_c^T gz_c per class; the GLM moments: the rotations, V and
                         the pair sums; the draws: randn, the two batched products), all in fp32
  diag_*                 the same calls on the diagonal DiagLaplace, for context (another posterior, not a competitor)
The torch loop's factors and covariance are held against the device's before anything is timed.  Each window is one call (fit,
decompose, prior) or `--reps` calls (the rest) on a host clock that ends in a device synchronise; the routes alternate in one
process; median and spread of `--rounds` windows after `--warmup`.
One JSON line; --out also writes it to a file.
usage: python tools/kfac_bench.py [--rounds 7] [--warmup 2] [--reps 10] [--rows 60000] [--out results/kfac_bench.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch         # noqa: E402

from laplace_bench import CONFIGS, build, data, spread, timed   # noqa: E402

TAU = 1.0
MC = 100
MEMBERS = 30


def _passes(mlp, x, cfg, seeded):
    """One forward and C backward passes: (inputs per layer, logits, gz [C, B, out] per layer).  seeded: the GGN factor's
    deltas (the fit); otherwise the identity (the Jacobian of the GLM moments)."""
    lins = [m for m in mlp.net if isinstance(m, torch.nn.Linear)]
    h = x.reshape(x.shape[0], -1)
    ins, outs = [], []
    for i, m in enumerate(lins):
        ins.append(h)
        z = m(h)
        outs.append(z)
        h = torch.relu(z) if i + 1 < len(lins) else z
    z = outs[-1]
    C = z.shape[1]
    cls = cfg["net"]["mode"] == "classification"
    p = torch.softmax(z.detach(), dim=1) if cls else None
    eye = torch.eye(C, device=z.device)
    gz = [[] for _ in lins]
    for c in range(C):
        if seeded:
            delta = p[:, c].sqrt()[:, None] * (eye[c][None, :] - p) if cls else eye[c][None, :].expand_as(z) / cfg["sigma"]
        else:
            delta = eye[c][None, :].expand_as(z)
        for i, g in enumerate(torch.autograd.grad((z * delta).sum(), outs, retain_graph=c + 1 < C)):
            gz[i].append(g)
    return [t.detach() for t in ins], z.detach(), [torch.stack(g) for g in gz]


def torch_factors(mlp, batches, cfg):
    lins = [m for m in mlp.net if isinstance(m, torch.nn.Linear)]
    dev = lins[0].weight.device
    A = [torch.zeros((m.in_features, m.in_features), device=dev) for m in lins]
    s = [torch.zeros(m.in_features, device=dev) for m in lins]
    G = [torch.zeros((m.out_features, m.out_features), device=dev) for m in lins]
    for x, _ in batches:
        ins, _, gz = _passes(mlp, x, cfg, True)
        for i, xin in enumerate(ins):
            A[i].addmm_(xin.T, xin)
            s[i].add_(xin.sum(0))
            g = gz[i].reshape(-1, gz[i].shape[2])
            G[i].addmm_(g.T, g)
    return A, s, G


def torch_moments(mlp, la, x, cfg):
    ins, z, gz = _passes(mlp, x, cfg, False)
    B, C = z.shape
    cov = torch.zeros((B, C, C), device=z.device)
    for i, xin in enumerate(ins):
        at = torch.cat([xin, torch.ones((B, 1), device=z.device)], dim=1) @ la.Q_A[i]
        gt = gz[i] @ la.Q_G[i]
        V = at ** 2 @ (1.0 / (torch.outer(la.lam_G32[i], la.lam_A32[i]) + TAU)).T
        cov += torch.einsum("cno,dno,no->ncd", gt, gt, V)
    return z, cov


def torch_draws(mlp, la, members):
    out = []
    for i, m in enumerate(mm for mm in mlp.net if isinstance(mm, torch.nn.Linear)):
        sig = (torch.outer(la.lam_G32[i], la.lam_A32[i]) + TAU).rsqrt()
        e = torch.randn((members,) + tuple(sig.shape), device=sig.device) * sig
        wbar = torch.cat([m.weight.detach(), m.bias.detach()[:, None]], dim=1)
        out.append(wbar + la.Q_G[i] @ e @ la.Q_A[i].T)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kfac_bench: needs a ROCm device (no CPU timing stands in for it)")
    import bnn_hip
    dev = torch.device("cuda:0")
    bnn_hip.set_math("f32")
    result = {"tool": "kfac_bench", "rounds": args.rounds, "reps": args.reps, "rows": args.rows, "math": "f32", "mc_samples": MC,
              "members": MEMBERS, "prior_precision": TAU, "configs": {}}
    for name, cfg in CONFIGS.items():
        mlp = build(cfg, dev)
        batches = data(cfg, args.rows, dev)
        x = batches[0][0]
        kron = bnn_hip.KronLaplace(mlp, curvature="ggn", sigma=cfg["sigma"])
        diag = bnn_hip.DiagLaplace(mlp, curvature="ggn", sigma=cfg["sigma"])
        # agreement before anything is timed: the factors of a prefix, and the covariance of one minibatch
        head = batches[:8]
        kron.fit(head)
        tA, ts, tG = torch_factors(mlp, head, cfg)
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()          # noqa: E731
        entry = {"batch": cfg["batch"], "minibatches": len(batches),
                 "max_rel_diff_factors_vs_torch": max(max(rel(a, b) for a, b in zip(got, ref))
                                                      for got, ref in ((kron.A, tA), (kron.s, ts), (kron.G, tG)))}
        kron.decompose()
        _, cov = kron.glm_moments(x, prior_precision=TAU)
        entry["max_rel_diff_cov_vs_torch"] = rel(cov, torch_moments(mlp, kron, x, cfg)[1])
        # whole-pass windows
        routes = (("fit", lambda: kron.fit(batches)), ("torch_fit", lambda: torch_factors(mlp, batches, cfg)),
                  ("diag_fit", lambda: diag.fit(batches)))
        for _ in range(args.warmup):
            for _, fn in routes:
                fn()
        times = {k: [] for k, _ in routes}
        for _ in range(args.rounds):
            for k, fn in routes:
                times[k].append(timed(fn))

        def decompose():
            kron._invalidate()
            kron.decompose()
        singles = (("decompose", decompose), ("fit_prior_precision_33", lambda: (kron.fit_prior_precision(), kron.prior_precision)),
                   ("diag_fit_prior_precision_33", lambda: (diag.fit_prior_precision(), diag.prior_precision)))
        for k, fn in singles:
            times[k] = [timed(fn) for _ in range(args.warmup + args.rounds)][args.warmup:]
        # per-call windows
        probit = kron.glm_predictive_graph(x, link="probit", prior_precision=TAU)
        mc = kron.glm_predictive_graph(x, MC, link="mc", prior_precision=TAU)
        dprobit = diag.glm_predictive_graph(x, link="probit", prior_precision=TAU)
        dmc = diag.glm_predictive_graph(x, MC, link="mc", prior_precision=TAU)
        bank = kron.sample_bank(MEMBERS, prior_precision=TAU)
        calls = (("glm_probit", probit.replay), (f"glm_mc{MC}", mc.replay), ("torch_glm_moments", lambda: torch_moments(mlp, kron, x, cfg)),
                 ("diag_glm_probit", dprobit.replay), (f"diag_glm_mc{MC}", dmc.replay),
                 (f"sample_bank_{MEMBERS}", lambda: kron.sample_bank(MEMBERS, bank=bank, prior_precision=TAU)),
                 (f"torch_draws_{MEMBERS}", lambda: torch_draws(mlp, kron, MEMBERS)))
        loop = lambda fn: [fn() for _ in range(args.reps)]                       # noqa: E731
        for _ in range(args.warmup):
            for _, fn in calls:
                loop(fn)
        for k, _ in calls:
            times[k] = []
        for _ in range(args.rounds):
            for k, fn in calls:
                times[k].append(timed(lambda: loop(fn)) / args.reps)
        entry.update({k: spread(v) for k, v in times.items()})
        entry["prior_precision_chosen"] = kron.prior_precision
        print(f"{name}: done", file=sys.stderr, flush=True)
        result["configs"][name] = entry
    bnn_hip.set_math("bf16")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
