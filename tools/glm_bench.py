#!/usr/bin/env python3
"""F18: the time of the linearised (GLM) predictive of a DiagLaplace posterior for one minibatch at ClassConfig
(784-1200-1200-10, batch 128) and at RegConfig (1-400-400-1, batch 400), in exact-fp32 and in bf16 math (the input-gradient
product and the forward only; V and the covariance are always fp32):
  glm_probit_graph     glm_predictive_graph(link='probit').replay()
  glm_mc100_graph      glm_predictive_graph(100, link='mc').replay() (regression: the same closed form, nothing is sampled)
  torch_c_backward     a torch loop on the same device that builds the same moments: one forward, then C backward passes
                       (torch.autograd.grad down to every Linear's output), cov += einsum(gz_c, gz_c', V) with V from the same
                       curvature, all in fp32
  network_predict_mc   la.network().predict_mc(x, 100), for context: the NN-sampling predictive of the same posterior
The posterior is fitted on 16 synthetic minibatches first; tau = 1.  The torch loop's covariance is held against the device's
before anything is timed.  Each window is `--reps` calls on a host clock that ends in a device synchronise, reported per call;
the routes alternate in one process; median and spread of `--rounds` windows after `--warmup`.
One JSON line; --out also writes it to a file.
usage: python tools/glm_bench.py [--rounds 7] [--warmup 2] [--reps 20] [--out results/glm_bench.json]"""
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


def torch_moments(mlp, curv, x):
    """(mean, cov [B, C, C]) by C autograd passes, fp32."""
    lins = [m for m in mlp.net if isinstance(m, torch.nn.Linear)]
    h = x.reshape(x.shape[0], -1)
    ins, outs = [], []
    for i, m in enumerate(lins):
        ins.append(h)
        z = m(h)
        outs.append(z)
        h = torch.relu(z) if i + 1 < len(lins) else z
    z = outs[-1]
    B, C = z.shape
    gz = [[] for _ in lins]
    for c in range(C):
        for i, g in enumerate(torch.autograd.grad(z[:, c].sum(), outs, retain_graph=c + 1 < C)):
            gz[i].append(g)
    cov = torch.zeros((B, C, C), device=z.device)
    for i, xin in enumerate(ins):
        V = xin.detach() ** 2 @ (1.0 / (curv[2 * i] + TAU)).T + 1.0 / (curv[2 * i + 1] + TAU)
        g = torch.stack(gz[i])
        cov += torch.einsum("cno,dno,no->ncd", g, g, V)
    return z.detach(), cov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("glm_bench: needs a ROCm device (no CPU timing stands in for it)")
    import bnn_hip
    dev = torch.device("cuda:0")
    result = {"tool": "glm_bench", "rounds": args.rounds, "reps": args.reps, "mc_samples": MC, "prior_precision": TAU, "configs": {}}
    for name, cfg in CONFIGS.items():
        mlp = build(cfg, dev)
        batches = data(cfg, 17 * cfg["batch"], dev)
        x = batches[16][0]
        entry = {"batch": cfg["batch"]}
        for math_mode in ("f32", "bf16"):
            bnn_hip.set_math(math_mode)
            la = bnn_hip.DiagLaplace(mlp, curvature="ggn", sigma=cfg["sigma"]).fit(batches[:16])
            probit = la.glm_predictive_graph(x, link="probit", prior_precision=TAU)
            mc = la.glm_predictive_graph(x, MC, link="mc", prior_precision=TAU)
            net = la.network(prior_precision=TAU)
            mean, cov = la.glm_moments(x, prior_precision=TAU)
            t_mean, t_cov = torch_moments(mlp, la.curv, x)
            entry[f"max_rel_diff_cov_vs_torch_{math_mode}"] = ((cov - t_cov).abs().max() / t_cov.abs().max()).item()
            routes = ((f"glm_probit_graph_{math_mode}", probit.replay), (f"glm_mc{MC}_graph_{math_mode}", mc.replay))
            if math_mode == "f32":
                routes += (("torch_c_backward", lambda: torch_moments(mlp, la.curv, x)),)
            def sampled(net=net):
                with torch.no_grad():
                    return net.predictive(x, MC, sigma=cfg["sigma"]) if cfg["net"]["mode"] == "regression" else net.predict_mc(x, MC)
            routes += ((f"network_predict_mc{MC}_{math_mode}", sampled),)
            loop = lambda fn: [fn() for _ in range(args.reps)]      # noqa: E731
            for _ in range(args.warmup):
                for _, fn in routes:
                    loop(fn)
            times = {k: [] for k, _ in routes}
            for _ in range(args.rounds):                            # alternating, in one process
                for k, fn in routes:
                    times[k].append(timed(lambda: loop(fn)) / args.reps)
            entry.update({k: spread(v) for k, v in times.items()})
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
