#!/usr/bin/env python3
"""F24: the times of IVON (bnn_hip.FusedIVON) at ClassConfig (784-1200-1200-10, batch 128) and RegConfig (1-400-400-1, batch
400), bf16 math (the product's default):
  step_ivon_s1 / _s2   one replay of the captured K6 training step (dense_train.GraphedDenseTrainStep) with FusedIVON in the
                       optimiser's place, 1 and 2 MC samples (9 and 17 launches)
  step_adam / step_sgd the captured FusedAdam and FusedSGD steps (8 launches) built in the same process
  step_bbb_s2          the captured Bayes-by-Backprop step (train.GraphedTrainStep, 2 samples) on a BayesianNetwork of the
                       same widths
  launch_draw / launch_step / launch_adam
                       the two IVON launches (S = 1) and bnn_adam_step alone over the same parameter tensors, INNER of each
                       back to back in one captured graph (a lone eager launch is bound by the host's enqueue, not by the
                       kernel), per launch, with the TB/s of their documented traffic (16, 28 and 28 bytes per parameter).
                       The tensors of ClassConfig (9.6 MB each) stay in the 256 MiB Infinity Cache between the launches, for all
                       three alike: the rates compare the kernels, they are not HBM rates
  sample_bank_30       FusedIVON.sample_bank(30) into an existing bank
  torch_draws_30       torch on the same device: mean + sigma * randn   (a new [30, stride] tensor)
Every window is `--reps` calls between two HIP events on a warm device; the routes alternate in one process; median and
spread of `--rounds` windows after `--warmup`.  --trace CONFIG: a short run of the lone launches and sample_bank(30) of one
configuration, for rocprofv3 --kernel-trace --stats -- python3 tools/ivon_bench.py --trace ClassConfig.
One JSON line; --out also writes it to a file.
usage: python tools/ivon_bench.py [--rounds 7] [--warmup 2] [--reps 20] [--out profiles/ivon_bench.json] [--trace CONFIG]"""
import argparse
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch         # noqa: E402

from laplace_bench import CONFIGS, build, data, spread   # noqa: E402
from swag_bench import event_ms                           # noqa: E402

BYTES = {"launch_draw": 16, "launch_step": 28, "launch_adam": 28}     # per parameter (include/bnn_hip.h F24, F2)
ESS = 60000.0
INNER = 10                                                            # lone launches per captured graph


def captured(fn):
    """INNER calls of fn back to back as one hipGraph; its replay."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    return g.replay


def steps_of(cfg, mlp, x, y):
    """name -> a replay callable of a captured step on its own copy of the network."""
    import networks
    from bnn_hip.optim import FusedAdam, FusedSGD
    from bnn_hip.train import GraphedTrainStep
    out = {}
    for S in (1, 2):
        net = copy.deepcopy(mlp)
        out[f"step_ivon_s{S}"] = net.graphed_train_step(net.ivon(0.1, ESS, samples=S), x, y).replay
    net = copy.deepcopy(mlp)
    out["step_adam"] = net.graphed_train_step(FusedAdam(net.parameters(), lr=1e-3, capturable=True), x, y).replay
    net = copy.deepcopy(mlp)
    out["step_sgd"] = net.graphed_train_step(FusedSGD(net.parameters(), 1e-4, capturable=True), x, y).replay
    mp = dict(cfg["net"], batch_size=cfg["batch"], mu_init=[-0.2, 0.2], rho_init=[-5.0, -4.0], prior_init=[1.0],
              mixture_prior=False, local_reparam=False)
    bbb = networks.BayesianNetwork(mp).to(x.device).train()
    step = GraphedTrainStep(bbb, FusedAdam(bbb.parameters(), lr=1e-3, capturable=True), x, y, 2)
    step.beta.fill_(0.5)
    out["step_bbb_s2"] = step.replay
    return out


def launches_of(mlp):
    """The two IVON launches and bnn_adam_step alone, over copies of the network's parameter tensors and a random gradient."""
    from bnn_hip import ivon, ops
    ps = [p.detach().clone() for p in mlp.parameters()]
    gs = [1e-3 * torch.randn_like(p) for p in ps]
    opt = ivon.FusedIVON(ps, 0.1, ESS, loss_scale=1.0)
    g, d = opt.param_groups[0], opt._dev[0]
    kw = dict(ess=g["ess"], weight_decay=g["weight_decay"])

    def draw():
        ops.ivon_draw(ps, hess=d[ivon._HESS], mean=d[ivon._MEAN], step=d[ivon._STEP], seed=opt.seed, **kw)

    def step():
        ops.ivon_step(ps, gs, lr=opt.lr_eff(), beta1=g["beta1"], beta2=g["beta2"], loss_scale=1.0, mean=d[ivon._MEAN],
                      hess=d[ivon._HESS], avg_grad=d[ivon._GM], step=d[ivon._STEP], beta1_prod=d[ivon._PROD], ticket=d[ivon._TICKET],
                      seed=opt.seed, **kw)

    aps = [p.clone() for p in ps]
    m1, m2 = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]

    def adam():
        ops.adam_step(aps, gs, m1, m2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)

    draw()                                                           # (the step reads the mean the first draw files)
    return {"launch_draw": draw, "launch_step": step, "launch_adam": adam}, sum(opt.numels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, choices=sorted(CONFIGS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivon_bench: needs a ROCm device (no CPU timing stands in for it)")
    import bnn_hip
    dev = torch.device("cuda:0")
    assert bnn_hip.get_math() == "bf16"
    result = {"tool": "ivon_bench", "rounds": args.rounds, "reps": args.reps, "math": "bf16", "ess": ESS,
              "bytes_per_parameter": BYTES, "configs": {}}
    if args.trace:
        mlp = build(CONFIGS[args.trace], dev)
        alone, _ = launches_of(mlp)
        post = mlp.ivon(0.1, ESS)
        bank = post.sample_bank(30)
        alone["sample_bank_30"] = lambda: post.sample_bank(30, bank)
        for fn in alone.values():
            for _ in range(args.reps):
                fn()
        torch.cuda.synchronize()
        return
    result["lone_launches_per_graph"] = INNER
    for name, cfg in CONFIGS.items():
        mlp = build(cfg, dev)
        x, y = data(cfg, cfg["batch"], dev)[0]
        routes = steps_of(cfg, mlp, x, y)
        alone, n_params = launches_of(mlp)
        routes.update({k: captured(fn) for k, fn in alone.items()})
        post = mlp.ivon(0.1, ESS)
        bank = post.sample_bank(30)
        sigma = torch.cat([v.reshape(-1) for v in post.variance()]).sqrt()
        mean = torch.cat([p.detach().reshape(-1) for p in mlp.parameters()])
        routes["sample_bank_30"] = lambda: post.sample_bank(30, bank)
        routes["torch_draws_30"] = lambda: mean + sigma * torch.randn((30, mean.numel()), device=dev)
        for _ in range(args.warmup):
            for fn in routes.values():
                event_ms(fn, args.reps)
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(event_ms(fn, args.reps) / (INNER if k in BYTES else 1))
        entry = {"batch": cfg["batch"], "parameters": n_params, "stride": post.stride}
        entry.update({k: spread(v) for k, v in times.items()})
        for k, b in BYTES.items():
            entry[k]["tb_per_s"] = round(b * n_params / (entry[k]["median_ms"] * 1e-3) / 1e12, 3)
        print(f"{name}: done", file=sys.stderr, flush=True)
        result["configs"][name] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
