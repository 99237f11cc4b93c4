#!/usr/bin/env python3
"""Microseconds per training step of a deep ensemble of M MLP_Dropout members (F21, bnn_hip.ensemble) three ways:
  (e) EnsembleTrainStep.step: all M members per launch, 8 launches per step whatever M
  (a) M replays of M separately captured GraphedDenseTrainSteps (K6: what training the members one after another costs)
  (b) an eager torch step over the bank's views: baddbmm forward, F.dropout, summed loss, .backward() into one flat
      parameter, torch.optim.SGD / Adam (fp32; timed once per optimiser, not per math mode)
for ClassConfig (784-1200-1200-10, batch 128) and RegConfig (1-400-400-1, batch 400), M in {1, 5, 10, 30}, SGD and Adam, bf16
and f32 math.  Each number is the median over `--reps` timed groups of the device-timeline time of `--steps` consecutive
steps (torch.cuda.Event) divided by the steps; us_per_member = e / M.
usage: python tools/ensemble_bench.py [--steps 100] [--reps 7] [--members 1,5,10,30] [--only class,reg] [--optimisers sgd,adam]
       [--math bf16,f32] [--no-baselines] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bnn_hip  # noqa: E402
import networks  # noqa: E402
from bnn_hip.optim import FusedAdam, FusedSGD  # noqa: E402

CONFIGS = {   # name -> (input, hidden, classes, mode, batch)
    "class": (784, 1200, 10, "classification", 128),
    "reg": (1, 400, 1, "regression", 400),
}
LR = {"sgd": 1e-4, "adam": 1e-3}


def make(cfg, dev):
    inp, hid, C, mode, B = cfg
    torch.manual_seed(0)
    mlp = networks.MLP_Dropout(dict(input_shape=inp, classes=C, batch_size=B, hidden_units=hid, mode=mode)).to(dev)
    if mode == "classification":
        x, y = torch.rand((B, 1, 28, 28), device=dev), torch.randint(0, C, (B,), device=dev)
    else:
        x, y = torch.randn((B, inp), device=dev), torch.randn((B, C), device=dev)
    return mlp, x, y


def fused(kind, params):
    return (FusedSGD if kind == "sgd" else FusedAdam)(params, lr=LR[kind], capturable=True)


def timed(fn, steps, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / steps)
    return statistics.median(per)


def ensemble_step(cfg, dev, M, kind):
    mlp, x, y = make(cfg, dev)
    ens = mlp.ensemble(M, seeds=range(M))
    step = ens.graphed_train_step(fused(kind, ens.parameters()), x, y)
    return ens, step, (lambda: step.step(x, y))


def separate_steps(cfg, dev, M, kind):
    mlp, x, y = make(cfg, dev)
    ens = mlp.ensemble(M, seeds=range(M))
    nets = [ens.member(j) for j in range(M)]
    steps = [n.graphed_train_step(fused(kind, n.parameters()), x, y) for n in nets]

    def run():
        for s in steps:
            s.step(x, y)
    return run


def torch_bank_step(cfg, dev, M, kind):
    """(b): one leaf parameter [M, stride]; every layer's weights are views of it, so backward() fills one gradient buffer."""
    mlp, x, y = make(cfg, dev)
    ens = mlp.ensemble(M, seeds=range(M))
    bank = ens.bank
    P = torch.nn.Parameter(bank.buffer.clone())
    opt = torch.optim.SGD([P], lr=LR[kind]) if kind == "sgd" else torch.optim.Adam([P], lr=LR[kind])
    xf = x.reshape(x.shape[0], -1)
    cls = cfg[3] == "classification"
    dims = [(d.linear.out_features, d.linear.in_features, d.relu, d.p) for d in bank.layers]

    def run():
        opt.zero_grad(set_to_none=True)
        h = xf.unsqueeze(0).expand(M, -1, -1)
        for l, (N, K, relu, p) in enumerate(dims):
            W = P[:, bank._w_off[l]:bank._w_off[l] + N * K].view(M, N, K)
            b = P[:, bank._b_off[l]:bank._b_off[l] + N].unsqueeze(1)
            h = torch.baddbmm(b, h, W.transpose(1, 2))
            if relu:
                h = torch.relu(h)
            if p:
                h = F.dropout(h, p, training=True)
        if cls:
            loss = F.cross_entropy(h.reshape(-1, h.shape[-1]), y.repeat(M), reduction="sum")
        else:
            loss = F.mse_loss(h, y.unsqueeze(0).expand(M, -1, -1), reduction="sum")
        loss.backward()
        opt.step()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--members", default="1,5,10,30")
    ap.add_argument("--only", default=None, help="comma-separated config names")
    ap.add_argument("--optimisers", default="sgd,adam")
    ap.add_argument("--math", default="bf16,f32")
    ap.add_argument("--no-baselines", action="store_true", help="time (e) only: a run under a profiler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    members = [int(m) for m in args.members.split(",")]
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, reps=args.reps, rows=[])
    for name in (args.only.split(",") if args.only else list(CONFIGS)):
        cfg = CONFIGS[name]
        for kind in args.optimisers.split(","):
            for M in members:
                bnn_hip.set_math("f32")
                b_us = float("nan") if args.no_baselines else timed(torch_bank_step(cfg, dev, M, kind), args.steps, args.reps)
                for mm in args.math.split(","):
                    bnn_hip.set_math(mm)
                    ens, step, run = ensemble_step(cfg, dev, M, kind)
                    e_us = timed(run, args.steps, args.reps)
                    launches = step.launches
                    del ens, step, run
                    a_us = float("nan") if args.no_baselines else timed(separate_steps(cfg, dev, M, kind), args.steps, args.reps)
                    row = dict(config=name, optimiser=kind, math=mm, members=M, launches_per_step=launches,
                               ensemble_us=round(e_us, 1), us_per_member=round(e_us / M, 1),
                               separate_k6_us=round(a_us, 1), torch_bank_eager_f32_us=round(b_us, 1))
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    torch.cuda.empty_cache()
    bnn_hip.set_math("bf16")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
