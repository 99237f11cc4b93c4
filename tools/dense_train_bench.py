#!/usr/bin/env python3
"""Microseconds per training step of MLP / MLP_Dropout (K6, bnn_hip.dense_train) three ways:
  (a) the reference's eager loop on stock modules: zero_grad, forward, loss(sum), backward, torch.optim step
  (b) that same torch loop captured with torch.cuda.graph (the fair baseline for a graph)
  (c) GraphedDenseTrainStep.step (bf16 math, the product default, and f32 math)
for ClassConfig (784-1200-1200-10, batch 128, SGD lr 1e-4; MLP_Dropout and MLP), RegConfig's MCDropout_Regression
(1-400-400-1, batch 128, Adam lr 1e-3) and the bandit's greedy agent (119-100-100-1, batch 64, Adam), plus one
MNIST-shaped epoch (468 x 128 + 1 x 96 rows of synthetic data) for (a) and (c).  Each number is the median over
`--reps` timed groups of the device-timeline time of `--steps` consecutive steps (torch.cuda.Event), divided by the steps.
usage: python tools/dense_train_bench.py [--steps 200] [--reps 7] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bnn_hip  # noqa: E402
import networks  # noqa: E402
from bnn_hip.optim import FusedAdam, FusedSGD  # noqa: E402

CONFIGS = {   # name -> (input, hidden, classes, mode, dropout, batch, optimiser, lr)
    "class_dropout": (784, 1200, 10, "classification", True, 128, "sgd", 1e-4),
    "class_mlp": (784, 1200, 10, "classification", False, 128, "sgd", 1e-4),
    "reg_dropout": (1, 400, 1, "regression", True, 128, "adam", 1e-3),
    "bandit_greedy": (119, 100, 1, "regression", False, 64, "adam", 1e-3),
}


def make(cfg, dev):
    inp, hid, C, mode, dropout, B, kind, lr = cfg
    torch.manual_seed(0)
    cls = networks.MLP_Dropout if dropout else networks.MLP
    mlp = cls(dict(input_shape=inp, classes=C, batch_size=B, hidden_units=hid, mode=mode)).to(dev)
    if mode == "classification":
        x = torch.rand((B, 1, 28, 28) if inp == 784 else (B, 1, 1, inp), device=dev)
        y = torch.randint(0, C, (B,), device=dev)
    else:
        x, y = torch.randn((B, inp), device=dev), torch.randn((B, C), device=dev)
    return mlp, x, y


def torch_opt(kind, mlp, lr, capturable=False):
    if kind == "sgd":
        return torch.optim.SGD(mlp.parameters(), lr=lr)
    return torch.optim.Adam(mlp.parameters(), lr=lr, capturable=capturable)


def loss_fn(mode):
    return (lambda z, y: F.cross_entropy(z, y, reduction="sum")) if mode == "classification" else \
        (lambda z, y: F.mse_loss(z, y, reduction="sum"))


def timed(fn, steps, reps, warm=20):
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


def eager_step(mlp, opt, lf):
    def run(x, y):
        mlp.train()
        opt.zero_grad()
        loss = lf(mlp(x), y)
        loss.backward()
        opt.step()
        return loss
    return run


def graphed_torch(mlp, opt, lf, x, y):
    sx, sy = x.clone(), y.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            lf(mlp(sx), sy).backward()
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(g):
        static_loss = lf(mlp(sx), sy)
        static_loss.backward()
        opt.step()

    def run(xb, yb):
        sx.copy_(xb)
        sy.copy_(yb)
        g.replay()
        return static_loss
    return run


def ours(mlp, cfg, x, y, math_mode):
    bnn_hip.set_math(math_mode)
    kind, lr = cfg[6], cfg[7]
    opt = FusedSGD(mlp.parameters(), lr=lr, capturable=True) if kind == "sgd" else \
        FusedAdam(mlp.parameters(), lr=lr, capturable=True)
    return mlp.graphed_train_step(opt, x, y), opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated config names")
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, reps=args.reps, configs={})
    names = args.only.split(",") if args.only else list(CONFIGS)
    for name in names:
        cfg = CONFIGS[name]
        lf = loss_fn(cfg[3])
        r = {}
        mlp, x, y = make(cfg, dev)
        run = eager_step(mlp, torch_opt(cfg[6], mlp, cfg[7]), lf)
        r["a_eager_torch_us"] = timed(lambda: run(x, y), args.steps, args.reps)
        mlp, x, y = make(cfg, dev)
        mlp.train()
        run = graphed_torch(mlp, torch_opt(cfg[6], mlp, cfg[7], capturable=True), lf, x, y)
        r["b_graphed_torch_us"] = timed(lambda: run(x, y), args.steps, args.reps)
        for mm in ("bf16", "f32"):
            mlp, x, y = make(cfg, dev)
            s, _ = ours(mlp, cfg, x, y, mm)
            r[f"c_graphed_hip_{mm}_us"] = timed(lambda: s.step(x, y), args.steps, args.reps)
        bnn_hip.set_math("bf16")
        res["configs"][name] = r
        print(json.dumps({name: r}), flush=True)

    if not args.no_epoch:
        # one MNIST-shaped epoch of the ClassConfig MLP_Dropout: 468 x 128 + 1 x 96 rows (synthetic, device-resident)
        cfg = CONFIGS["class_dropout"]
        X = torch.rand((468 * 128 + 96, 1, 28, 28), device=dev)
        Y = torch.randint(0, 10, (X.shape[0],), device=dev)
        batches = [(X[i:i + 128], Y[i:i + 128]) for i in range(0, X.shape[0], 128)]
        ep = {}
        mlp, _, _ = make(cfg, dev)
        run = eager_step(mlp, torch_opt("sgd", mlp, cfg[7]), loss_fn("classification"))

        def epoch_a():
            for xb, yb in batches:
                run(xb, yb)
        mlp2, _, _ = make(cfg, dev)
        bnn_hip.set_math("bf16")
        opt = FusedSGD(mlp2.parameters(), lr=cfg[7], capturable=True)
        full = mlp2.graphed_train_step(opt, *batches[0])
        last = mlp2.graphed_train_step(opt, *batches[-1])

        def epoch_c():
            for xb, yb in batches:
                (full if xb.shape[0] == 128 else last).step(xb, yb)
        for key, fn in (("a_eager_torch_ms", epoch_a), ("c_graphed_hip_bf16_ms", epoch_c)):
            fn()
            torch.cuda.synchronize()
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            ep[key] = statistics.median(wall)
        res["mnist_epoch"] = ep
        print(json.dumps({"mnist_epoch": ep}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
