#!/usr/bin/env python3
"""F22: the times of SWAG (bnn_hip.FusedSWAG / SwagPosterior) at ClassConfig (784-1200-1200-10, batch 128) and RegConfig
(1-400-400-1, batch 400), bf16 math (the product's default):
  step_*            one replay of the captured K6 training step (dense_train.GraphedDenseTrainStep) with FusedSWAG in the
                    optimiser's place: momentum 0 and 0.9, on steps that collect (start 0, every 1) and that do not (start
                    2^31); beside the captured FusedSGD step built in the same process and timed twice (sgd_a, sgd_b), so that
                    its own run-to-run spread is on record
  sample_bank_M     SwagPosterior.sample_bank(M) at rank 20, M = 30 and 100, into an existing bank
  torch_draws_M     torch on the same device: mean + c_d * s * randn + c_lr * (randn @ D)   (a new [M, stride] tensor)
  kfac_sample_bank_30  F20's KronLaplace.sample_bank(30) on the same network (tools/kfac_bench.py times it too)
  predictive_30     the whole SWAG predictive of one minibatch of 128 rows: sample_bank(30) + bank.predictive
Every window is `--reps` calls between two HIP events on a warm device; the routes alternate in one process; median and
spread of `--rounds` windows after `--warmup`.  --trace: a short run of the SWAG launches alone, for
rocprofv3 --kernel-trace --stats -- python3 tools/swag_bench.py --trace.
One JSON line; --out also writes it to a file.
usage: python tools/swag_bench.py [--rounds 7] [--warmup 2] [--reps 20] [--out profiles/swag_bench.json] [--trace]"""
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

RANK = 20
NEVER = 1 << 31


def event_ms(fn, reps):
    """`reps` calls between two HIP events: device time per call in ms."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def fill(post, n=RANK + 1):
    """Moments as a fit leaves them: the mean at the weights, variances ~1e-4, deviations ~1e-2, count above the rank."""
    from bnn_hip import sgmcmc
    g = torch.Generator(device=post.device).manual_seed(1)
    with torch.no_grad():
        for v, p in zip(post.mean_views(), post.params):
            v.copy_(p)
        post.m2.copy_(n * 1e-4 * torch.rand(post.stride, generator=g, device=post.device))
        post.dev.copy_(1e-2 * torch.randn((post.rank, post.stride), generator=g, device=post.device))
    sgmcmc._set_word(post.count_word, n)


def torch_draws(post, M, scale=1.0):
    from bnn_hip import ops
    n = post.count()
    K = min(n, post.rank)
    c_d, c_lr = ops.swag_coefficients(scale, True)
    s = torch.sqrt(torch.clamp(post.m2 / n, min=1e-30))
    z1 = torch.randn((M, post.stride), device=post.device)
    z2 = torch.randn((M, K), device=post.device)
    return post.mean + c_d * s * z1 + float(c_lr[K]) * (z2 @ post.dev[:K])


def steps_of(mlp, x, y):
    """name -> a replay callable of a captured step on its own copy of the network."""
    import bnn_hip
    from bnn_hip.optim import FusedSGD
    out = {}
    for name in ("sgd_a", "sgd_b"):
        net = copy.deepcopy(mlp)
        opt = FusedSGD(net.parameters(), 1e-4, capturable=True)
        out["step_" + name] = net.graphed_train_step(opt, x, y).replay
    for mom in (0.0, 0.9):
        for collecting in (False, True):
            net = copy.deepcopy(mlp)
            opt, _ = net.swag(1e-4, momentum=mom, rank=RANK, start=0 if collecting else NEVER, every=1)
            tag = f"step_swag_m{mom:g}_{'collecting' if collecting else 'plain'}"
            out[tag] = net.graphed_train_step(opt, x, y).replay
    assert bnn_hip.get_math() == "bf16"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swag_bench: needs a ROCm device (no CPU timing stands in for it)")
    import bnn_hip
    dev = torch.device("cuda:0")
    result = {"tool": "swag_bench", "rounds": args.rounds, "reps": args.reps, "math": "bf16", "rank": RANK, "configs": {}}
    for name, cfg in CONFIGS.items():
        mlp = build(cfg, dev)
        x, y = data(cfg, cfg["batch"], dev)[0]
        routes = steps_of(mlp, x, y)
        post = bnn_hip.SwagPosterior(mlp, rank=RANK)
        fill(post)
        banks = {M: post.sample_bank(M) for M in (30, 100)}
        xs = x[:128]
        for M in (30, 100):
            routes[f"sample_bank_{M}"] = lambda M=M: post.sample_bank(M, banks[M])
        routes["predictive_30"] = lambda: (post.sample_bank(30, banks[30]), banks[30].predictive(xs))
        if args.trace:
            for _, fn in routes.items():
                for _ in range(args.reps):
                    fn()
            torch.cuda.synchronize()
            continue
        for M in (30, 100):
            routes[f"torch_draws_{M}"] = lambda M=M: torch_draws(post, M)
        bnn_hip.set_math("f32")                                      # (KronLaplace fits in exact fp32, as tools/kfac_bench.py)
        kron = bnn_hip.KronLaplace(mlp, curvature="ggn", sigma=cfg["sigma"])
        kron.fit(data(cfg, 8 * cfg["batch"], dev))
        kbank = kron.sample_bank(30, prior_precision=1.0)
        bnn_hip.set_math("bf16")

        def kfac_draw():
            bnn_hip.set_math("f32")
            kron.sample_bank(30, bank=kbank, prior_precision=1.0)
            bnn_hip.set_math("bf16")
        routes["kfac_sample_bank_30"] = kfac_draw
        for _ in range(args.warmup):
            for fn in routes.values():
                event_ms(fn, args.reps)
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(event_ms(fn, args.reps))
        entry = {"batch": cfg["batch"], "parameters": sum(post.numels), "stride": post.stride}
        entry.update({k: spread(v) for k, v in times.items()})
        print(f"{name}: done", file=sys.stderr, flush=True)
        result["configs"][name] = entry
    if args.trace:
        return
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
