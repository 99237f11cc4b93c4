#!/usr/bin/env python3
"""F19: the SG-MCMC training step and the weight bank's predictive at ClassConfig (784-1200-1200-10).
  step (batch 128, one captured graph replay per call, bf16 and f32 math):
    sgd_graph            GraphedDenseTrainStep on FusedSGD (the step that exists without F19)
    sgld_graph           the same step on FusedSGMCMC, every step filed into a 30-member bank
    sghmc_graph          ... with friction 0.1 (a momentum buffer)
  predictive (M = 10 / 30 / 100 members, 128 and 2 048 rows per launch, bf16 and f32 math):
    bank_forward         WeightBank.forward: one bnn_bank_fwd per layer; bank_GBps = M * member bytes / its time -- the
                         rate at which the launches stream the bank, to hold against HBM's 8.0 TB/s (spec; ~6.3 measured)
    bank_predictive      WeightBank.predictive_graph(x).replay(): the forward and the summary launch, captured
    torch_baddbmm        the same [M, rows, 10] stack by torch.baddbmm over the bank's views (fp32, on the same device)
    member_loop          a Python loop of bank.member(m, into=mlp); mlp(x)
The baddbmm stack is held against bank_forward's (exact-fp32 math) before anything is timed.  Each window is `--reps` calls
(a fifth of that at 2 048 rows) on a host clock that ends in a device synchronise, reported per call; the routes alternate
in one process; median and spread of `--rounds` windows after `--warmup`.  One JSON line; --out also writes it to a file.
usage: python tools/sgmcmc_bench.py [--rounds 7] [--warmup 2] [--reps 20] [--out results/sgmcmc_bench.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch         # noqa: E402

from laplace_bench import CONFIGS, build, data, spread, timed   # noqa: E402

MEMBERS = (10, 30, 100)
ROWS = (128, 2048)


def windows(routes, reps, rounds, warmup):
    loop = lambda fn: [fn() for _ in range(reps)]      # noqa: E731
    for _ in range(warmup):
        for _, fn in routes:
            loop(fn)
    times = {k: [] for k, _ in routes}
    for _ in range(rounds):                            # alternating, in one process
        for k, fn in routes:
            times[k].append(timed(lambda: loop(fn)) / reps)
    return {k: spread(v) for k, v in times.items()}


def baddbmm_stack(bank, x, M):
    h = x.reshape(x.shape[0], -1).unsqueeze(0).expand(M, -1, -1)
    for i, d in enumerate(bank.layers):
        N, K = d.linear.weight.shape
        W = bank.buffer[:M, bank._w_off[i]:bank._w_off[i] + N * K].view(M, N, K)
        b = bank.buffer[:M, bank._b_off[i]:bank._b_off[i] + N].unsqueeze(1)
        h = torch.baddbmm(b, h, W.transpose(1, 2))
        if d.relu:
            h = torch.relu(h)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgmcmc_bench: needs a ROCm device (no CPU timing stands in for it)")
    import bnn_hip
    from bnn_hip.dense_train import GraphedDenseTrainStep
    from bnn_hip.optim import FusedSGD
    from bnn_hip.sgmcmc import FusedSGMCMC, WeightBank, _set_word
    dev = torch.device("cuda:0")
    cfg = CONFIGS["ClassConfig"]
    result = {"tool": "sgmcmc_bench", "rounds": args.rounds, "reps": args.reps, "config": "ClassConfig", "step": {}, "predictive": {}}

    # ---- the training step
    (x, y), = data(cfg, cfg["batch"], dev)
    for math_mode in ("bf16", "f32"):
        bnn_hip.set_math(math_mode)
        routes = []
        for name, friction in (("sgd_graph", None), ("sgld_graph", None), ("sghmc_graph", 0.1)):
            mlp = build(cfg, dev).train()
            if name == "sgd_graph":
                opt = FusedSGD(mlp.parameters(), lr=1e-3, capturable=True)
            else:
                opt = FusedSGMCMC(mlp.parameters(), 1e-6, dataset_size=60000, batch_size=cfg["batch"], friction=friction,
                                  bank=WeightBank(mlp, 30))
            routes.append((f"{name}_{math_mode}", GraphedDenseTrainStep(mlp, opt, x, y).replay))
        result["step"].update(windows(routes, args.reps, args.rounds, args.warmup))
        del routes

    # ---- the predictive
    mlp = build(cfg, dev)
    bank = WeightBank(mlp, max(MEMBERS))
    g = torch.Generator(device=dev).manual_seed(0)
    for v, p in zip(zip(*[bank.views(m) for m in range(bank.capacity)]), mlp.parameters()):
        for t in v:                                    # members drawn around the network's own initialisation scale
            t.copy_(p.detach() + 0.02 * torch.randn(p.shape, generator=g, device=dev))
    member_bytes = 4 * sum(bank.numels)
    result["member_MB"] = round(member_bytes / 1e6, 3)
    for rows in ROWS:
        xs = torch.cat([b[0] for b in data(cfg, rows, dev)])
        reps = args.reps if rows <= 128 else max(2, args.reps // 5)
        for M in MEMBERS:
            _set_word(bank.collected, M)
            entry = {}
            bnn_hip.set_math("f32")
            with torch.no_grad():
                ref, got = baddbmm_stack(bank, xs, M), bank.forward(xs)
            entry["max_rel_diff_vs_baddbmm_f32"] = ((got - ref).abs().max() / ref.abs().max()).item()
            del ref, got

            def loop_members():
                with torch.no_grad():
                    return [bank.member(m, into=mlp)(xs) for m in range(M)]

            def batched():
                with torch.no_grad():
                    return baddbmm_stack(bank, xs, M)
            for math_mode in ("bf16", "f32"):
                bnn_hip.set_math(math_mode)
                graphed = bank.predictive_graph(xs)
                routes = [(f"bank_forward_{math_mode}", lambda: bank.forward(xs)), (f"bank_predictive_{math_mode}", graphed.replay)]
                if math_mode == "f32":
                    routes += [("torch_baddbmm", batched), ("member_loop", loop_members)]
                entry.update(windows(routes, reps, args.rounds, args.warmup))
                ms = entry[f"bank_forward_{math_mode}"]["median_ms"]
                entry[f"bank_GBps_{math_mode}"] = round(M * member_bytes / (ms * 1e-3) / 1e9, 1)
                del graphed, routes
            result["predictive"][f"M{M}_rows{rows}"] = entry
            torch.cuda.empty_cache()
    bnn_hip.set_math("bf16")
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
