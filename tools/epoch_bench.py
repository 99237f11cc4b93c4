#!/usr/bin/env python3
"""Microseconds per training epoch and per step of the supervised tasks, three ways (F8, bnn_hip.epoch):
  (a) epoch.EpochRunner.run_epoch(): permutation, gather, cast, beta and loss filing on the device
      (a_u8: the same with the data set held as uint8, ClassConfig only)
  (b) the best the existing path does with device-resident data: perm = torch.randperm(N, device), then a host loop of
      step.step(x[idx_j], y[idx_j], beta_j)
  (c) the reference's loop: a CPU torch DataLoader(shuffle=True, drop_last=True) over in-memory tensors, .to(DEVICE),
      step.step
at ClassConfig (784-1200-1200-10, 60 000 synthetic rows, batch 128, 2 MC samples; BBB and local reparameterisation) and
RegConfig (1-400-400-1, 1 024 rows, batch 128, 5 MC samples, sigma 0.1), bf16 math.  Plus the permutation launch alone.

Each figure: a host clock around consecutive epochs (1 at ClassConfig, 40 at RegConfig) that end in a device synchronise, per epoch; the three
ways are interleaved within a repetition; median and min - max over `--reps` repetitions.  Every configuration runs in a
child process of its own under a time limit; the first failure stops the run.
usage: python tools/epoch_bench.py [--reps 5] [--out FILE.json] [--only NAME]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {   # name -> (dims, mode, local_reparam, rows, batch, MC samples, sigma, epochs per timed window)
    "class_bbb": ((784, 1200, 10), "classification", False, 60000, 128, 2, 1.0, 1),
    "class_lr": ((784, 1200, 10), "classification", True, 60000, 128, 2, 1.0, 1),
    "reg_bbb": ((1, 400, 1), "regression", False, 1024, 128, 5, 0.1, 40),
    "reg_lr": ((1, 400, 1), "regression", True, 1024, 128, 5, 0.1, 40),
}
CHILD_LIMIT_S = 420


def child(name, reps):
    import numpy as np
    import torch
    import bnn_hip
    import networks
    from bnn_hip import epoch, ops
    from bnn_hip.optim import FusedAdam
    from bnn_hip.train import GraphedTrainStep
    dims, mode, lr, N, B, S, sigma, E = CONFIGS[name]
    dev = torch.device("cuda:0")
    bnn_hip.set_math("bf16")
    rs = np.random.RandomState(0)
    if mode == "classification":
        X8 = rs.randint(0, 256, (N, 1, 28, 28)).astype(np.uint8)
        X, Y = X8.astype(np.float32) / np.float32(255.0), rs.randint(0, dims[2], N).astype(np.int64)
    else:
        X8 = None
        X = rs.uniform(-1, 1, (N, dims[0])).astype(np.float32)
        Y = (np.sin(3 * X) + 0.1 * rs.standard_normal((N, 1))).astype(np.float32)
    M = N // B

    def build(x_np):
        torch.manual_seed(0)
        net = networks.BayesianNetwork(dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode=mode,
                                            mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                                            local_reparam=lr)).to(dev).train()
        opt = FusedAdam(net.parameters(), lr=1e-4, capturable=True)
        ld = epoch.DeviceLoader(epoch.DeviceDataset(x_np, Y, device=dev), B)
        step = GraphedTrainStep(net, opt, *ld.example(), S, sigma=sigma)
        return step, ld

    step_a, ld_a = build(X)
    run_a = epoch.EpochRunner(step_a, ld_a)
    ways = {"a_epoch_runner": run_a.run_epoch}
    if X8 is not None:
        step_8, ld_8 = build(X8)
        ways["a_epoch_runner_uint8"] = epoch.EpochRunner(step_8, ld_8).run_epoch
    step_b, _ = build(X)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    betas = [2 ** (M - (j + 1)) / (2 ** M - 1) for j in range(M)]

    def way_b():
        perm = torch.randperm(N, device=dev)
        for j in range(M):
            idx = perm[j * B:(j + 1) * B]
            step_b.step(Xd[idx], Yd[idx], betas[j])
    ways["b_host_loop_device_data"] = way_b
    step_c, _ = build(X)
    cpu_loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)),
                                             batch_size=B, shuffle=True, drop_last=True)

    def way_c():
        for j, (x, y) in enumerate(cpu_loader):
            step_c.step(x.to(dev), y.to(dev), betas[j])
    ways["c_cpu_dataloader"] = way_c

    for fn in ways.values():                              # warm-up: every shape, every first launch
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(reps):
        for k, fn in ways.items():                        # interleaved
            e = E
            t0 = time.perf_counter()
            for _ in range(e):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / e)
    res = {"rows": N, "batch": B, "steps_per_epoch": M, "samples": S, "epochs_per_window": E, "reps": reps}
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = {"us_per_epoch": med, "min": min(v), "max": max(v), "us_per_step": med / M}
    sp = res["b_host_loop_device_data"]
    res["b_spread_us"] = sp["max"] - sp["min"]
    # the permutation launch alone (device events around 20 launches)
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            ops.epoch_permutation(ld_a._perm)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / 20)
    res["permutation_launch_us"] = {"median": statistics.median(per), "min": min(per), "max": max(per)}
    print(json.dumps({name: res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    out = {}
    for name in (args.only.split(",") if args.only else list(CONFIGS)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr)
            print(f"{name}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        out.update(json.loads(line))
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
