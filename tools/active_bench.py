#!/usr/bin/env python3
"""Microseconds per acquisition round of pool-based active learning (F10, bnn_hip.active) at ClassConfig shape
(784-1200-1200-10 BBB, bf16 math, batch 128): a pool of 60 000 synthetic rows, 1 280 of them labelled, S = 10 MC samples,
k = 128 and 1 024, BALD scores.  A round = one training epoch on the labelled subset, scoring the pool, selecting k.  Two
ways, interleaved within a repetition:
  (a) the device-resident path: EpochRunner over pool.loader (no row copied), pool.score, pool.acquire (bnn_acquire_topk)
  (b) the best the public API allowed before: DeviceDataset(x[idx], y[idx]) + DeviceLoader + EpochRunner, a loop of
      net.predictive(16 stacked minibatches, stacked=True) + torch.cat, torch.topk on the masked scores, the mask and the
      index tensor updated with torch ops -- index tensors kept on the device, nothing read back
Also: train / score / select of both ways on their own, and bnn_acquire_topk alone between device events.

Each figure: a host clock around a piece that ends in a device synchronise; the pool is rewound to its starting state
between the pieces (outside the clock); median and min - max over `--reps` repetitions.
usage: python tools/active_bench.py [--reps 5] [--rows 60000] [--out FILE.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bnn_hip
    import networks
    from bnn_hip import active, epoch, ops
    from bnn_hip.optim import FusedAdam
    from bnn_hip.train import GraphedTrainStep
    dims, N, B, S, S_train, n0, G = (784, 1200, 10), args.rows, 128, 10, 2, 1280, 16
    dev = torch.device("cuda:0")
    bnn_hip.set_math("bf16")
    rs = np.random.RandomState(0)
    X = rs.uniform(0, 1, (N, 1, 28, 28)).astype(np.float32)
    Y = rs.randint(0, dims[2], N).astype(np.int64)
    lab0 = rs.permutation(N)[:n0]
    torch.manual_seed(0)
    net = networks.BayesianNetwork(dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1],
                                        mode="classification", mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                                        mixture_prior=False, local_reparam=False)).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=1e-4, capturable=True)
    ds = epoch.DeviceDataset(X, Y, device=dev)
    pool = active.ActivePool(ds, lab0)
    sub = pool.loader(B)
    step = GraphedTrainStep(net, opt, *sub.example(), S_train)
    runner = epoch.EpochRunner(step, sub)
    cand0, lab_init = pool.candidate.clone(), pool._labelled.clone()
    nb_full, tail = N // B, N % B

    def rewind():
        pool.candidate.copy_(cand0)
        pool._labelled.copy_(lab_init)
        pool._words[0:1].fill_(n0)
        pool.n_labelled = n0
        state_b["mask"], state_b["idx"] = cand0.bool(), lab_init[:n0].long()

    state_b = {}

    # ---- (a)
    def a_train():
        runner.run_epoch()

    def a_score():
        state_b["scores_a"] = pool.score(net, S, "bald", chunk=G)

    def a_select(k):
        pool.acquire(state_b["scores_a"], k)

    # ---- (b)
    def b_train():
        idx = state_b["idx"]
        ld = epoch.DeviceLoader(epoch.DeviceDataset(ds.x[idx].reshape(-1, 1, 28, 28), ds.y[idx], device=dev), B)
        epoch.EpochRunner(step, ld).run_epoch()

    def b_score():
        parts = []
        with torch.no_grad():
            for g0 in range(0, nb_full, G):
                g1 = min(nb_full, g0 + G)
                parts.append(net.predictive(ds.x[g0 * B:g1 * B].view(g1 - g0, B, dims[0]), S, stacked=True).mutual_information.reshape(-1))
            if tail:
                parts.append(net.predictive(ds.x[nb_full * B:].view(tail, 1, 28, 28), S).mutual_information)
        state_b["scores_b"] = torch.cat(parts)

    def b_select(k):
        masked = state_b["scores_b"].masked_fill(~state_b["mask"], float("-inf"))
        top = torch.topk(masked, k).indices
        state_b["mask"][top] = False
        state_b["idx"] = torch.cat([state_b["idx"], top])

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    res = {"rows": N, "batch": B, "samples": S, "labelled": n0, "train_steps": n0 // B, "train_samples": S_train, "reps": args.reps}
    rewind()
    for fn in (a_train, a_score, lambda: a_select(128), b_train, b_score, lambda: b_select(128)):       # warm-up
        fn()
    for k in (128, 1024):
        pieces = {"a_round": lambda: (a_train(), a_score(), a_select(k)), "b_round": lambda: (b_train(), b_score(), b_select(k)),
                  "a_train": a_train, "b_train": b_train, "a_score": a_score, "b_score": b_score,
                  "a_select": lambda: a_select(k), "b_select": lambda: b_select(k)}
        times = {name: [] for name in pieces}
        for _ in range(args.reps):
            for name, fn in pieces.items():                # interleaved
                rewind()
                times[name].append(clock(fn))
        out = {name: {"us": statistics.median(v), "min": min(v), "max": max(v)} for name, v in times.items()}
        # the selection launch alone, between device events (the pool rewound before every launch, outside the events)
        a = ops.acquire_topk_args(scores=state_b["scores_a"], candidate=pool.candidate, k=k,
                                  selected=torch.empty(k, dtype=torch.int32, device=dev), labelled=pool._labelled,
                                  n_labelled=pool._words[0:1], n_selected=pool._words[1:2], workspace=ops.acquire_topk_workspace(dev))
        per = []
        for _ in range(4 * args.reps):
            rewind()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.acquire_topk(a)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3)
        out["acquire_topk_device_us"] = {"us": statistics.median(per), "min": min(per), "max": max(per)}
        out["round_b_over_a"] = out["b_round"]["us"] / out["a_round"]["us"]
        res[f"k{k}"] = out
    print(json.dumps({"active_round": res}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
