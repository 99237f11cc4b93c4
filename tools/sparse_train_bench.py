#!/usr/bin/env python3
"""F14: what one captured fine-tuning step of a compressed pruned network (sparse_train.SparseTrainStep: CSR, exact fp32,
survivors only) costs beside the dense captured step, at ClassConfig (784-1200-1200-10), batch 128, S = 2, the paper's drop
levels.  Per level three routes take turns in one process:
  sparse       CompressedNetwork.graphed_train_step on the network compressed at the level;
  dense_f32    train.GraphedTrainStep on the prune_weights copy, f32 math;
  dense_bf16   the same in bf16 math
(the dense routes do the same work at every level: they train the zeros too).  One window is `--reps` replays on a host clock
ending in a synchronise; the median and the spread (min, max) of `--rounds` windows after `--warmup` windows are reported, in
microseconds per step.  There is no speed gate.  One JSON line; --out also writes it to a file.
usage: python tools/sparse_train_bench.py [--rounds 7] [--warmup 2] [--reps 50] [--out results/sparse_train_bench.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

LEVELS = (0., .5, .75, .95, .98)
BATCH, SAMPLES = 128, 2
DIMS = (784, 1200, 10)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def alternate(routes, rounds, warmup, reps):
    """{name: (median, min, max) us per step}: the routes take turns, window by window."""
    times = {k: [] for k in routes}
    for r in range(warmup + rounds):
        for k, fn in routes.items():
            t = window(fn, reps)
            if r >= warmup:
                times[k].append(t)
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--levels", type=float, nargs="*", default=list(LEVELS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_train_bench needs a ROCm device: a timing taken without one says nothing")
    import bnn_hip
    import networks
    from bnn_hip import posthoc, synth
    from bnn_hip.optim import FusedAdam
    from bnn_hip.train import GraphedTrainStep
    dev = torch.device("cuda:0")
    net = networks.BayesianNetwork(dict(input_shape=DIMS[0], hidden_units=DIMS[1], classes=DIMS[2], mode="classification",
                                        batch_size=BATCH, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                                        mixture_prior=False, local_reparam=False))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*DIMS, False).items()})
    net = net.to(dev).train()
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(0, 1, (BATCH, DIMS[0])).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, DIMS[2], BATCH)).to(dev)
    out = dict(config="ClassConfig 784-1200-1200-10", batch=BATCH, samples=SAMPLES, rounds=a.rounds, warmup=a.warmup, reps=a.reps,
               levels={})
    for p in a.levels:
        bnn_hip.set_math("f32")
        cn = posthoc.compress(net, p)
        sparse = cn.graphed_train_step(FusedAdam(cn.parameters(), lr=1e-3, capturable=True), x, y, SAMPLES)
        dense = {}
        for mode in ("f32", "bf16"):
            bnn_hip.set_math(mode)
            pruned = copy.deepcopy(net)
            posthoc.prune_weights(pruned, None, p)
            pruned.train()
            dense[mode] = GraphedTrainStep(pruned, FusedAdam(pruned.parameters(), lr=1e-3, capturable=True), x, y, SAMPLES)
        rec = dict(nnz=list(cn.nnz), density=round(cn.density, 6))
        rec["step"] = alternate({"sparse": sparse.replay, "dense_f32": dense["f32"].replay, "dense_bf16": dense["bf16"].replay},
                                a.rounds, a.warmup, a.reps)
        rec["loss_finite"] = bool(torch.isfinite(sparse.out[0]).all())
        out["levels"][str(p)] = rec
        print(f"# p={p}: {json.dumps(rec)}", file=sys.stderr)
        del sparse, dense
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
