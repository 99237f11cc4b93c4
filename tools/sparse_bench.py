#!/usr/bin/env python3
"""F13: what the compressed pruned network (posthoc.CompressedNetwork: CSR, exact fp32, survivors only) costs beside the dense
paths, at ClassConfig (784-1200-1200-10), 10 000 synthetic rows, batch 128, the paper's drop levels.  Per level:
  evaluate    CompressedNetwork.evaluate against a ONE-level PruneSweep.evaluate in f32 math and in bf16 math -- one window is
              `--reps` whole passes over the 10 000 rows on a host clock, ending in the read of the counts (a synchronise);
  forward_mc  CompressedNetwork.forward_mc at S = 10 against predict_mc of the prune_weights copy (the dense network with
              zeros in it, in the math mode bf16) -- one window is every minibatch of the data once, then a synchronise;
  state       state_bytes with and without the sign bits, nnz per layer, beside the bytes of a prune_weights copy.
The routes of a comparison alternate in one process; the median and the spread (min, max) of `--rounds` windows after
`--warmup` windows are reported, in milliseconds per pass.  Before anything is timed the counts of the compressed and the f32
sweep evaluation are compared and printed.  One JSON line; --out also writes it to a file.
usage: python tools/sparse_bench.py [--rounds 7] [--warmup 2] [--reps 3] [--out results/sparse_bench.json]"""
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
ROWS, BATCH, SAMPLES = 10000, 128, 10
DIMS = (784, 1200, 10)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(routes, rounds, warmup, reps):
    """{name: (median, min, max) ms per pass}: the routes take turns, window by window."""
    times = {k: [] for k in routes}
    for r in range(warmup + rounds):
        for k, fn in routes.items():
            t = window(fn, reps)
            if r >= warmup:
                times[k].append(t)
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_bench needs a ROCm device: a timing taken without one says nothing")
    import bnn_hip
    import networks
    from bnn_hip import posthoc, synth
    dev = torch.device("cuda:0")
    net = networks.BayesianNetwork(dict(input_shape=DIMS[0], hidden_units=DIMS[1], classes=DIMS[2], mode="classification",
                                        batch_size=BATCH, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                                        mixture_prior=False, local_reparam=False))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*DIMS, False).items()})
    net = net.to(dev).eval()
    rng = np.random.default_rng(1)
    X = torch.from_numpy(rng.uniform(0, 1, (a.rows, DIMS[0])).astype(np.float32)).to(dev)
    Y = torch.from_numpy(rng.integers(0, DIMS[2], a.rows)).to(dev)
    dense_bytes = sum(p.numel() * p.element_size() for p in net.parameters())
    out = dict(config="ClassConfig 784-1200-1200-10", rows=a.rows, batch=BATCH, samples=SAMPLES, rounds=a.rounds, warmup=a.warmup,
               reps=a.reps, dense_state_bytes=dense_bytes, levels={})
    for p in LEVELS:
        bnn_hip.set_math("f32")
        sweep32 = posthoc.PruneSweep(net, (p,))
        cn = sweep32.compress(0)
        bnn_hip.set_math("bf16")
        sweep16 = posthoc.PruneSweep(net, (p,))
        pruned = copy.deepcopy(net)
        posthoc.prune_weights(pruned, None, p)
        pruned.eval()
        r_cn, r_32, r_16 = cn.evaluate((X, Y), batch_size=BATCH), sweep32.evaluate((X, Y), batch_size=BATCH), sweep16.evaluate((X, Y), batch_size=BATCH)
        same_bits = all(torch.equal(cn.forward(X[i:i + BATCH]).view(torch.int32), sweep32.forward(X[i:i + BATCH])[0].view(torch.int32))
                        for i in range(0, min(a.rows, 4 * BATCH), BATCH))
        rec = dict(nnz=list(cn.nnz), density=round(cn.density, 6), state_bytes=cn.state_bytes,
                   state_bytes_without_sign_bits=posthoc.compressed_state_bytes([(784, 1200), (1200, 1200), (1200, 10)], cn.nnz, False),
                   correct=dict(compressed=int(r_cn.correct[0]), sweep_f32=int(r_32.correct[0]), sweep_bf16=int(r_16.correct[0])),
                   nll=dict(compressed=float(r_cn.nll[0]), sweep_f32=float(r_32.nll[0])),
                   logits_bit_equal_to_sweep_f32_first_minibatches=bool(same_bits))
        rec["evaluate"] = alternate({"compressed": lambda: cn.evaluate((X, Y), batch_size=BATCH).accuracy,
                                     "sweep_f32": lambda: sweep32.evaluate((X, Y), batch_size=BATCH).accuracy,
                                     "sweep_bf16": lambda: sweep16.evaluate((X, Y), batch_size=BATCH).accuracy},
                                    a.rounds, a.warmup, a.reps)

        def mc_sparse():
            for i in range(0, a.rows, BATCH):
                cn.forward_mc(X[i:i + BATCH], SAMPLES)

        def mc_dense():
            with torch.no_grad():
                for i in range(0, a.rows, BATCH):
                    pruned.predict_mc(X[i:i + BATCH], SAMPLES)

        rec["forward_mc_S10"] = alternate({"compressed_forward_mc": mc_sparse, "pruned_copy_predict_mc_bf16": mc_dense},
                                          a.rounds, a.warmup, 1)
        out["levels"][str(p)] = rec
        print(f"# p={p}: {json.dumps(rec)}", file=sys.stderr)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
