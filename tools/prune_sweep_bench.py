#!/usr/bin/env python3
"""Milliseconds for weight_pruning.py's table -- the network pruned at the paper's five drop levels, each evaluated over the
test set -- two ways (F9, bnn_hip.posthoc):
  (a) posthoc.PruneSweep: one selection for all thresholds, one byte of level code per parameter, every minibatch through
      all levels at once (build + evaluate; `a_eval`: the evaluate alone on an already built sweep)
  (b) the loop the public API allowed before the sweep, per level: copy.deepcopy(net), prune_weights (a full sort of the
      2.4 M SNRs, two host reads, six in-place launches), 79 minibatches through the copy in eval mode with softmax,
      argmax and the correct count on the device, ECELoss over the level's probabilities
at ClassConfig (784-1200-1200-10, 10 000 synthetic rows, batch 128, a last minibatch of 16), both layer types, bf16 and f32
math.  Each figure: a host clock around one whole table that ends in a device synchronise; the two ways alternate within a
repetition; median and min - max over `--reps` repetitions after `--warmup` untimed ones.  Every configuration runs in a
child process of its own under a time limit; the first failure stops the run.  The correct counts of the two ways are
compared (f32: equal; bf16: reported).
usage: python tools/prune_sweep_bench.py [--reps 7] [--warmup 2] [--out FILE.json] [--only NAME]"""
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

LEVELS = (0., .5, .75, .95, .98)
CONFIGS = {"bbb_bf16": (False, "bf16"), "lr_bf16": (True, "bf16"), "bbb_f32": (False, "f32"), "lr_f32": (True, "f32")}
DIMS, ROWS, BATCH = (784, 1200, 10), 10000, 128
CHILD_LIMIT_S = 300


def child(name, reps, warmup):
    import copy
    import numpy as np
    import torch
    import bnn_hip
    import networks
    from bnn_hip import posthoc, synth
    lr, math_mode = CONFIGS[name]
    dev = torch.device("cuda:0")
    bnn_hip.set_math(math_mode)
    net = networks.BayesianNetwork(dict(input_shape=DIMS[0], classes=DIMS[2], batch_size=BATCH, hidden_units=DIMS[1],
                                        mode="classification", mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                                        mixture_prior=False, local_reparam=lr))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*DIMS, lr).items()})
    net.to(dev).eval()
    rs = np.random.RandomState(0)
    X = torch.from_numpy(rs.uniform(0, 1, (ROWS, 1, 28, 28)).astype(np.float32)).to(dev)
    Y = torch.from_numpy(rs.randint(0, DIMS[2], ROWS).astype(np.int64)).to(dev)

    def sweep_table():
        r = posthoc.PruneSweep(net, LEVELS).evaluate((X, Y), batch_size=BATCH)
        return r.correct, r.ece

    built = posthoc.PruneSweep(net, LEVELS)

    def sweep_eval():
        r = built.evaluate((X, Y), batch_size=BATCH)
        return r.correct, r.ece

    def loop_table():
        counts, eces = [], []
        crit = posthoc.ECELoss(bin_step=0.1)
        with torch.no_grad():
            for p in LEVELS:
                c = copy.deepcopy(net)
                posthoc.prune_weights(c, None, p)
                c.eval()
                correct = torch.zeros((), dtype=torch.int64, device=dev)
                probs = []
                for i in range(0, ROWS, BATCH):
                    pr = torch.softmax(c(X[i:i + BATCH]), dim=1)
                    probs.append(pr)
                    correct += (pr.argmax(1) == Y[i:i + BATCH]).sum()
                eces.append(crit(torch.cat(probs), Y)[0])
                counts.append(correct)
        return torch.stack(counts), np.asarray(eces)

    ways = {"a": sweep_table, "a_eval": sweep_eval, "b": loop_table}
    times = {k: [] for k in ways}
    last = {}
    for rep in range(warmup + reps):
        for k, fn in ways.items():                                  # alternating within a repetition
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= warmup:
                times[k].append(dt)
            last[k] = (out[0].cpu().numpy().tolist(), [float(e) for e in out[1]])
    if math_mode == "f32" and last["a"][0] != last["b"][0]:
        raise SystemExit(f"{name}: the sweep's correct counts {last['a'][0]} differ from the loop's {last['b'][0]}")
    res = {"config": name, "levels": LEVELS, "rows": ROWS, "batch": BATCH, "reps": reps, "warmup": warmup,
           "correct_sweep": last["a"][0], "correct_loop": last["b"][0], "ece_sweep": last["a"][1], "ece_loop": last["b"][1]}
    for k, v in times.items():
        res[f"{k}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    res["loop_over_sweep"] = res["b_ms"]["median"] / res["a_ms"]["median"]
    res["loop_over_sweep_eval"] = res["b_ms"]["median"] / res["a_eval_ms"]["median"]
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.warmup)
        return
    results = []
    for name in CONFIGS:
        if a.only and name != a.only:
            continue
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--warmup",
                            str(a.warmup)], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"{name}: child exited with {p.returncode}; stopping")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        print(f"{name}: sweep {r['a_ms']['median']:.1f} ms (evaluate alone {r['a_eval_ms']['median']:.1f}), loop "
              f"{r['b_ms']['median']:.1f} ms, loop / sweep {r['loop_over_sweep']:.2f}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
