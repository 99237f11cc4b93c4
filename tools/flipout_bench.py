#!/usr/bin/env python3
"""What the Flipout estimator (F16, bnn_hip.flipout) costs and buys at ClassConfig (784-1200-1200-10, batch 128, Gaussian
prior, bf16 math) on synthetic data.  Not on the product path; bench.py does not call it.

  predict   milliseconds per predict_mc call at S = 10 / 64 / 256: the Flipout view with base_draws = 1 and = S, the BBB net
            (BayesianLinear, one weight draw per sample) and the LR net (local reparameterisation); median and min - max of
            `--reps` windows of `--inner` back-to-back calls between device events, the four ways interleaved window by window
  train     milliseconds per captured training step at S = 2: FlipoutNetwork.graphed_train_step (base_draws = 1) against
            train.GraphedTrainStep on the BBB and the LR net; the same windows over replay()
  variance  the trace of the covariance of the one-sample estimate of d NLL / d mu of layer 1 over `--seeds` Philox seeds on
            one fixed minibatch and one fixed parameter set (beta = 0: the likelihood term, which is where the estimators
            differ), BBB against Flipout with one base draw, exact fp32 math, accumulated in fp64 on the device
usage: python tools/flipout_bench.py [--reps 7] [--inner 20] [--seeds 64] [--quick] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--quick", action="store_true", help="a small network and S = 4: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bnn_hip
    import networks
    from bnn_hip import synth
    from bnn_hip.optim import FusedAdam
    from bnn_hip.train import GraphedTrainStep
    assert torch.cuda.is_available(), "flipout_bench measures on a ROCm device"
    dev = torch.device("cuda:0")
    C = networks.ClassConfig
    hidden, B = (64, 32) if args.quick else (C.hidden_units, C.batch_size)
    samples = (4,) if args.quick else (10, 64, 256)

    def make(lr):
        torch.manual_seed(7)
        return networks.BayesianNetwork(dict(input_shape=C.x_shape, classes=C.classes, batch_size=B, hidden_units=hidden,
                                             mode="classification", mu_init=C.mu_init, rho_init=C.rho_init, prior_init=C.prior_init,
                                             mixture_prior=False, local_reparam=lr)).to(dev)
    x, y = synth.synth_batch("classification", B, C.x_shape, C.classes)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.inner

    def compare(ways):
        for fn in ways.values():                                       # warm-up: code objects, allocator pools
            fn()
            fn()
        t = {k: [] for k in ways}
        for _ in range(args.reps):
            for k, fn in ways.items():
                t[k].append(window(fn))
        return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}

    out = {"config": dict(hidden=hidden, batch=B, math="bf16", reps=args.reps, inner=args.inner), "predict": {}, "train": {}}
    bnn_hip.set_math("bf16")
    bbb, lrn = make(False).eval(), make(True).eval()
    flip = bbb.flipout()
    with torch.no_grad():
        for S in samples:
            out["predict"][S] = compare({
                "flipout_d1": lambda: flip.predict_mc(x, S, base_draws=1), "flipout_dS": lambda: flip.predict_mc(x, S, base_draws=S),
                "bbb": lambda: bbb.predict_mc(x, S), "lr": lambda: lrn.predict_mc(x, S)})
            print("predict", S, json.dumps(out["predict"][S]), flush=True)

    # ---- the captured training step, S = 2
    steps = {}
    for name, lr in (("flipout_d1", False), ("bbb", False), ("lr", True)):
        net = make(lr).train()
        opt = FusedAdam(net.parameters(), lr=C.lr, capturable=True)
        if name == "flipout_d1":
            steps[name] = net.flipout().graphed_train_step(opt, x, y, 2, base_draws=1)
        else:
            steps[name] = GraphedTrainStep(net, opt, x, y, 2)
        steps[name].beta.fill_(0.5)
    out["train"] = compare({k: s.replay for k, s in steps.items()})
    print("train", json.dumps(out["train"]), flush=True)

    # ---- variance of the one-sample likelihood gradient of layer 1's means
    bnn_hip.set_math("f32")
    net = make(False).train()
    views = {"bbb": net, "flipout_d1": net.flipout()}
    w = net.l1.weight_mu
    var = {}
    for name, v in views.items():
        s1 = torch.zeros(w.shape, dtype=torch.float64, device=dev)
        s2 = torch.zeros(w.shape, dtype=torch.float64, device=dev)
        for seed in range(args.seeds):
            bnn_hip.manual_seed(1000 + seed)
            net.zero_grad()
            v.sample_elbo(x, y, 0.0, 1)[0].backward()
            g = w.grad.double()
            s1 += g
            s2 += g * g
        n = args.seeds
        var[name] = {"trace": float(((s2 - s1 * s1 / n) / (n - 1)).sum()), "mean_norm2": float(((s1 / n) ** 2).sum())}
    var["ratio_flipout_over_bbb"] = var["flipout_d1"]["trace"] / var["bbb"]["trace"]
    out["variance"] = dict(var, seeds=args.seeds, samples=1, beta=0.0, math="f32")
    print("variance", json.dumps(out["variance"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
