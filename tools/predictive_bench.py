"""F3 measurement: the predictive summaries (net.predictive_graph: bnn_mc_predictive behind the evaluation's launch chain)
against the MC-averaged prediction alone (net.predictor), replay for replay, at test_samples = 10 (the reference's config.py):
  - MNIST shape 784-1200-1200-10, batch 128, BBB and LR;
  - regression 1-400-400-1 over 400 points with 5 quantiles (no predictor exists for regression: its baseline is the same
    launch chain without the summary launch, engine.GraphedElbo);
  - 78 stacked minibatches of 128 rows (one predictive_graph replay) against 78 predictor replays.
Wall time per replay (host loop of replays, synchronised at the ends).  Prints one line per case, then the rows as JSON.
usage: python tools/predictive_bench.py [samples]"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bnn_hip  # noqa: E402
import networks  # noqa: E402
from bnn_hip import engine, synth  # noqa: E402

dev = torch.device("cuda:0")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def net_of(dims, mode, lr, B):
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    sd = synth.synth_state_dict(*dims, lr)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dev).eval()


def timed(fn, n, reps_per_call=1):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (n * reps_per_call) * 1e6


rows = []


def report(case, form, us, per):
    rows.append(dict(case=case, form=form, test_samples=S, us=us, per=per))
    print(f"{case:34s} {form:44s}: {us:9.1f} us per {per}", flush=True)


bnn_hip.set_math("bf16")
with torch.no_grad():
    for lr in (False, True):
        case = f"784-1200-1200-10 B128 {'LR' if lr else 'BBB'}"
        net = net_of((784, 1200, 10), "classification", lr, 128)
        x = torch.from_numpy(synth.synth_batch("classification", 128, 784, 10)[0]).to(dev)
        report(case, "net.predictor(x, S).replay()", timed(net.predictor(x, S).replay, 300), "minibatch")
        report(case, "net.predictive_graph(x, S).replay()", timed(net.predictive_graph(x, S).replay, 300), "minibatch")
        report(case, "predictive_graph(capture='calls').replay()", timed(net.predictive_graph(x, S, capture="calls").replay, 300),
               "minibatch")

    case = "1-400-400-1 400 points, 5 quantiles"
    net = net_of((1, 400, 1), "regression", False, 400)
    x = torch.from_numpy(np.asarray(synth.synth_batch("regression", 400, 1, 1)[0], np.float32).reshape(400, 1)).to(dev)
    chain = engine.GraphedElbo(net, x, torch.zeros((400, 1), device=dev), S, sigma=0.1)
    report(case, "launch chain alone (GraphedElbo.replay())", timed(chain.replay, 300), "evaluation")
    g = net.predictive_graph(x, S, quantiles=[0, .25, .5, .75, 1], sigma=0.1)
    report(case, "net.predictive_graph(x, S, quantiles).replay()", timed(g.replay, 300), "evaluation")

    G = 78
    case = f"784-1200-1200-10 {G} x 128 rows BBB"
    net = net_of((784, 1200, 10), "classification", False, 128)
    xs = torch.stack([torch.from_numpy(synth.synth_batch("classification", 128, 784, 10, seed=70 + m)[0]).view(128, 784)
                      for m in range(G)]).to(dev)
    pred = net.predictor(xs[0], S)

    def walk():
        for m in range(G):
            pred.x.copy_(xs[m])
            pred.replay()
    report(case, f"{G} x (copy into .x + net.predictor replay)", timed(walk, 10, G), "minibatch")
    st = net.predictive_graph(xs, S, stacked=True)
    report(case, "net.predictive_graph(xs, S, stacked=True)", timed(st.replay, 30, G), "minibatch")
print(json.dumps(rows))
