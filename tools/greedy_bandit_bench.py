"""F6 measurement: microseconds per update of epsilon-greedy MLP bandits at RLConfig shapes (119-100-100-1, batch 64,
buffer 4096, Adam) in the steady state (l >= buffer_size: every update trains on all 64 minibatches).
  (a) eager torch: Greedy_Bandit's update restated here (batch-1 decision forwards ending in .item(), then 64 minibatches
      of forward, mse_loss(sum), backward, torch.optim.Adam.step());
  (b) one agent, its 64 minibatch steps as 64 replays of the K6 training graph (GraphedDenseTrainStep), glued the way
      BNNBandit glues GraphedTrainStep (training only: no decision);
  (c) bnn_hip.bandit.GreedyBanditGroup, the whole update (6 launches, one hipGraph) at G = 1, 3, 16, 64, 256;
  and the main-loop step of the four-agent experiment (main.py:70-104): BNNBandit (mean rule, n_samples 2) plus a 3-agent
  group, against BNNBandit plus three eager agents (a).
Device-timeline time from torch.cuda.Event pairs around `--steps` updates after `--warmup` untimed ones, median of
`--reps` groups.  The device loops are fast-forwarded to the steady state by setting their step words (the rings then hold
random contexts).  Prints one line per row, then the rows as JSON.
usage: python tools/greedy_bandit_bench.py [--steps K] [--warmup W] [--reps R] [--groups 1,3,16,64,256]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bnn_hip  # noqa: E402
import networks  # noqa: E402
from bnn_hip import bandit, synth  # noqa: E402
from bnn_hip.optim import FusedAdam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--groups", default="1,3,16,64,256")
args = ap.parse_args()

dev = torch.device("cuda:0")
PARAMS = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression", epsilon=0.0,
              n_samples=1)
BNN_PARAMS = dict(PARAMS, mixture_prior=True, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, -0, -6], n_samples=2)
BUF, BS, NB = PARAMS["buffer_size"], PARAMS["batch_size"], PARAMS["buffer_size"] // PARAMS["batch_size"]
x, y = synth.mushroom_like(8124, 1)
D = x.shape[1] + 2
rows = []


def timed(step):
    """Median over reps of the device time of args.steps calls of step(i), in us per call."""
    seq = np.random.RandomState(2).randint(0, len(x), args.warmup + args.reps * args.steps)
    for i in seq[:args.warmup]:
        step(int(i))
    torch.cuda.synchronize()
    per = []
    for r in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in seq[args.warmup + r * args.steps:args.warmup + (r + 1) * args.steps]:
            step(int(i))
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / args.steps)
    return float(np.median(per))


def report(name, us, **kw):
    row = dict(name=name, us_per_update=round(us, 1), **kw)
    rows.append(row)
    print(f"{name:48s} {us:12.1f} us", kw if kw else "")


class EagerGreedy:
    """(a): Greedy_Bandit's update, restated: decision forwards with .item(), then the 64 training minibatches."""

    def __init__(self, seed):
        torch.manual_seed(seed)
        self.net = networks.MLP(dict(input_shape=D, classes=1, batch_size=BS, hidden_units=100, mode="regression")).to(dev)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=PARAMS["lr"])
        g = torch.Generator().manual_seed(seed)
        self.pool_x = torch.rand((BUF, D), generator=g).to(dev)
        self.pool_y = torch.randn(BUF, generator=g).to(dev)
        self.xt = torch.from_numpy(x).to(dev)

    def update(self, i):
        ctx = self.xt[i]
        with torch.no_grad():
            eat = self.net(torch.cat([ctx, torch.tensor([1., 0.], device=dev)]).view(1, -1)).item()
            rej = self.net(torch.cat([ctx, torch.tensor([0., 1.], device=dev)]).view(1, -1)).item()
        _ = eat > rej
        perm = torch.from_numpy(np.random.permutation(BUF)).to(dev)
        cx, cy = self.pool_x[perm], self.pool_y[perm]
        for j in range(0, BUF, BS):
            self.net.train()
            self.net.zero_grad()
            loss = torch.nn.functional.mse_loss(self.net(cx[j:j + BS]).squeeze(), cy[j:j + BS], reduction="sum")
            loss.backward()
            self.opt.step()


def k6_agent():
    """(b): 64 K6 graph replays per update."""
    bnn_hip.set_math("f32")
    torch.manual_seed(5)
    net = networks.MLP(dict(input_shape=D, classes=1, batch_size=BS, hidden_units=100, mode="regression")).to(dev)
    opt = FusedAdam(net.parameters(), lr=PARAMS["lr"], capturable=True)
    slab = torch.rand((NB, BS, D), device=dev)
    targets = torch.randn((NB, BS), device=dev)
    step = net.graphed_train_step(opt, slab[0], targets[0].contiguous(), loss="mse")

    def update(_i):
        for j in range(NB):
            step.step(slab[j], targets[j])
    return update


def fast_forward(grp):
    grp.step_word.fill_(BUF)
    grp.ring_index.random_(0, len(x))
    grp.ring_action.random_(0, 2)
    grp.t = BUF


def group(G):
    total = args.warmup + args.reps * args.steps
    torch.manual_seed(7)
    grp = bandit.GreedyBanditGroup("bench", PARAMS, x, y, epsilons=[0.0, 0.01, 0.05] * (G // 3) + [0.0] * (G % 3),
                                   max_steps=BUF + total + 2)
    fast_forward(grp)
    return grp


def main():
    eager = EagerGreedy(1)
    report("(a) eager torch, one agent", timed(eager.update))
    report("(b) K6 graph per minibatch, one agent (training)", timed(k6_agent()))
    for G in [int(g) for g in args.groups.split(",")]:
        grp = group(G)
        us = timed(grp.update)
        report(f"(c) GreedyBanditGroup G={G}", us, us_per_agent=round(us / G, 2))
        del grp
        torch.cuda.empty_cache()

    # the four-agent main-loop step
    bnn_hip.set_math("bf16")
    total = args.warmup + args.reps * args.steps
    torch.manual_seed(0)
    b = bandit.BNNBandit("bnn", BNN_PARAMS, x, y, policy="mean", max_steps=BUF + 2 * total + 2)
    b.step_word.fill_(BUF)
    b.t = BUF
    grp = group(3)
    eagers = [EagerGreedy(s) for s in (11, 12, 13)]

    def with_group(i):
        b.update(i)
        grp.update(i)

    def with_eager(i):
        b.update(i)
        for e in eagers:
            e.update(i)
    report("main loop: BNNBandit + 3-agent group", timed(with_group))
    report("main loop: BNNBandit + 3 eager agents", timed(with_eager))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
