"""F7 measurement: microseconds per update of Thompson-sampling BNN bandits at RLConfig shapes (119-100-100-1, batch 64,
buffer 4096, n_samples 2, mixture prior, Adam) in the steady state (l >= buffer_size: every update trains on all 64
minibatches).
  (a) bnn_hip.bandit.BNNBandit, one agent: the decision graph, the replay graph and 64 replays of GraphedTrainStep (f32
      math, the arithmetic the group runs, and bf16 math, its default);
  (b) bnn_hip.bandit.BNNBanditGroup, the whole update (6 launches, one hipGraph) at G = 1, 3, 16, 64, 256;
  and the main-loop step of the four-agent experiment (main.py:70-104): BNNBanditGroup(G = 1) plus a 3-agent greedy group
  against BNNBandit plus the same 3-agent greedy group.
Device-timeline time from torch.cuda.Event pairs around `--steps` updates after `--warmup` untimed ones; the rows are
measured `--reps` times each, interleaved (every row once, then every row again, ...): the median and the (min, max) spread
are reported.  The device loops are fast-forwarded to the steady state by setting their step words (the rings then hold
random contexts).  `--profile G` runs `--steps` steady-state updates of one group of G agents and nothing else (for a kernel
trace).  Prints one line per row, then the rows as JSON.
usage: python tools/bnn_bandit_group_bench.py [--steps K] [--warmup W] [--reps R] [--groups 1,3,16,64,256] [--profile G]"""
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
from bnn_hip import bandit, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--groups", default="1,3,16,64,256")
ap.add_argument("--profile", type=int, default=0)
args = ap.parse_args()

dev = torch.device("cuda:0")
GREEDY = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression", epsilon=0.0,
              n_samples=1)
BNN = dict(GREEDY, mixture_prior=True, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, -0, -6], n_samples=2)
BUF = BNN["buffer_size"]
x, y = synth.mushroom_like(8124, 1)
TOTAL = args.warmup + args.reps * args.steps
SEQ = np.random.RandomState(2).randint(0, len(x), TOTAL)


def fast_forward(b):
    b.step_word.fill_(BUF)
    b.ring_index.random_(0, len(x))
    b.ring_action.random_(0, 2)
    b.t = BUF


def bnn_group(G):
    torch.manual_seed(7)
    grp = bandit.BNNBanditGroup("bench", BNN, x, y, seeds=list(range(100, 100 + G)), max_steps=BUF + TOTAL + 2)
    fast_forward(grp)
    return grp


def greedy_group():
    torch.manual_seed(8)
    grp = bandit.GreedyBanditGroup("greedy", GREEDY, x, y, epsilons=[0.0, 0.01, 0.05], max_steps=BUF + TOTAL + 2)
    fast_forward(grp)
    return grp


def bnn_single(math):
    bnn_hip.set_math(math)
    torch.manual_seed(0)
    b = bandit.BNNBandit("bnn", BNN, x, y, policy="thompson", max_steps=BUF + TOTAL + 2)
    fast_forward(b)
    return b


class Row:
    def __init__(self, name, step, **kw):
        self.name, self.step, self.kw, self.per, self.pos = name, step, kw, [], 0

    def run(self, n, timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in SEQ[self.pos:self.pos + n]:
            self.step(int(i))
        e1.record()
        torch.cuda.synchronize()
        self.pos += n
        if timed:
            self.per.append(e0.elapsed_time(e1) * 1e3 / n)


def main():
    if args.profile:
        grp = bnn_group(args.profile)
        for i in SEQ[:args.steps]:
            grp.update(int(i))
        torch.cuda.synchronize()
        print(f"profiled {args.steps} steady-state updates of a {args.profile}-agent group")
        return
    rows = []
    for math in ("f32", "bf16"):
        b = bnn_single(math)
        rows.append(Row(f"(a) BNNBandit, one agent, {math} math", b.update))
    for G in [int(g) for g in args.groups.split(",")]:
        grp = bnn_group(G)
        rows.append(Row(f"(b) BNNBanditGroup G={G}", grp.update, agents=G))
    one, greedy_a = bnn_group(1), greedy_group()
    single, greedy_b = bnn_single("bf16"), greedy_group()

    def with_group(i):
        one.update(i)
        greedy_a.update(i)

    def with_single(i):
        single.update(i)
        greedy_b.update(i)
    rows.append(Row("main loop: BNNBanditGroup(G=1) + 3-agent greedy group", with_group))
    rows.append(Row("main loop: BNNBandit (bf16) + 3-agent greedy group", with_single))
    for r in rows:
        r.run(args.warmup, False)
    for _ in range(args.reps):                                   # interleaved: every row once per round
        for r in rows:
            r.run(args.steps, True)
    out = []
    for r in rows:
        med, lo, hi = float(np.median(r.per)), min(r.per), max(r.per)
        row = dict(name=r.name, us_per_update=round(med, 1), min=round(lo, 1), max=round(hi, 1))
        if "agents" in r.kw:
            row["us_per_agent"] = round(med / r.kw["agents"], 2)
        out.append(row)
        print(f"{r.name:58s} {med:12.1f} us  (min {lo:.1f}, max {hi:.1f})", f"per agent {row['us_per_agent']}" if "agents" in r.kw else "")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
