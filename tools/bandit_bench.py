"""F5 measurement: one bandit step at RLConfig shapes (119-100-100-1, mixture prior, n_samples 2, batch 64, buffer 4096,
64 minibatches per step) in the steady state (l >= buffer_size: every step trains on all 64 minibatches).
  - device loop (bnn_hip.bandit.BNNBandit, hipGraphs): per step, the device-timeline time of the decision (rows + forward +
    act), the replay kernels (sort + gather) and the training pass (64 GraphedTrainStep replays), from events recorded
    between the parts (no synchronisation inside the loop), and the wall time per step;
  - eager: Bandit.update of base_bandit.py:75-99 restated on the drop-in network (batch-1 decision forwards ending in
    .item(), Python lists, numpy permutation, torch.Tensor(list) of the pool, 64 sample_elbo + backward + Adam steps),
    over ~20 steps from a full buffer.
The device bandit is fast-forwarded to the steady state by setting its step word (the ring then holds context 0).
Prints one line per part, then the rows as JSON.
usage: python tools/bandit_bench.py [steps] [policy]"""
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
from bnn_hip import bandit, synth  # noqa: E402

dev = torch.device("cuda:0")
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
POLICY = sys.argv[2] if len(sys.argv) > 2 else "thompson"
PARAMS = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-4, hidden_units=100, mode="regression", mixture_prior=True,
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, -0, -6], n_samples=2, epsilon=0.0)

x, y = synth.mushroom_like(8124, 1)
rows = []


def device_loop():
    W = PARAMS["buffer_size"]
    b = bandit.BNNBandit("bench", PARAMS, x, y, policy=POLICY, max_steps=W + STEPS + 10)
    b.step_word.fill_(W)                 # steady state: l >= buffer_size from the first measured step on
    b.t = W
    seq = np.random.RandomState(2).randint(0, len(x), STEPS + 5)
    for i in seq[:5]:                    # settle
        b.update(int(i))
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(STEPS)]
    t0 = time.perf_counter()
    for k, i in enumerate(seq[5:]):
        e = ev[k]
        b.indices[b.t].fill_(int(i))
        e[0].record()
        b.train._shared.sync()
        b.g_decide.replay()
        b.train._shared.advance(b.dec_samples) if POLICY == "thompson" else None
        e[1].record()
        b.g_replay.replay()
        e[2].record()
        for j in range(bandit.n_batches(b.t, b.batch_size, b.buffer_size)):
            b.train.step(b.slab[j], b.targets[j], bandit.beta(j, b.num_batches))
        b.scheduler.step()
        b.t += 1
        e[3].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / STEPS * 1e6
    parts = np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3])] for e in ev]) * 1e3
    med = np.median(parts, axis=0)
    for name, v in zip(("decision", "replay kernels", "training (64 steps)"), med):
        rows.append(dict(path="device", part=name, us_per_step=round(float(v), 1)))
    rows.append(dict(path="device", part="wall per step", us_per_step=round(wall, 1)))


def eager_loop(steps=20):
    """base_bandit.py:37-99 + bandits.py:39-51 on the drop-in network (torch.optim.Adam, as bandits.py:36)."""
    mp = dict(input_shape=x.shape[1] + 2, classes=1, batch_size=64, hidden_units=100, mode="regression", mixture_prior=True,
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, -0, -6], local_reparam=False)
    net = networks.BayesianNetwork(mp).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    bs, W, M, S = 64, 4096, 64, 2
    rs = np.random.RandomState(3)
    buffer_x = [np.concatenate((x[i], [1, 0])) for i in rs.randint(0, len(x), W)]
    buffer_y = [0.0] * W
    t_dec = t_pool = t_train = 0.0
    for step in range(steps + 2):
        m = rs.randint(len(x))
        torch.cuda.synchronize()
        a = time.perf_counter()
        context = x[m]
        eat_tuple = torch.FloatTensor(np.concatenate((context, [1, 0]))).unsqueeze(0).to(dev)
        reject_tuple = torch.FloatTensor(np.concatenate((context, [0, 1]))).unsqueeze(0).to(dev)
        with torch.no_grad():
            net.eval()
            reward_eat = sum([net(eat_tuple) for _ in range(S)]).item()
            reward_reject = sum([net(reject_tuple) for _ in range(S)]).item()
        eat = reward_eat > reward_reject
        buffer_x.append(np.concatenate((context, [1, 0] if eat else [0, 1])))
        buffer_y.append(5.0)
        b = time.perf_counter()
        l = len(buffer_x)
        idx_pool = np.random.permutation(list(range(l))[-W:])
        context_pool = torch.Tensor(np.array([buffer_x[i] for i in idx_pool])).to(dev)
        value_pool = torch.Tensor([buffer_y[i] for i in idx_pool]).to(dev).view(-1, 1)
        c = time.perf_counter()
        for i in range(0, len(idx_pool), bs):
            j = i // bs
            beta = 2 ** (M - (j + 1)) / (2 ** M - 1)
            net.train()
            net.zero_grad()
            loss = net.sample_elbo(context_pool[i:i + bs], value_pool[i:i + bs], beta, S)[0]
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        d = time.perf_counter()
        if step >= 2:
            t_dec, t_pool, t_train = t_dec + (b - a), t_pool + (c - b), t_train + (d - c)
    for name, v in (("decision", t_dec), ("replay pool", t_pool), ("training (64 steps)", t_train)):
        rows.append(dict(path="eager", part=name, us_per_step=round(v / steps * 1e6, 1)))
    rows.append(dict(path="eager", part="wall per step", us_per_step=round((t_dec + t_pool + t_train) / steps * 1e6, 1)))


bnn_hip.set_math("bf16")
device_loop()
eager_loop()
for r in rows:
    print(f"{r['path']:7s} {r['part']:22s} {r['us_per_step']:10.1f} us")
print(json.dumps(dict(policy=POLICY, math="bf16", config="119-100-100-1 S=2 bs=64 buffer=4096 nb=64", rows=rows)))
