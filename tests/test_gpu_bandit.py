"""The device contextual bandit (bnn_bandit_rows / _act / _replay, bnn_hip.bandit.BNNBandit): the kernels against numpy
restatements (coins and permutations recomputed with the oracle's Philox), the whole loop against an eager restatement of
Bandit.update (reinforcement_learning/base_bandit.py:75-99, bandits.py:43-51) on a second replica at the same Philox
sample indices, no host synchronisation in update(), run() against update(), and learning on mushroom-like data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import bandit, ops, synth
from oracle import bnn_oracle as O


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_math():
    yield
    bnn_hip.set_math("bf16")


# ---------------------------------------------------------------------------------------------------- numpy restatement
def coins(seed, t):
    """(r0, r1, r2, r3) of the bandit stream at step t: Philox((0, t, 0, 1), seed)."""
    r = O.philox4x32(0, t, 0, 1, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [np.uint32(v) for v in np.asarray(r).reshape(4)]


def u(r):
    return O._u01(np.asarray([r], dtype=np.uint32))[0]


def pick(r, n):
    return min(int(np.floor(np.float32(u(r)) * np.float32(n))), n - 1)


def decide(v):
    """argmax, ties to the highest index."""
    best = max(v)
    return max(a for a in range(len(v)) if v[a] == best)


def act_step(seed, t, v, eps, A):
    r = coins(seed, t)
    a = decide(v)
    if u(r[0]) < np.float32(eps):
        a = pick(r[1], A)
    return a, r


def reward_of(table, k, a, r2):
    hi, lo, thr = table[k][a]
    return np.float32(hi) if u(r2) > np.float32(thr) else np.float32(lo)


def shuffled_pool(seed, l, bs, buf):
    """Pool entries in slab order: positions sorted by (Philox word p & 3 of (p >> 2, t, 1, 1), p)."""
    ent = bandit.pool_entries(l, bs, buf)
    P = len(ent)
    p = np.arange(P, dtype=np.uint32)
    r = np.stack(O.philox4x32(p >> 2, np.uint32(l - 1), 1, 1, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), axis=-1)
    keys = r[np.arange(P), p & 3].astype(np.uint64)
    order = np.argsort((keys << np.uint64(32)) | p.astype(np.uint64), kind="stable")
    return ent[order]


def _act_state(dev, N, d, K, A, S, stride, T, buf, x, y, table, oracle, seed, eps, indices):
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    st = dict(outputs=torch.zeros((S if stride else 1) * A, **f32), step=torch.zeros(1, **i32), cur_index=torch.zeros(1, **i32),
              rows=torch.zeros((A, d + A), **f32), actions=torch.zeros(T, dtype=torch.int64, device=dev), reward_out=torch.zeros(T, **f32),
              regrets=torch.zeros(T + 1, dtype=torch.float64, device=dev), counts=torch.zeros((K, A), dtype=torch.int64, device=dev),
              ring_index=torch.zeros(buf, **i32), ring_action=torch.zeros(buf, **i32), ring_reward=torch.zeros(buf, **f32))
    a = ops.bandit_act_args(x=x, labels=y, rewards=table, oracle=oracle, n_samples=S, output_sample_stride=stride, epsilon=eps, seed=seed,
                            indices=indices, **st)
    return a, st


# ---------------------------------------------------------------------------------------------------- 1. act
@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("A,K", [(2, 2), (5, 3)])
@pytest.mark.parametrize("stride0", [False, True])
def test_bandit_act_matches_numpy(dev, eps, A, K, stride0):
    rs = np.random.RandomState(10 * A + K)
    N, d, S, T, buf = 37, 6, 3, 45, 16                              # 45 steps: the ring wraps twice
    seed = 0x1234_5678_9ABC + A
    xh = rs.randn(N, d).astype(np.float32)
    yh = rs.randint(0, K, N).astype(np.int64)
    tab = np.stack([np.stack([rs.choice([-3.0, 0.0, 2.0, 5.0], 2).tolist() + [rs.uniform(0.2, 0.8)] for _ in range(A)])
                    for _ in range(K)]).astype(np.float32)
    orc = tab[:, :, :2].max(axis=(1, 2)).astype(np.float32)
    idx = np.where(rs.uniform(size=T) < 0.5, rs.randint(0, N, T), -1).astype(np.int64)          # -1: drawn on the device
    x, y = torch.from_numpy(xh).to(dev), torch.from_numpy(yh).to(dev)
    a, st = _act_state(dev, N, d, K, A, S, 0 if stride0 else A, T, buf, x, y, torch.from_numpy(tab).to(dev),
                       torch.from_numpy(orc).to(dev), seed, eps, torch.from_numpy(idx).to(dev))
    regret, counts = [0.0], np.zeros((K, A), np.int64)
    ring = np.zeros((3, buf))
    acts, rews = [], []
    ties = 0
    for t in range(T):
        ops.bandit_rows(a)
        o = (rs.randint(-2, 3, (1 if stride0 else S, A)) * 0.5).astype(np.float32)              # small halves: planted ties
        st["outputs"].copy_(torch.from_numpy(o.reshape(-1)))
        ops.bandit_act(a)
        r = coins(seed, t)
        i = int(idx[t]) if idx[t] >= 0 else pick(r[3], N)
        assert int(st["cur_index"].item()) == i
        rows = st["rows"].cpu().numpy()
        np.testing.assert_array_equal(rows[:, :d], np.broadcast_to(xh[i], (A, d)))
        np.testing.assert_array_equal(rows[:, d:], np.eye(A, dtype=np.float32))
        v = []
        for c in range(A):
            acc = o[0, c]
            for s in range(1, S):
                acc = np.float32(acc + o[0 if stride0 else s, c])
            v.append(acc)
        ties += len(set(v)) < A
        act, _ = act_step(seed, t, v, eps, A)
        k = int(yh[i])
        rw = reward_of(tab, k, act, r[2])
        acts.append(act)
        rews.append(rw)
        regret.append(regret[-1] + (float(orc[k]) - float(rw)))
        counts[k, act] += 1
        ring[:, t % buf] = (i, act, rw)
    assert ties > 0
    assert int(st["step"].item()) == T
    np.testing.assert_array_equal(st["actions"].cpu().numpy(), acts)
    np.testing.assert_array_equal(st["reward_out"].cpu().numpy(), np.asarray(rews, np.float32))
    np.testing.assert_array_equal(st["regrets"].cpu().numpy(), np.asarray(regret))
    np.testing.assert_array_equal(st["counts"].cpu().numpy(), counts)
    np.testing.assert_array_equal(st["ring_index"].cpu().numpy(), ring[0].astype(np.int32))
    np.testing.assert_array_equal(st["ring_action"].cpu().numpy(), ring[1].astype(np.int32))
    np.testing.assert_array_equal(st["ring_reward"].cpu().numpy(), ring[2].astype(np.float32))


# ---------------------------------------------------------------------------------------------------- 2. replay
@pytest.mark.parametrize("l", [1, 5, 63, 64, 65, 127, 1000, 4095, 4096, 4097, 10000])
def test_bandit_replay_matches_the_restatement(dev, l):
    rs = np.random.RandomState(l)
    N, d, A, bs, buf, M = 300, 119 - 2, 2, 64, 4096, 64
    seed = 2026 + l
    xh = rs.randn(N, d).astype(np.float32)
    ring_i = rs.randint(0, N, buf).astype(np.int32)
    ring_a = rs.randint(0, A, buf).astype(np.int32)
    ring_r = rs.randn(buf).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(dev)
    slab = torch.full((M, bs, d + A), -7.0, dtype=torch.float32, device=dev)
    tg = torch.full((M, bs), -7.0, dtype=torch.float32, device=dev)
    nb = torch.full((1,), -1, dtype=torch.int32, device=dev)
    a = ops.bandit_replay_args(x=T(xh), step=torch.tensor([l], dtype=torch.int32, device=dev), ring_index=T(ring_i),
                               ring_action=T(ring_a), ring_reward=T(ring_r), workspace=torch.zeros(buf, dtype=torch.int32, device=dev),
                               slab=slab, targets=tg, batch_size=bs, n_actions=A, seed=seed, n_batches=nb)
    ops.bandit_replay(a)
    ent = shuffled_pool(seed, l, bs, buf)
    P = len(ent)
    slot = ent % buf
    want = np.concatenate([xh[ring_i[slot]], np.eye(A, dtype=np.float32)[ring_a[slot]]], axis=1)
    assert int(nb.item()) == P // bs == bandit.n_batches(l - 1, bs, buf)
    got = slab.view(-1, d + A).cpu().numpy()
    np.testing.assert_array_equal(got[:P], want)
    np.testing.assert_array_equal(tg.view(-1).cpu().numpy()[:P], ring_r[slot])
    assert (got[P:] == -7.0).all()                                                # rows past the pool untouched
    if l > 1:
        assert sorted(ent.tolist()) == sorted(bandit.pool_entries(l, bs, buf).tolist())
        assert ent.tolist() != bandit.pool_entries(l, bs, buf).tolist()           # shuffled


# ---------------------------------------------------------------------------------------------------- 3. end to end
SMALL = dict(buffer_size=32, batch_size=8, num_batches=4, lr=1e-3, hidden_units=16, mode="regression", mixture_prior=True,
             mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.2)


def _eager_replay(b, params, state0, xh, yh, idx, policy, local_reparam, seed, eps_seed, snaps, dev):
    """Bandit.update restated eagerly on a replica: reference-shaped forwards, numpy coins / pool, sample_elbo + FusedAdam
    (not capturable) + StepLR.  Returns the number of steps whose decision was compared."""
    import networks
    from bnn_hip.optim import FusedAdam
    mp = dict(input_shape=xh.shape[1] + 2, classes=1, batch_size=params["batch_size"], hidden_units=params["hidden_units"],
              mode="regression", mixture_prior=params["mixture_prior"], mu_init=params["mu_init"], rho_init=params["rho_init"],
              prior_init=params["prior_init"], local_reparam=local_reparam)
    net = networks.BayesianNetwork(mp).to(dev)
    net.load_state_dict(state0)
    opt = FusedAdam(net.parameters(), lr=params["lr"])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=5000, gamma=0.5)
    S, bs, buf, M = params["n_samples"], params["batch_size"], params["buffer_size"], params["num_batches"]
    tab = np.asarray(bandit.MUSHROOM.rewards, np.float32)
    bnn_hip.manual_seed(eps_seed, counter=0)
    buffer, regret = [], [0.0]
    acts_dev, rews_dev = b.history()
    regrets_dev = b.cumulative_regrets
    for t, i in enumerate(idx):
        rows = torch.from_numpy(np.concatenate([np.broadcast_to(xh[i], (2, xh.shape[1])), np.eye(2, dtype=np.float32)], 1)).to(dev)
        net.eval()
        with torch.no_grad():
            outs = [net(rows)] * S if policy == "mean" else list(net.forward_mc(rows, S))
            v = outs[0]
            for o in outs[1:]:
                v = v + o                                                         # Python's sum of the S outputs
        v = v.view(-1).cpu().numpy()
        if abs(float(v[0]) - float(v[1])) < 1e-4 * max(abs(float(v[0])), abs(float(v[1])), 1e-30):
            return t                                                              # margin too thin to compare on
        a, r = act_step(seed, t, list(v), params["epsilon"], 2)
        k = int(yh[i])
        rw = reward_of(tab, k, a, r[2])
        assert a == int(acts_dev[t]) and rw == rews_dev[t], t
        regret.append(regret[-1] + (float(bandit.MUSHROOM.oracle[k]) - float(rw)))
        assert regret[-1] == regrets_dev[t + 1], t
        buffer.append((i, a, rw))
        ent = shuffled_pool(seed, t + 1, bs, buf)
        xb = np.stack([np.concatenate([xh[buffer[e][0]], np.eye(2, dtype=np.float32)[buffer[e][1]]]) for e in ent])
        yb = np.asarray([buffer[e][2] for e in ent], np.float32).reshape(-1, 1)
        net.train()
        for j in range(len(ent) // bs):
            opt.zero_grad()
            elbo = net.sample_elbo_lr if local_reparam else net.sample_elbo
            loss = elbo(torch.from_numpy(xb[j * bs:(j + 1) * bs]).to(dev), torch.from_numpy(yb[j * bs:(j + 1) * bs]).to(dev),
                        bandit.beta(j, M), S)[0]
            loss.backward()
            opt.step()
        sched.step()
        for (name, p), q in zip(net.state_dict().items(), snaps[t]):
            assert float((p - q).abs().max()) <= 2e-5 * float(p.abs().max()), (t, name)
    return len(idx)


@pytest.mark.parametrize("policy,local_reparam", [("mean", False), ("mean", True), ("thompson", False)])
def test_bandit_end_to_end_equals_eager_restatement(dev, policy, local_reparam):
    bnn_hip.set_math("f32")
    rs = np.random.RandomState(5)
    N, d, steps = 64, 10, 40
    xh = rs.uniform(0, 1, (N, d)).astype(np.float32)
    yh = rs.randint(0, 2, N).astype(np.int64)
    idx = rs.randint(0, N, steps)
    seed, eps_seed = 777, 4242
    params = dict(SMALL, prior_init=[1.0], mixture_prior=False) if local_reparam else SMALL   # (LR layers: a Gaussian prior)
    torch.manual_seed(3)
    bnn_hip.manual_seed(eps_seed, counter=0)
    b = bandit.BNNBandit("e2e", params, xh, yh, policy=policy, seed=seed, max_steps=steps, local_reparam=local_reparam)
    state0 = {k: v.clone() for k, v in b.net.state_dict().items()}
    snaps = []
    for i in idx:
        b.update(int(i))
        snaps.append([v.clone() for v in b.net.state_dict().values()])
    compared = _eager_replay(b, params, state0, xh, yh, idx, policy, local_reparam, seed, eps_seed, snaps, dev)
    print(f"{policy} lr={local_reparam}: compared {compared} of {steps} steps")
    assert compared >= 20
    assert b.t == steps and len(b.cumulative_regrets) == steps + 1
    c = b.counts
    assert c.sum() == steps and (b.tp, b.fn, b.fp, b.tn) == (c[1, 0], c[1, 1], c[0, 0], c[0, 1])


# ---------------------------------------------------------------------------------------------------- 4.-5.
def test_bandit_update_does_not_synchronise(dev):
    x, y = synth.mushroom_like(256, 11)
    b = bandit.BNNBandit("nosync", dict(SMALL, hidden_units=32), x, y, policy="thompson", seed=5, max_steps=60)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(50):
            b.update(t % 256 if t % 3 else None)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert b.t == 50 and len(b.cumulative_regrets) == 51


def test_bandit_run_equals_updates(dev):
    x, y = synth.mushroom_like(200, 12)
    seq = np.random.RandomState(13).randint(0, 200, 70)         # 70 steps: past the 32-entry buffer
    out = []
    for mode in ("update", "run"):
        torch.manual_seed(21)
        bnn_hip.manual_seed(99, counter=0)
        b = bandit.BNNBandit(mode, dict(SMALL, hidden_units=32), x, y, policy="thompson", seed=8, max_steps=80,
                             capture=True if mode == "update" else "calls")
        if out:
            b.net.load_state_dict(out[0][0])
        state0 = {k: v.clone() for k, v in b.net.state_dict().items()}
        if mode == "update":
            for i in seq:
                b.update(int(i))
        else:
            b.run(seq)
        out.append((state0, b.net.state_dict(), b.history(), b.cumulative_regrets, b.counts))
    (s0a, pa, ha, ra, ca), (s0b, pb, hb, rb, cb) = out
    for k in pa:
        assert torch.equal(s0a[k], s0b[k]) and torch.equal(pa[k], pb[k]), k
    assert np.array_equal(ha[0], hb[0]) and np.array_equal(ha[1], hb[1]) and ra == rb and np.array_equal(ca, cb)


# ---------------------------------------------------------------------------------------------------- 6. learning
def test_bandit_learns_on_mushroom_like_data(dev):
    bnn_hip.set_math("bf16")
    x, y = synth.mushroom_like(2000, 17)
    params = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression",
                  mixture_prior=True, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.0)
    torch.manual_seed(0)
    bnn_hip.manual_seed(2026, counter=0)
    b = bandit.BNNBandit("learn", params, x, y, policy="thompson", seed=31, max_steps=1000)
    b.run(np.random.RandomState(32).randint(0, 2000, 1000))
    R = b.cumulative_regrets
    last = (R[1000] - R[800]) / 200
    print(f"mean regret of the last 200 steps: {last:.3f} (uniform-random agent: 5.0); tp fn fp tn = {b.tp} {b.fn} {b.fp} {b.tn}")
    assert last <= 0.4 * 5.0
