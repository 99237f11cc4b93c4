"""The grouped Thompson-sampling BNN bandits (include/bnn_hip.h F7, bnn_hip.bandit.BNNBanditGroup): the training launch
against the drop-in's eager sample_elbo + backward + Adam loop at the same Philox sample indices, the decision forward
against forward_mc / the eval forward, a group against its agents run one by one and graph replay against eager launches
(bit for bit), the whole loop against BNNBandit, no host synchronisation in update() / run(), and learning on
mushroom-like data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import networks
from bnn_hip import _lib as L
from bnn_hip import bandit, ops, synth
from bnn_hip.optim import FusedAdam
from oracle import bnn_oracle as O

# Both sides of comparisons 1, 2 and 4 are fp32 with different summation orders.  The bound is 4 x the deviation of the
# reference side against itself in another order (two independent orderings on each side of the comparison, and a factor 2
# for the chain's growth between seeds), and never more than F6's 2e-4 of a tensor's scale.  Measured on an MI355X on the
# inputs of test 1 (f32 math), train.GraphedTrainStep's hand-chained kernels against the eager autograd loop, largest
# deviation over the twelve tensors relative to each tensor's max |.|: 64 minibatches at 119-100-100-1 (mixture prior, S 2)
# parameters 2.13e-7, exp_avg 5.97e-7, exp_avg_sq 1.15e-7; 3 minibatches at 37-19-19-1 (Gaussian prior, S 3) 7.5e-8, 2.1e-8,
# 9.0e-9.  (Switching state.form between AUTO and TILE changes no bit at these shapes: both take the same kernels.)
REF_SELF = 5.97e-7
TOL = min(4 * REF_SELF, 2e-4)          # 2.4e-6 of a tensor's scale
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_math():
    yield
    bnn_hip.set_math("bf16")


def _bnn(I, H, dev, seed, prior_init, mixture):
    torch.manual_seed(seed)
    mp = dict(input_shape=I, classes=1, batch_size=1, hidden_units=H, mode="regression", mixture_prior=mixture,
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=prior_init, local_reparam=False)
    return networks.BayesianNetwork(mp).to(dev)


class _Launch:
    """One agent's bnn_bbb_group_train / _fwd blocks over a BayesianNetwork and plain device tensors."""

    def __init__(self, net, slab, targets, dev, lr, S, eps_seed, counter, kl_weights=(), rows=None, mean=False):
        self.params = [p.detach() for p in net.parameters()]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.nbw = torch.tensor([slab.shape[0]], dtype=torch.int32, device=dev)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)
        self.counter = torch.tensor([counter], dtype=torch.int32, device=dev)
        I, H = net.input_shape, net.hidden_units
        self.ws = torch.zeros(ops.bbb_group_workspace_bytes(I, H) // 4, dtype=torch.float32, device=dev)
        self.out = None if rows is None else torch.zeros((1 if mean else S, rows.shape[0]), dtype=torch.float32, device=dev)
        ag = ops.bbb_group_agent(params=self.params, exp_avg=self.m, exp_avg_sq=self.v, step=self.step, lr=self.lr, slab=slab,
                                 targets=targets, n_batches=self.nbw, loss_info=self.loss, rows=rows, outputs=self.out,
                                 sample_counter=self.counter, workspace=self.ws, eps_seed=eps_seed,
                                 eps_mode=L.EPS_ZERO if mean else L.EPS_PHILOX)
        shape = dict(in_features=I, hidden=H, n_samples=S, device=dev, prior=net.l1._prior_spec)
        if len(kl_weights):
            self.train = ops.bbb_group_args([ag], batch=slab.shape[1], max_batches=slab.shape[0], kl_weights=kl_weights, **shape)
        if rows is not None:
            self.fwd = ops.bbb_group_args([ag], n_rows=rows.shape[0], **shape)


def _close(a, b, rel, what=""):
    scale = float(b.abs().max())
    dev_ = float((a - b).abs().max())
    print(f"    {what}: deviation {dev_ / max(scale, 1e-30):.3e} of the scale {scale:.3e} (bound {rel:.1e})")
    assert dev_ <= rel * max(scale, 1e-30), (what, dev_, scale)


def _stat_terms(sd, prior_init, mixture, eps_seed, first, S):
    """fp64 sum |term| of log q and of log p, averaged over draws first .. first + S - 1 of the network `sd` (CPU fp32
    tensors), with the device's epsilon restated by the oracle: what the two statistics are compared relative to."""
    c0 = -0.9189385332046727
    lq = lp = 0.0
    for s in range(S):
        for li, name in enumerate(("l1", "l2", "l3")):
            for kind, pre in enumerate(("weight", "bias")):
                mu, rho = sd[f"{name}.{pre}_mu"].double().numpy(), sd[f"{name}.{pre}_rho"].double().numpy()
                shape = mu.shape if kind == 0 else (1, mu.shape[0])
                e = O.philox_normal(eps_seed, O.tensor_id(li, kind), first + s, *shape).astype(np.float64).reshape(mu.shape)
                sg = np.log1p(np.exp(rho))
                w = mu + sg * e
                lq += np.abs(c0 - np.log(sg) - e * e / 2).sum()
                if mixture:
                    pi, s1, s2 = prior_init[0], np.exp(prior_init[1]), np.exp(prior_init[2])
                    d1 = np.exp(c0 - np.log(s1) - w * w / (2 * s1 * s1))
                    d2 = np.exp(c0 - np.log(s2) - w * w / (2 * s2 * s2))
                    lp += np.abs(np.log(pi * d1 + (1 - pi) * d2)).sum()
                else:
                    sp = prior_init[0]
                    lp += np.abs(c0 - np.log(sp) - w * w / (2 * sp * sp)).sum()
    return lq / S, lp / S


# ---------------------------------------------------------------------------------------------------- 1. vs the drop-in
@pytest.mark.parametrize("I,H,B,nb,S,prior_init,mixture", [(119, 100, 64, 64, 2, [0.5, 0, -6], True),
                                                            (37, 19, 8, 3, 3, [1.0], False)])
def test_training_launch_matches_the_dropin(dev, I, H, B, nb, S, prior_init, mixture):
    bnn_hip.set_math("f32")
    g = torch.Generator().manual_seed(I + nb)
    slab = torch.rand((nb, B, I), generator=g).to(dev)
    targets = (torch.randn((nb, B), generator=g) * 5).to(dev)
    net = _bnn(I, H, dev, 1, prior_init, mixture)
    ref = _bnn(I, H, dev, 1, prior_init, mixture)
    opt = FusedAdam(ref.parameters(), lr=1e-3)
    eps_seed, c = 4242 + I, 7
    betas = [bandit.beta(j, nb) for j in range(nb)]
    run = _Launch(net, slab, targets, dev, 1e-3, S, eps_seed, c, kl_weights=betas)
    ops.bbb_group_train(run.train)
    bnn_hip.manual_seed(eps_seed, counter=c)
    ref.train()
    before_last = None
    for j in range(nb):
        if j == nb - 1:
            before_last = {k: v.detach().cpu().clone() for k, v in ref.state_dict().items()}
        opt.zero_grad()
        info = ref.sample_elbo(slab[j], targets[j].view(B, 1), betas[j], S)
        info[0].backward()
        opt.step()
    torch.cuda.synchronize()
    print(f"  {I}-{H}-{H}-1, batch {B}, {nb} minibatches, S = {S}")
    for (name, q), p, m, v in zip(ref.named_parameters(), run.params, run.m, run.v):
        _close(p, q.detach(), TOL, name)
        _close(m, opt.state[q]["exp_avg"], TOL, name + " exp_avg")
        _close(v, opt.state[q]["exp_avg_sq"], TOL, name + " exp_avg_sq")
    assert int(run.step) == nb and int(run.counter) == c + nb * S
    # loss_info = (loss, mean log_p, mean log_q, mean nll) of the last minibatch.  The statistics are sums of ~P terms:
    # compared relative to sum |term| (fp64, here).  Each side's deepest accumulator chain is at most 64 additions (the
    # launch: ceil(P / 512) = 44 terms per thread, then 6 + 8 tree levels), so a side's sum is off by at most 64 u sum|term|,
    # u = 2^-24: 64 ULP for the two; and a parameter deviation of TOL moves every term by about TOL |term|.
    sum_q, sum_p = _stat_terms(before_last, prior_init, mixture, eps_seed, c + (nb - 1) * S, S)
    loss, lp, lq, nll = [float(v) for v in run.loss.tolist()]
    r_loss, r_lp, r_lq, r_nll = [float(v.detach()) for v in info]
    tol_q, tol_p = (64 * ULP + TOL) * sum_q, (64 * ULP + TOL) * sum_p
    tol_nll = 1e-4 * abs(r_nll)                                  # F6's bound on its loss after the same chain of steps
    print(f"    log_q {lq:.6f} vs {r_lq:.6f} (bound {tol_q:.3e}); log_p {lp:.6f} vs {r_lp:.6f} (bound {tol_p:.3e}); "
          f"nll {nll:.6f} vs {r_nll:.6f} (bound {tol_nll:.3e}); loss {loss:.6f} vs {r_loss:.6f}")
    assert abs(lq - r_lq) <= tol_q and abs(lp - r_lp) <= tol_p and abs(nll - r_nll) <= tol_nll
    assert abs(loss - r_loss) <= betas[-1] * (tol_q + tol_p) + tol_nll


# ---------------------------------------------------------------------------------------------------- 2. decision forward
@pytest.mark.parametrize("I,H,A,S,prior_init,mixture", [(119, 100, 2, 2, [0.5, 0, -6], True), (37, 19, 5, 3, [1.0], False)])
def test_decision_forward_matches_the_dropin(dev, I, H, A, S, prior_init, mixture):
    bnn_hip.set_math("f32")
    rows = torch.rand((A, I), generator=torch.Generator().manual_seed(A)).to(dev)
    net = _bnn(I, H, dev, 3, prior_init, mixture)
    eps_seed, c = 999 + A, 11
    zero = (torch.zeros((1, 1, I), device=dev), torch.zeros((1, 1), device=dev))
    run = _Launch(net, *zero, dev, 1e-3, S, eps_seed, c, rows=rows)
    ops.bbb_group_fwd(run.fwd)
    bnn_hip.manual_seed(eps_seed, counter=c)
    net.eval()
    with torch.no_grad():
        want = net.forward_mc(rows, S).view(S, A)
    _close(run.out, want, TOL, f"thompson {I}-{H} A={A}")
    assert int(run.counter) == c                                 # read, not advanced: bnn_bandit_act advances it
    assert float((want[0] - want[1]).abs().max()) > 0            # the draws differ
    mean = _Launch(net, *zero, dev, 1e-3, S, eps_seed, c, rows=rows, mean=True)
    ops.bbb_group_fwd(mean.fwd)
    with torch.no_grad():
        want = net(rows).view(1, A)
    _close(mean.out, want, TOL, f"mean {I}-{H} A={A}")


# ---------------------------------------------------------------------------------------------------- 3. grouping, capture
SMALL = dict(buffer_size=128, batch_size=16, num_batches=8, lr=1e-3, hidden_units=24, mode="regression", mixture_prior=True,
             mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.0)
EPS, SEEDS, EPS_SEEDS = [0.0, 0.05, 0.01, 0.2], [11, 12, 13, 14], [101, 102, 103, 104]
POLICIES = ["thompson", "thompson", "mean", "thompson"]


def _snapshot(grp, g):
    view = grp[g]
    a, r = view.history()
    opt = view.optimiser
    qs = list(view.net.parameters())
    return dict(actions=a, rewards=r, regrets=np.asarray(view.cumulative_regrets), counts=view.counts,
                params=[p.detach().cpu().clone() for p in qs], m=[opt.state[q]["exp_avg"].cpu().clone() for q in qs],
                v=[opt.state[q]["exp_avg_sq"].cpu().clone() for q in qs], counter=view.sample_counter,
                step=opt.device_step(), loss=np.asarray(view.loss_info, np.float32))


def _same(x, y):
    assert x.keys() == y.keys()
    for k in x:
        u, v = x[k], y[k]
        if isinstance(u, list):
            assert all(torch.equal(p, q) for p, q in zip(u, v)), k
        else:
            assert np.array_equal(np.asarray(u), np.asarray(v)), k


def _run_group(x, y, idx, sel, states, capture=True):
    grp = bandit.BNNBanditGroup("g", SMALL, x, y, seeds=[SEEDS[g] for g in sel], eps_seeds=[EPS_SEEDS[g] for g in sel],
                                epsilons=[EPS[g] for g in sel], policy=[POLICIES[g] for g in sel], max_steps=len(idx),
                                capture=capture)
    assert len(grp) == len(sel)
    for k, g in enumerate(sel):
        grp.nets[k].load_state_dict(states[g])
    for t, i in enumerate(idx):
        grp.update(None if t % 7 == 3 else int(i))              # some steps draw their context on the device
    return [_snapshot(grp, k) for k in range(len(sel))]


def test_grouping_changes_nothing_and_graph_equals_eager(dev):
    x, y = synth.mushroom_like(300, 21)
    idx = np.random.RandomState(22).randint(0, 300, 300)      # 300 steps: l <= bs, bs < l < buffer, the full ring
    states = [{k: v.clone() for k, v in _bnn(x.shape[1] + 2, SMALL["hidden_units"], dev, 30 + g, SMALL["prior_init"],
                                             True).state_dict().items()} for g in range(4)]
    together = _run_group(x, y, idx, [0, 1, 2, 3], states)
    for g in range(4):
        alone = _run_group(x, y, idx, [g], states)[0]
        _same(together[g], alone)
    eager = _run_group(x, y, idx, [0, 1, 2, 3], states, capture=False)
    calls = _run_group(x, y, idx, [3, 1], states, capture="calls")       # another place in the group, recorded launches
    for g in range(4):
        _same(together[g], eager[g])
    _same(together[3], calls[0])
    _same(together[1], calls[1])
    assert len(set(tuple(s["actions"][:100]) for s in together)) > 1            # the agents did not all act alike
    # a sampled decision takes S indices and every minibatch S; the mean rule's decisions take none
    nbs = sum(bandit.n_batches(t, SMALL["batch_size"], SMALL["buffer_size"]) for t in range(300))
    assert [s["step"] for s in together] == [nbs] * 4
    assert [s["counter"] for s in together] == [2 * nbs + (600 if q == "thompson" else 0) for q in POLICIES]


# ---------------------------------------------------------------------------------------------------- 4. against BNNBandit
E2E = dict(buffer_size=32, batch_size=8, num_batches=4, lr=1e-3, hidden_units=16, mode="regression", mixture_prior=True,
           mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.2)   # test_gpu_bandit.SMALL


def test_end_to_end_equals_bnn_bandit(dev):
    bnn_hip.set_math("f32")
    rs = np.random.RandomState(5)
    N, d, steps = 64, 10, 40
    xh = rs.uniform(0, 1, (N, d)).astype(np.float32)
    yh = rs.randint(0, 2, N).astype(np.int64)
    idx = rs.randint(0, N, steps)
    seeds, eps_seeds, policies = [777, 778, 779], [4242, 4243, 4244], ["thompson", "thompson", "mean"]
    torch.manual_seed(3)
    grp = bandit.BNNBanditGroup("e2e", E2E, xh, yh, seeds=seeds, eps_seeds=eps_seeds, policy=policies, max_steps=steps)
    state0 = [{k: v.clone() for k, v in grp[g].net.state_dict().items()} for g in range(3)]
    snaps = []
    for i in idx:
        grp.update(int(i))
        snaps.append([[v.clone() for v in grp[g].net.state_dict().values()] for g in range(3)])
    S = E2E["n_samples"]
    for g in range(3):
        view = grp[g]
        acts, rews = view.history()
        regrets = view.cumulative_regrets
        # one BNNBandit after the other, each to its last step: the eps key and the host's sample counter are process-wide
        bnn_hip.manual_seed(eps_seeds[g], counter=0)
        b = bandit.BNNBandit("ref", E2E, xh, yh, policy=policies[g], seed=seeds[g], max_steps=steps)
        b.net.load_state_dict(state0[g])
        compared, worst = steps, 0.0
        for t, i in enumerate(idx):
            b.update(int(i))
            out = b.h[-1].view(b.dec_samples, 2).cpu().numpy()
            outs = [out[0]] * S if policies[g] == "mean" else list(out)
            v = outs[0]
            for o in outs[1:]:
                v = v + o
            if abs(float(v[0]) - float(v[1])) < 1e-4 * max(abs(float(v[0])), abs(float(v[1])), 1e-30):
                compared = t                                                  # margin too thin to compare on
                break
            ra, rr = b.history()
            assert int(ra[t]) == int(acts[t]) and rr[t] == rews[t], (g, t)
            assert b.cumulative_regrets[t + 1] == regrets[t + 1], (g, t)
            worst = 0.0
            for (name, p), q in zip(b.net.state_dict().items(), snaps[t][g]):
                dv = float((p - q).abs().max()) / float(p.abs().max())
                worst = max(worst, dv)
                assert dv <= TOL, (g, t, name, dv)
        print(f"  agent {g} ({policies[g]}): compared {compared} of {steps} steps; last compared step's largest "
              f"parameter deviation {worst:.3e} of max |p| (bound {TOL:.1e})")
        assert compared >= 20, (g, compared)
        if compared == steps:
            assert view.sample_counter == (b.train._shared["mirror"] & 0xFFFFFFFF)
    assert grp.t == steps
    c = grp[0].counts
    assert c.sum() == steps and (grp[0].tp, grp[0].fn, grp[0].fp, grp[0].tn) == (c[1, 0], c[1, 1], c[0, 0], c[0, 1])


# ---------------------------------------------------------------------------------------------------- 5. no synchronisation
def test_update_and_run_do_not_synchronise(dev):
    x, y = synth.mushroom_like(256, 11)
    grp = bandit.BNNBanditGroup("nosync", SMALL, x, y, seeds=[1, 2, 3], policy=["thompson", "mean", "thompson"], max_steps=110)
    seq = np.random.RandomState(4).randint(0, 256, 50)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(50):
            grp.update(t % 256 if t % 3 else None)
        grp.run(seq)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert grp.t == 100 and len(grp[2].cumulative_regrets) == 101
    assert len(grp[1].loss_info) == 4 and all(np.isfinite(grp[1].loss_info))


def test_run_equals_updates(dev):
    x, y = synth.mushroom_like(200, 12)
    idx = np.random.RandomState(13).randint(0, 200, 150)        # past the 128-entry buffer
    states = [{k: v.clone() for k, v in _bnn(x.shape[1] + 2, SMALL["hidden_units"], dev, 40 + g, SMALL["prior_init"],
                                             True).state_dict().items()} for g in range(2)]

    def go(use_run):
        grp = bandit.BNNBanditGroup("r", SMALL, x, y, seeds=SEEDS[:2], eps_seeds=EPS_SEEDS[:2], epsilons=EPS[:2], max_steps=150)
        for k in range(2):
            grp.nets[k].load_state_dict(states[k])
        if use_run:
            grp.run(idx)
        else:
            for i in idx:
                grp.update(int(i))
        return [_snapshot(grp, k) for k in range(2)]
    a, b = go(False), go(True)
    for k in range(2):
        _same(a[k], b[k])


# ---------------------------------------------------------------------------------------------------- 6. learning
def test_bnn_agents_learn_on_mushroom_like_data(dev):
    x, y = synth.mushroom_like(2000, 17)
    params = dict(buffer_size=4096, batch_size=64, num_batches=64, lr=1e-3, hidden_units=100, mode="regression",
                  mixture_prior=True, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[0.5, 0, -6], n_samples=2, epsilon=0.0)
    torch.manual_seed(0)
    grp = bandit.BNNBanditGroup("learn", params, x, y, seeds=[31, 32, 33, 34], eps_seeds=[2026, 2027, 2028, 2029],
                                policy="thompson", max_steps=1000)
    grp.run(np.random.RandomState(32).randint(0, 2000, 1000))
    lasts = []
    for g in range(4):
        v = grp[g]
        R = v.cumulative_regrets
        lasts.append((R[1000] - R[800]) / 200)
        print(f"  agent {g}: mean regret of the last 200 steps {lasts[-1]:.3f} (uniform-random agent: 5.0); tp fn fp tn = "
              f"{v.tp} {v.fn} {v.fp} {v.tn}; loss_info {v.loss_info}")
    assert all(last <= 0.4 * 5.0 for last in lasts), lasts
